/* C ABI of libdcl_attn.so: global multi-head self-attention (reference models/Transformers.py SelfAttention, the block
 * Projector(trans=True) appends) on gfx950 kernels, forward and backward, without an N x N tensor.
 *
 * A third, small library next to the main one, with its own prefix (dat_) and its own binding module (_lib_attn.py).
 * Every device entry launches on `stream`, never waits for the device, uses no floating-point atomics and gives bitwise
 * the same result from run to run.
 *
 * Layout.  qkv is f32 [B, N, 3 C] contiguous as the qkv Linear writes it, C = heads * D: q / k / v of head h are the D-wide
 * slices of a token's row at columns 0 C + h D, 1 C + h D, 2 C + h D.  out is f32 [B, N, C] with head h in columns h D ..;
 * lse is f32 [B, heads, N], the log-sum-exp of the scaled scores of a query's row.
 *   out = softmax(scale * q k^T) v     per image and head.
 * Both products run on v_mfma_f32_32x32x16_f16 with split-f16 operands (hi.hi + hi.lo + lo.hi, f32 accumulation); the
 * operand scales of q, k, v and dout are powers of two from their absmax per (image, head), the probabilities take 2^14
 * and the score gradients a running power of two per wave.  The softmax is the online form (running max and sum, fp32). */
#ifndef DAT_ATTN_H
#define DAT_ATTN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DAT_OK 0
#define DAT_EINVAL 1
#define DAT_MAX_HEAD_DIM 256
#define DAT_QUERY_BLOCK 128 /* tokens one workgroup owns (four waves of 32) */

int dat_version(void);
const char *dat_last_error(void);

/* Host only (no device is touched): 1 when the kernels take the shape, else 0.
 * Taken: B >= 1, N >= 1, heads >= 1, D % 16 == 0, 16 <= D <= DAT_MAX_HEAD_DIM, B * N * 3 * heads * D < 2^31 and
 * B * heads <= 65535. */
int dat_supported(int B, int N, int heads, int D);

/* Host only.  Bytes of workspace, with r(x) = x rounded up to 256:
 *
 *   backward = 0 (dat_attn_fwd):   r(16 * B * heads)                              absmax of q, k, v (and dout) per (image, head)
 *   backward = 1 (dat_attn_bwd):   r(16 * B * heads) + r(4 * B * heads * N)       ... and delta = rowsum(dout * out)
 *
 * Returns -1 for a shape dat_supported refuses. */
int64_t dat_workspace_bytes(int B, int N, int heads, int D, int backward);

/* Forward.
 *   qkv        f32 [B, N, 3 C], 16-byte aligned
 *   scale      the factor of the scores (the module's qk_scale or D^-0.5)
 *   workspace  workspace_bytes >= dat_workspace_bytes(B, N, heads, D, 0) bytes, 256-byte aligned; contents on entry do not matter
 *   out        f32 [B, N, C] out, 16-byte aligned        lse   f32 [B, heads, N] out */
int dat_attn_fwd(const float *qkv, int B, int N, int heads, int D, float scale, void *workspace, int64_t workspace_bytes,
                 float *out, float *lse, void *stream);

/* Backward: dqkv f32 [B, N, 3 C] is written completely (the caller may hand uninitialised memory), from
 *   qkv, out, lse   as of dat_attn_fwd         dout   f32 [B, N, C], 16-byte aligned
 *   workspace       workspace_bytes >= dat_workspace_bytes(B, N, heads, D, 1) bytes, 256-byte aligned
 * by four launches: absmax, delta, a key-block-owned kernel (dk, dv) and a query-block-owned kernel (dq); the scores are
 * recomputed in both of the last two. */
int dat_attn_bwd(const float *qkv, const float *out, const float *lse, const float *dout, int B, int N, int heads, int D,
                 float scale, void *workspace, int64_t workspace_bytes, float *dqkv, void *stream);

#ifdef __cplusplus
}
#endif
#endif
