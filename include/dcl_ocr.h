/* C ABI of libdcl_ocr.so: the object-contextual (OCR) context core of OCRNet (reference models/OCR.py: SpatialGatherModule
 * and the middle of ObjectAttentionBlock2D.forward) on gfx950 kernels, forward and backward.
 *
 * A fourth, small library next to the main one, with its own prefix (dco_) and its own binding module (_lib_ocr.py).
 * Every device entry launches on `stream`, never waits for the device, uses no floating-point atomics and gives bitwise
 * the same result from run to run: sums over N are per-split partial sums (a split is a fixed range of pixel tiles, walked in
 * order) that a second kernel adds in the order of the splits.
 *
 * Layouts (all f32, contiguous, 16-byte aligned; nothing is transposed on the way in or out):
 *   x      [B, C, N]    the NCHW feature map                 logits [B, K, N]
 *   ctx    [B, K, C]    (the module returns its [B, C, K, 1] view)
 *   stats  [B, K, 2]    per (image, class): max_n(scale * logits) and sum_n exp(scale * logits - max)
 *   q, out [B, Ck, N]   key, val [B, Ck, K]  (f_object(proxy) / f_down(proxy) as their convolutions write them, viewed)
 *
 * Gather:     p = softmax_N(scale * logits) per (image, class);  ctx[b,k,c] = sum_n p[b,k,n] x[b,c,n]
 * Attention:  a[b,n,.] = softmax_K(s * sum_c q[b,c,n] key[b,c,.]);  out[b,c,n] = sum_k a[b,n,k] val[b,c,k]
 *
 * Arithmetic: plain fp32 FMA with fp32 accumulation, the softmax with its maximum subtracted (expf).  A block of 256 threads
 * owns a tile of DCO_TILE_N pixels with all K classes (padded to a multiple of 16) in LDS; channels go in chunks of DCO_CHUNK_C. */
#ifndef DCO_OCR_H
#define DCO_OCR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCO_OK 0
#define DCO_EINVAL 1
#define DCO_TILE_N 64    /* pixels one workgroup holds at a time */
#define DCO_CHUNK_C 64   /* channels of one accumulation chunk */
#define DCO_MAX_SPLIT 16 /* most partial sums over N per (image, channel chunk) */
#define DCO_MAX_C 1024
#define DCO_MAX_K 256
#define DCO_MAX_B 65535 /* the batch is a launch's grid y dimension */

#define DCO_OP_GATHER_FWD 0
#define DCO_OP_GATHER_BWD 1
#define DCO_OP_ATTN_FWD 2
#define DCO_OP_ATTN_BWD 3

int dco_version(void);
const char *dco_last_error(void);

/* Host only (no device is touched): 1 when the kernels take the shape, else 0.  C is the gather's channel count or the
 * attention's key width Ck.  Taken: 1 <= B <= DCO_MAX_B (grid y; grid x is at most ceil(N / DCO_TILE_N) < 2^25, grid z at most
 * DCO_MAX_C / DCO_CHUNK_C), C % 16 == 0, 16 <= C <= DCO_MAX_C, 1 <= K <= DCO_MAX_K, N >= 1, B * C * N < 2^31 and
 * B * K * N < 2^31. */
int dco_supported(int B, int C, int K, int N);

/* Host only.  The number of partial sums over N: with tiles = ceil(N / DCO_TILE_N) and chunks = ceil(C / DCO_CHUNK_C),
 *   want = min(tiles, DCO_MAX_SPLIT, max(1, ceil(512 / (B * chunks)))),  per = ceil(tiles / want),  splits = ceil(tiles / per):
 * every split walks `per` tiles (the last one the rest), none is empty.  0 for a shape dco_supported refuses. */
int dco_splits(int B, int C, int N);

/* Host only.  Bytes of workspace of one entry, with r(x) = x rounded up to 256:
 *   DCO_OP_GATHER_FWD   r(4 * B * splits * K * C)       the partial ctx of every split
 *   DCO_OP_GATHER_BWD   0                               (a null workspace is accepted)
 *   DCO_OP_ATTN_FWD     0
 *   DCO_OP_ATTN_BWD     r(8 * B * splits * C * K)       the partial dval and dkey of every split
 * Returns -1 for an unknown op or a shape dco_supported refuses. */
int64_t dco_workspace_bytes(int op, int B, int C, int K, int N);

/* Every device entry: workspace of at least dco_workspace_bytes(op, ...) bytes, 256-byte aligned, contents on entry do not
 * matter; a smaller one is refused before anything is launched.  Outputs are written completely. */

/* ctx and stats from x and logits (three launches: stats, partial sums, sum of the splits). */
int dco_gather_fwd(const float *x, const float *logits, int B, int C, int K, int N, float scale, void *workspace,
                   int64_t workspace_bytes, float *ctx, float *stats, void *stream);

/* dx[b,c,n] = sum_k p dctx[b,k,c] and dlogits[b,k,n] = scale p (g - dot[b,k]) with g = sum_c dctx[b,k,c] x[b,c,n] and
 * dot[b,k] = sum_c dctx[b,k,c] ctx[b,k,c], in one pass over x and one launch.  g - dot is evaluated as
 * sum_c dctx[b,k,c] (x[b,c,n] - ctx[b,k,c]): where a pixel owns its class the two sums cancel, and their difference taken
 * after rounding each would lose the digits the softmax's own backward keeps. */
int dco_gather_bwd(const float *x, const float *logits, const float *ctx, const float *stats, const float *dctx, int B, int C,
                   int K, int N, float scale, void *workspace, int64_t workspace_bytes, float *dx, float *dlogits, void *stream);

/* out from q, key, val; s is the factor of the scores (Ck^-0.5).  One launch. */
int dco_attn_fwd(const float *q, const float *key, const float *val, int B, int Ck, int K, int N, float s, void *workspace,
                 int64_t workspace_bytes, float *out, void *stream);

/* dq, dkey, dval from q, key, val and dout; the probabilities are recomputed (four launches: dq per pixel tile, the partial
 * dval / dkey per split and channel chunk, and their two sums). */
int dco_attn_bwd(const float *q, const float *key, const float *val, const float *dout, int B, int Ck, int K, int N, float s,
                 void *workspace, int64_t workspace_bytes, float *dq, float *dkey, float *dval, void *stream);

#ifdef __cplusplus
}
#endif
#endif
