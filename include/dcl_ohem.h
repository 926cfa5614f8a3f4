/* C ABI of libdcl_ohem.so: online hard example mining for the pixel-wise cross-entropy (the public HRNet OhemCrossEntropy) on gfx950
 * kernels: the per-pixel target probability, an exact k-th-smallest selection by radix select, and the masked reduction.
 *
 * A thirteenth, small library next to the main one, with its own prefix (doh_) and its own binding module (_lib_ohem.py).  It sits
 * BETWEEN two entries of the main library, which it neither links nor changes: dcl_upsample_ce_fwd gives the log-sum-exp map the
 * first entry reads, dcl_upsample_ce_bwd takes the hard-target map the last entry writes.  Every device entry launches on `stream`
 * and never waits for the device; nothing comes back to the host.  The only atomics are integer additions (histograms, the count of
 * valid pixels); float sums are two-stage in a fixed order: results are bitwise the same from run to run.
 *
 * The arithmetic (losses/OhemCrossEntropy.py states it in torch):
 *   valid_i = 0 <= t_i < C and t_i != ignore
 *   p_i = exp(z_i[t_i] - lse_i),  l_i = w[t_i] (lse_i - z_i[t_i])                       (valid pixels)
 *   n = #valid,  k = min(min_kept, n - 1),  v = sort(p)[k],  thr = max(v, thresh)
 *   kept_i = valid_i and p_i < thr,  m = #kept,  loss = sum_kept l_i / max(m, 1)
 * z_i is the bilinear resize of the low-resolution logits (ATen's index arithmetic, csrc/dcl_bilinear.h; with h == H and w == W it
 * reads the logits as they are), evaluated for the target class only:
 *   z = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11)
 *
 * Layouts: logits f32 contiguous [N, C, h, w]; labels int64 [N, H, W]; maps f32 / int64 / uint8 [N, H, W]; the workspace is
 * doh_workspace_bytes(N, H) bytes, 16-byte aligned, and is initialised by doh_target_prob.  p >= 0, so the order of its bits as
 * uint32 is the order of the floats; a NaN is given the bits 0x7fc00000 (it orders last and is never kept); an invalid pixel holds
 * DOH_INVALID_BITS, which no pass selects (the sign bit is set) and which compares false with every threshold. */
#ifndef DOH_OHEM_H
#define DOH_OHEM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DOH_OK 0
#define DOH_EINVAL 1
#define DOH_MAX_C 255
#define DOH_INVALID_BITS 0xffffffffu

/* the eight 32-bit words of the result (doh_reduce writes all of them) */
#define DOH_RES_LOSS 0  /* f32: sum_kept l / max(m, 1) */
#define DOH_RES_DENOM 1 /* f32: max(m, 1): the backward's scale is grad_out / this */
#define DOH_RES_V 2     /* f32: the k-th smallest p (0 when n == 0) */
#define DOH_RES_THR 3   /* f32: max(v, thresh) */
#define DOH_RES_N 4     /* i32: valid pixels */
#define DOH_RES_M 5     /* i32: kept pixels */
#define DOH_RES_K 6     /* i32: min(min_kept, n - 1) (0 when n == 0) */
#define DOH_RES_EMPTY 7 /* i32: 1 when n == 0 */
#define DOH_RES_WORDS 8

int doh_version(void);
const char *doh_last_error(void);

/* Host only: 1 when the entries below -- and the two entries of the main library around them -- take the shape, else 0.  Taken:
 * N, h, w >= 1, H >= h, W >= w, 1 <= C <= DOH_MAX_C, N * H * W and N * C * h * w below 2^31, 2 w <= 6144 (the forward's LDS stage),
 * 3 w + W <= 36864 and 2 ceil(H / h) + 8 <= 80 (the backward's LDS tile and row table). */
int doh_supported(int N, int C, int h, int w, int H, int W);

/* Bytes of workspace for N * H output rows (the histograms of the three digit passes, the selection state, the row partials);
 * -1 for N * H outside [1, 2^31). */
int64_t doh_workspace_bytes(int N, int H);

/* p, l [N, H, W] from the logits, the labels and lse (as dcl_upsample_ce_fwd wrote it); clears the workspace, counts n and fills
 * the histogram of the first digit.  weight: f32 [C] or null. */
int doh_target_prob(const float *z, int N, int C, int h, int w, int H, int W, int align_corners, const int64_t *target,
                    const float *weight, int ignore_index, const float *lse, float *p, float *l, void *workspace, void *stream);

/* The k-th smallest p among the valid pixels, k = min(max(min_kept, 1), n - 1) formed on the device from the counted n, and
 * thr = max(v, thresh): two more digit passes over p [total], a one-workgroup pick after each histogram.  Leaves v, thr, n, k and
 * the n == 0 flag in the workspace for doh_reduce. */
int doh_select(const float *p, int64_t total, int min_kept, float thresh, void *workspace, void *stream);

/* kept = p < thr; hard [N, H, W] = the label where kept, ignore_index elsewhere (the target map of dcl_upsample_ce_bwd); kept8
 * (optional, may be null) = 1 / 0; res = the DOH_RES_WORDS words above.  One workgroup per row writes {sum l, count}, one workgroup
 * sums the rows in double, both in a fixed order. */
int doh_reduce(const float *p, const float *l, const int64_t *target, int N, int H, int W, int ignore_index, void *workspace,
               int64_t *hard, uint8_t *kept8, void *res, void *stream);

/* ---- the plan: host arithmetic (csrc/dcl_ohem_plan.h), exported for the Python side and its tests ---- */

/* Word offsets (in 4-byte words from the workspace's start) of the three histograms, the state and the row partials, and the
 * number of bins of each pass: off[5], bins[3]. */
int doh_plan_layout(int *off, int *bins);

#ifdef __cplusplus
}
#endif
#endif
