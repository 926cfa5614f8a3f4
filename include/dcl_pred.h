/* C ABI of libdcl_pred.so: prediction maps from logits (reference managers/BaseManager.py save_output, utils/utils.py to_comb_image)
 * on gfx950 kernels, inference only.
 *
 * An eighth, small library next to the main one, with its own prefix (dpr_) and its own binding module (_lib_pred.py).  Every device
 * entry launches on `stream`, never waits for the device, uses no atomics and gives bitwise the same result from run to run: every
 * output byte is written by exactly one thread of one launch.
 *
 * Layouts: logits f32 contiguous [N, C, h, w]; maps uint8 [N, H, W]; colour maps uint8 [N, H, W, 3]; tables uint8[256] and
 * uint8[256][3] in device memory.  Nothing has to be 16-byte aligned: where an output's base is 4-byte aligned and W is a multiple of
 * DPR_RUN, a thread stores its run as 4-byte words, else byte by byte.
 *
 * Resizing is the bilinear resize of include/dcl_tta.h (ATen's index arithmetic, UpSample.h, f32):
 *   align_corners: scale = (in-1)/(out-1) (0 if out == 1), src = scale * dst
 *   otherwise    : scale = in/out,                         src = max(scale * (dst + 0.5) - 0.5, 0)
 *   i0 = min((int)src, in-1), i1 = i0 + (i0 < in-1), l1 = src - i0, l0 = 1 - l1
 *   value = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11)
 * The arg-max rule is torch.argmax's: the first maximal index wins, a NaN counts as the maximum. */
#ifndef DPR_PRED_H
#define DPR_PRED_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPR_OK 0
#define DPR_EINVAL 1
#define DPR_MAX_C 256
#define DPR_MAX_N 65535
#define DPR_RUN 4 /* consecutive output pixels along W that one thread owns */

int dpr_version(void);
const char *dpr_last_error(void);

/* Host only (no device is touched): 1 when dpr_predict takes the shape, else 0.  Taken: 1 <= C <= DPR_MAX_C, 1 <= N <= DPR_MAX_N,
 * every size >= 1, and N * C * h * w, N * H * W and (with_rgb != 0) N * H * W * 3 each below 2^31. */
int dpr_supported(int N, int C, int h, int w, int H, int W, int with_rgb);

/* ids[n, Y, X] = argmax_c resize(z[n] -> H x W)[c, Y, X]; mapped = lut[ids] when lut and mapped are given; rgb = palette[ids] when
 * palette and rgb are given (a table without its output, or the reverse, is an error).  With h == H and w == W the map is read as it
 * is: ids equals torch.argmax(z, 1).  One launch for all N; the full-size logits are never written. */
int dpr_predict(const float *z, int N, int C, int h, int w, int H, int W, int align_corners, const uint8_t *lut,
                const uint8_t *palette, uint8_t *ids, uint8_t *mapped, uint8_t *rgb, void *stream);

/* Host only: 1 when dpr_panel takes the shape (H, W >= 1, H * 3 W * 3 below 2^31; label_bytes 1, 4 or 8). */
int dpr_panel_supported(int H, int W, int label_bytes);

/* panel uint8 [H, 3 W, 3], one launch: columns [0, W) hold round(clamp(img * std + mean, 0, 1) * 255) of the normalised image
 * f32 [3, H, W] (product and sum rounded separately, round-half-even), [W, 2 W) palette[label] and [2 W, 3 W) palette[ids].  A label
 * equal to label_ignore or outside [0, 255], and a prediction equal to ids_ignore, are black (-1: no such id).  label is int64, int32
 * or uint8 (label_bytes = 8, 4, 1), ids uint8 [H, W]. */
int dpr_panel(const float *img, const void *label, int label_bytes, const uint8_t *ids, const uint8_t *palette, int H, int W,
              float mean0, float mean1, float mean2, float std0, float std1, float std2, int label_ignore, int ids_ignore,
              uint8_t *panel, void *stream);

/* ---- the plan: host arithmetic (csrc/dcl_pred_plan.h), exported for the Python side and its tests ---- */

/* Source index and weights of output index dst along an axis resized from in_size to out_size. */
int dpr_plan_src_index(int in_size, int out_size, int align, int dst, int *i0, int *i1, float *l0, float *l1);

/* Runs per row of width W (returned; < 1: bad arguments); *vec = 1 when a buffer at byte address `base` with rows of W pixels of
 * `pixel_bytes` bytes (1 or 3) is stored as 4-byte words. */
int dpr_plan_runs(int W, uint64_t base, int pixel_bytes, int *vec);

#ifdef __cplusplus
}
#endif
#endif
