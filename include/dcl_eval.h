/* C ABI of libdcl_eval.so: evaluation at the original label size (reference managers/HRNet_Manager.py post_process_output, the same
 * in its OCRNet and DeepLabv3 managers) on one gfx950 kernel, inference only.
 *
 * A ninth, small library next to the main one, with its own prefix (dve_) and its own binding module (_lib_eval.py).  The reference
 * cuts the fit_stride padding off the full-size logits, resizes them to the image's original size and scores the arg-max against
 * the label map that was never resized; done as a composition that forms [C, Hp, Wp] and [C, H0, W0] maps in memory.  Here one
 * launch reads the low-resolution (or the dense) logits and writes one byte per original pixel and the confusion matrix.
 *
 * Two resizes, both the bilinear resize of include/dcl_pred.h (ATen's index arithmetic, UpSample.h, f32):
 *   align_corners: scale = (in-1)/(out-1) (0 if out == 1), src = scale * dst
 *   otherwise    : scale = in/out,                         src = max(scale * (dst + 0.5) - 0.5, 0)
 *   i0 = min((int)src, in-1), i1 = i0 + (i0 < in-1), l1 = src - i0, l0 = 1 - l1
 *   value = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11)
 * stage 1 resizes z [C, h, w] to Hp x Wp; stage 2 resizes rows [0, rh) x columns [0, rw) of that map -- a map of size rh x rw: its
 * taps clamp at rh - 1 and rw - 1 -- to H0 x W0.  A stage-1 value is rounded to f32 before stage 2 uses it, so the result is the one
 * of resizing twice.  A stage whose input and output sizes are equal is the identity, bitwise.  The arg-max rule is torch.argmax's:
 * the first maximal index wins, a NaN counts as the maximum.
 *
 * The device entry launches on `stream`, never waits for the device and uses integer atomics only (the confusion matrix and the
 * out-of-range counter): results are bitwise the same from run to run, and every byte of ids is written by exactly one thread. */
#ifndef DVE_EVAL_H
#define DVE_EVAL_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVE_OK 0
#define DVE_EINVAL 1
#define DVE_MAX_C 256
#define DVE_RUN 4          /* consecutive output pixels along W0 that one thread owns */
#define DVE_LDS_CELLS 4096 /* cells of a workgroup's LDS histogram (16 KiB): above that, global atomics */

int dve_version(void);
const char *dve_last_error(void);

/* Host only (no device is touched): 1 when dve_evaluate takes the shape, else 0.  Taken: 1 <= C <= DVE_MAX_C, C <= cols <= C + 1,
 * every size >= 1, and C * h * w, C * Hp * Wp, C * H0 * W0 and H0 * W0 each below 2^31. */
int dve_supported(int C, int h, int w, int Hp, int Wp, int rh, int rw, int H0, int W0, int cols);

/* One image.  ids[Y, X] = argmax_c resize(resize(z -> Hp x Wp)[:, :rh, :rw] -> H0 x W0)[c, Y, X].  With label:
 * t = label_lut ? label_lut[label[Y, X]] : label[Y, X]; cm[ids * cols + t] += 1 when 0 <= t < cols, else *oob += 1 (callers slice
 * [:, :C]: column C collects the ignore id).  Neither full-size map is written to memory.
 * EINVAL before any launch: label without cm and oob or the reverse; neither cm nor ids; label_lut with label_bytes != 1;
 * label_bytes not 1, 4 or 8; rh > Hp or rw > Wp; a shape dve_supported rejects. */
int dve_evaluate(const float *z, int C, int h, int w,          /* logits f32 [C, h, w], contiguous */
                 int Hp, int Wp, int align_mid,                /* stage 1: resize z -> Hp x Wp (the network input size) */
                 int rh, int rw,                               /* crop: keep rows [0, rh), columns [0, rw) of stage 1 */
                 int H0, int W0, int align_out,                /* stage 2: resize the crop -> H0 x W0 (the original size) */
                 const void *label, int label_bytes,           /* [H0, W0] uint8 / int32 / int64 (1, 4, 8), or NULL */
                 const uint8_t *label_lut,                     /* uint8[256] or NULL; only with label_bytes == 1: t = lut[label] */
                 int cols, int32_t *cm, int32_t *oob,          /* cm int32 [C, cols], ADDED to; oob int32[1], added to */
                 uint8_t *ids,                                 /* uint8 [H0, W0] or NULL */
                 void *stream);

/* ---- the plan: host arithmetic (csrc/dcl_eval_plan.h), exported for the Python side and its tests ---- */

/* One axis, one output index dst of [0, out): j[2], m[2] = the stage-2 index pair into the crop and its weights; i[4], l[4] = for
 * j[0] (entries 0, 1) and j[1] (entries 2, 3) the stage-1 index pair into the input and its weights.  An identity stage
 * (in_size == mid, crop == out) gives the pair (q, q) with weights (1, 0).  Non-zero on bad arguments (crop > mid, dst outside). */
int dve_plan_taps(int in_size, int mid, int crop, int out, int align_mid, int align_out, int dst, int *j, float *m, int *i, float *l);

/* 1 when a workgroup keeps the [C, cols] histogram in LDS (C * cols <= DVE_LDS_CELLS) and flushes it once, 0 when every pixel
 * goes to the matrix with a global atomic. */
int dve_plan_hist_in_lds(int C, int cols);

/* Runs per row of width W0 (returned; < 1: bad arguments); *vec = 1 when ids at byte address `base` is stored as 4-byte words. */
int dve_plan_runs(int W0, uint64_t base, int *vec);

/* Slices the classes are split into inside a workgroup (1, 2, 4 or 8) for `items` runs of C classes. */
int dve_plan_class_split(int64_t items, int C);

#ifdef __cplusplus
}
#endif
#endif
