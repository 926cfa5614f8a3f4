/* C ABI of libdcl_tta.so: the merge of test-time-augmentation views (reference models/TTA_wrapper.py, models/TTA_wrapper_CTS.py)
 * on gfx950 kernels, inference only.
 *
 * A sixth, small library next to the main one, with its own prefix (dtt_) and its own binding module (_lib_tta.py).  Every device
 * entry launches on `stream`, never waits for the device, uses no floating-point atomics and gives bitwise the same result from run
 * to run: every element of an accumulator is read, added to and written by exactly one thread of one launch, and launches on one
 * stream are ordered, so `+=` from one view to the next is race-free.
 *
 * Layouts: all f32, contiguous, one image ([C, rows, columns]); the counts are int32.  Nothing has to be 16-byte aligned: where an
 * accumulator's base, row length and column offset allow, it is read and written 16 bytes per lane, else element by element.
 *
 * Resizing is bilinear with ATen's index arithmetic (UpSample.h: area_pixel_compute_scale / _source_index, f32), on both levels:
 *   align_corners: scale = (in-1)/(out-1) (0 if out == 1), src = scale * dst
 *   otherwise    : scale = in/out,                         src = max(scale * (dst + 0.5) - 0.5, 0)
 *   i0 = min((int)src, in-1), i1 = i0 + (i0 < in-1), l1 = src - i0, l0 = 1 - l1
 *   value = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11)
 * Arithmetic: plain fp32 FMA and expf. */
#ifndef DTT_TTA_H
#define DTT_TTA_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DTT_OK 0
#define DTT_EINVAL 1
#define DTT_MAX_C 1024
#define DTT_RUN 4 /* consecutive output pixels along W that one thread owns */

int dtt_version(void);
const char *dtt_last_error(void);

/* Host only (no device is touched): 1 when the kernels take the shape, else 0.  z is [C, h, w], the map it is resized to first is
 * Hm x Wm (never stored), the accumulator is [C, H, W].  Taken: 1 <= C <= DTT_MAX_C, every size >= 1, and C * h * w, C * Hm * Wm and
 * C * H * W each below 2^31. */
int dtt_supported(int C, int h, int w, int Hm, int Wm, int H, int W);

/* acc += weight * resize_outer(unflipW(resize_inner(z -> Hm x Wm)) -> H x W), one launch.  `flip` != 0: the Hm x Wm map is mirrored
 * along W before the outer resize (the view was computed on a mirrored image).  Each output pixel composes the 2 x 2 taps of the
 * outer level from the 2 x 2 taps of the inner level each; with h == Hm and w == Wm the inner level is the identity (z is the map:
 * a model that returns full-resolution logits). */
int dtt_merge(const float *z, int C, int h, int w, int Hm, int Wm, int align_inner, int flip, float *acc, int H, int W,
              int align_outer, float weight, void *stream);

/* canvas[:, h0:h0+wh, w0:w0+ww] += exp(m)[:, :wh, :ww] with m = up(z) when zf is NULL and m = 0.5 * (up(z) + unflipW(up(zf)))
 * otherwise; up is the resize of a [C, h, w] map to the crop's ch x cw, and zf holds the logits of the mirrored crop.  Needs
 * 1 <= wh <= ch, 1 <= ww <= cw and the window inside the [C, Hc, Wc] canvas.  One launch. */
int dtt_window_accum(const float *z, const float *zf, int C, int h, int w, int ch, int cw, int align_inner, float *canvas, int Hc,
                     int Wc, int h0, int w0, int wh, int ww, void *stream);

/* acc += resize(canvas / (rowcnt[y] * colcnt[x]) -> H x W): the number of windows over a canvas pixel is the product of the number
 * of window rows over y and of window columns over x (the cnt vectors of dtt_plan_windows).  One launch. */
int dtt_canvas_merge(const float *canvas, const int32_t *rowcnt, const int32_t *colcnt, int C, int Hc, int Wc, float *acc, int H,
                     int W, int align, void *stream);

/* ---- the plan: host arithmetic (csrc/dcl_tta_plan.h), exported for the Python side and its tests ---- */

/* The Cityscapes image-size rule: long = (int)(base_size * scale + 0.5) becomes the longer side (the width when H == W), the other
 * side is (int)(side * long / longer + 0.5). */
int dtt_plan_cts_size(int H, int W, int base_size, double scale, int *new_h, int *new_w);

/* Windows along one axis of length n: count = (int)ceil((n - crop) / stride) + 1 (returned; < 1: no window, nothing is written),
 * window r covers [lo[r], hi[r]) with hi = min(r * stride + crop, n) and lo = max(hi - crop, 0): the last one is shifted back, and a
 * window is shorter than the crop when the axis is.  lo / hi hold `cap` entries (a count above cap is returned, nothing written);
 * cnt (n entries, or NULL) receives the number of windows over each position. */
int dtt_plan_windows(int n, int crop, int stride, int cap, int *lo, int *hi, int32_t *cnt);

/* Source index and weights of output index dst along an axis resized from in_size to out_size. */
int dtt_plan_src_index(int in_size, int out_size, int align, int dst, int *i0, int *i1, float *l0, float *l1);

#ifdef __cplusplus
}
#endif
#endif
