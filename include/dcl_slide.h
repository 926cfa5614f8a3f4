/* C ABI of libdcl_slide.so: sliding-window test-time augmentation with equal-size windows (reference models/TTA_wrapper_PC.py,
 * models/TTAWrapperSlide.py) on gfx950 kernels, inference only.
 *
 * An eleventh, small library next to the main one, with its own prefix (dsw_) and its own binding module (_lib_slide.py).  Both
 * protocols cut many windows of ONE size out of one resized image (PASCAL-Context pads partial windows to the crop, the ADE20K
 * protocol shifts the last window back), run each plain and mirrored, and average exp(logits) over the windows that cover a pixel.
 * Here the windows of a scale are one batch: dsw_crops writes the batch (and its mirrors) from the original image in one launch,
 * dsw_gather writes the averaged canvas from the batch's logits in one launch.  The canvas is then added to the sum over the scales
 * by the merge entry of include/dcl_tta.h with an identity inner level.
 *
 * Every device entry launches on `stream`, never waits for the device, allocates nothing on it, uses no floating-point atomics and
 * gives bitwise the same result from run to run: every output element is written by exactly one thread, in a fixed order of
 * summation.  Window tables are host `int` arrays, handed to the kernels by value.
 *
 * Layouts: all f32, contiguous.  Nothing has to be 16-byte aligned: where base and row length allow, an output is written 16 bytes
 * per lane, else element by element.  Every tensor holds fewer than 2^31 elements; offsets are 64-bit.
 *
 * Resizing is bilinear with ATen's index arithmetic (csrc/dcl_bilinear.h, as include/dcl_tta.h states it):
 *   value = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11)
 * Arithmetic: plain fp32 FMA, expf and one division by the window count. */
#ifndef DSW_SLIDE_H
#define DSW_SLIDE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSW_OK 0
#define DSW_EINVAL 1
#define DSW_MAX_C 1024
#define DSW_MAX_CIN 8
#define DSW_MAX_WIN 64 /* windows per axis */
#define DSW_RUN 4      /* consecutive output pixels along W that one thread owns */

int dsw_version(void);
const char *dsw_last_error(void);

/* Host only (no device is touched): 1 when both kernels take one scale's shapes, else 0.  x is [Cin, H, W]; the R x Q windows are
 * wh x ww each; their logits are [R * Q, C, h, w] (h <= wh, w <= ww); the canvas is [C, Hc, Wc].  Taken: 1 <= Cin <= DSW_MAX_CIN,
 * 1 <= C <= DSW_MAX_C, 1 <= R, Q <= DSW_MAX_WIN, every size >= 1, h <= wh, w <= ww, and Cin * H * W, 2 * R * Q * Cin * wh * ww,
 * R * Q * C * h * w and C * Hc * Wc each below 2^31. */
int dsw_supported(int Cin, int H, int W, int C, int h, int w, int wh, int ww, int R, int Q, int Hc, int Wc);

/* out [R * Q * (1 + mirror), Cin, wh, ww]: window n = r * Q + q holds the half-pixel (align_corners = false) bilinear resize of
 * x [Cin, H, W] to nh x nw, read at (row_lo[r] + y, col_lo[q] + x); positions at or beyond nh / nw hold pad[c].  With `mirror`
 * block R * Q + n is block n mirrored along W, padding included (the reference flips the padded crop).  The resized image, the
 * padded image, the slices and the flips are never written.  Needs row_lo / col_lo >= 0.  One launch. */
int dsw_crops(const float *x, int Cin, int H, int W, int nh, int nw, const int *row_lo, int R, const int *col_lo, int Q, int wh, int ww,
              const float *pad, int mirror, float *out, void *stream);

/* canvas [C, Hc, Wc] = (sum over the windows (r, q) that cover the pixel, r ascending then q ascending, of exp(m)) / their number,
 *   m = up(z_n)(y - lo_r, x - lo_q)                                                   when zf is NULL,
 *   m = 0.5 * (up(z_n)(y - lo_r, x - lo_q) + up(zf_n)(y - lo_r, ww - 1 - (x - lo_q)))  otherwise,
 * n = r * Q + q, z and zf [R * Q, C, h, w], up = the bilinear resize h x w -> wh x ww.  Window r covers [lo_r, min(lo_r + wh, Hc)):
 * the canvas is the un-padded image, a window that reaches beyond it is clipped.  Needs 0 <= lo < Hc (Wc) for every window and at
 * least one window over every pixel (DSW_EINVAL otherwise, before any launch).  The canvas is stored, not added to.  One launch. */
int dsw_gather(const float *z, const float *zf, int C, int h, int w, int wh, int ww, int align_inner, const int *row_lo, int R,
               const int *col_lo, int Q, float *canvas, int Hc, int Wc, void *stream);

/* ---- the plan: host arithmetic (csrc/dcl_slide_plan.h), exported for the Python side and its tests ---- */

/* PASCAL-Context windows along one axis of length n >= crop (the caller pads a shorter axis to the crop first): no shift-back,
 * count = (int)ceil((n - crop) / stride) + 1 (returned; < 1: no window, nothing is written), window r covers [lo[r], hi[r]) with
 * lo = r * stride and hi = min(lo + crop, n).  lo / hi hold `cap` entries (a count above cap is returned, nothing written). */
int dsw_plan_pc_windows(int n, int crop, int stride, int cap, int *lo, int *hi);

/* cnt[i] (n entries) = number of the R windows [lo[r], min(lo[r] + wh, n)) over position i; returns the smallest entry, or -1 for
 * bad arguments (n < 1, wh < 1, R < 1 or R > DSW_MAX_WIN, a lo outside [0, n)).  cnt may be NULL. */
int dsw_plan_cover(int n, int wh, const int *lo, int R, int32_t *cnt);

#ifdef __cplusplus
}
#endif
#endif
