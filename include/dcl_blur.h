/* C ABI of libdcl_blur.so: the steps of the training-time input augmentation that follow the crop (reference utils/transforms.py
 * BlurPIL, utils/np_transforms.py PadNP, torchvision's ColorJitter / Normalize of utils/config_parsers.py) on gfx950 kernels, on ONE
 * image's float32 planes [C, h, w] on the 0..255 scale and its int64 [h, w] label map.
 *
 * A twelfth, small library next to the main one, with its own prefix (dbl_) and its own binding module (_lib_blur.py).  Every device
 * entry launches on `stream`, never waits for the device, never reads anything back and allocates nothing.  No floating-point
 * atomics; bitwise the same result from run to run.
 *
 * The arithmetic ("Input augmentation"):
 *   blur     : PIL's ImageFilter.GaussianBlur(R) restated in floating point.  PIL does not convolve with a Gaussian: it runs three
 *              "extended box" passes along the rows (x), then three along the columns (y).  The box radius, in double on the host:
 *                s2 = R^2 / 3, L = sqrt(12 s2 + 1), l = floor((L - 1) / 2),
 *                a = (2 l + 1) (l (l + 1) - 3 s2) / (6 (s2 - (l + 1)^2)), fr = l + a
 *              one pass: out[x] = ww * sum_{|d| <= l} in[clamp(x + d)] + fw * (in[clamp(x - l - 1)] + in[clamp(x + l + 1)]) with
 *              ww = 1 / (2 fr + 1), fw = (1 - (2 l + 1) ww) / 2, both rounded to fp32; the index is clamped to the image in EVERY
 *              pass; the 2 l + 1 inner taps are summed directly from d = -l upwards (no sliding accumulator)
 *   pad_rows : numpy.pad(mode='reflect') along the rows: output row y is source row |y - top| for y < top and
 *              2 (h - 1) - (y - top) beyond the last one (PadNP(ver=(top, bottom), hor=(0, 0)))
 *   colour   : the four operations of include/dcl_aug.h in the order perm[0 .. ncolor), the same device code (csrc/dcl_colour.h);
 *              m of contrast = mean of L over the h x w image at that point of the chain, summed in double in a fixed order
 *   from_unit: x * 255 (dau_apply without `normalise` writes x / 255)
 *   normalise: x / 255, then (x - mean) / std with mean (0.485, 0.456, 0.406), std (0.229, 0.224, 0.225) when `normalise` != 0
 *
 * Limits (dbl_supported answers them on the host): integer 1 <= R <= DBL_MAX_RADIUS, 1 <= C <= DBL_MAX_CHANNELS, h, w >= 1 (also
 * smaller than the filter's support), C h w below 2^31; pad_rows: 0 <= top, bottom <= h - 1 and C (h + top + bottom) w below 2^31. */
#ifndef DBL_BLUR_H
#define DBL_BLUR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DBL_OK 0
#define DBL_EINVAL 1
#define DBL_MAX_RADIUS 8   /* l <= 7: 2 l + 3 <= 17 taps of one pass */
#define DBL_MAX_CHANNELS 4
#define DBL_ROW_TILE_H 4   /* the row kernel's workgroup: 4 rows of ... */
#define DBL_ROW_TILE_W 256 /* ... 256 columns (+ halo) in LDS */
#define DBL_COL_TILE_H 64  /* the column kernel's workgroup: 64 rows (+ halo) of ... */
#define DBL_COL_TILE_W 64  /* ... a strip 64 columns wide */
#define DBL_WS_INTS 576    /* int32 words of one image's workspace, zero before its first use */
#define DBL_WS_TICKET 32   /* word of the dbl_gray_mean ticket (left at zero by every call) */
#define DBL_WS_MEAN 33     /* word that holds m (fp32 bits) */
#define DBL_WS_PART 64     /* first of DBL_MAX_BLOCKS double partial sums (two words each) */
#define DBL_MAX_BLOCKS 256

typedef struct dbl_colour_plan {
    int32_t h, w;    /* the planes' size */
    int32_t ncolor;  /* colour operations applied, 0 .. 4 */
    int32_t perm[4]; /* their codes in order: 0 brightness, 1 contrast, 2 saturation, 3 hue */
    float b, c, s, delta;
} dbl_colour_plan;

int dbl_version(void);
const char *dbl_last_error(void);

/* Host only (no device is touched): 1 when dbl_blur takes the shape and the radius, else 0. */
int dbl_supported(int C, int h, int w, int radius);

/* Host only: the box of radius R: *l, *ww and *fw of the arithmetic above.  0, or DBL_EINVAL for a radius outside the limits. */
int dbl_box(int radius, int *l, float *ww, float *fw);

/* dst = GaussianBlur(radius) of src, both float32 [C, h, w]; scratch: float32 [C, h, w] (holds the rows' result between the two
 * launches).  The three buffers are distinct. */
int dbl_blur(const float *src, float *dst, float *scratch, int C, int h, int w, int radius, void *stream);

/* dst: float32 [C, h + top + bottom, w], lbl_dst: int64 [h + top + bottom, w]: the rows of src / lbl_src reflected about the first
 * and the last row.  One launch. */
int dbl_pad_rows(const float *src, float *dst, const int64_t *lbl_src, int64_t *lbl_dst, int C, int h, int w, int top, int bottom,
                 void *stream);

/* ws[DBL_WS_MEAN] = m of the plan's chain over planes (float32 [3, h, w]).  EINVAL when the chain holds no contrast. */
int dbl_gray_mean(const float *planes, const dbl_colour_plan *plan, int32_t *ws, void *stream);

/* The plan's chain on planes (float32 [3, h, w]) in place (m from ws when the chain holds contrast). */
int dbl_colour(float *planes, const dbl_colour_plan *plan, const int32_t *ws, void *stream);

/* dst[i] = src[i] * 255 for n values (dst may be src). */
int dbl_from_unit(const float *src, float *dst, int64_t n, void *stream);

/* out = planes / 255, normalised when `normalise` != 0; both float32 [3, n] (n pixels a plane). */
int dbl_normalise(const float *planes, float *out, int normalise, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif
