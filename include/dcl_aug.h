/* C ABI of libdcl_aug.so: the training-time input augmentation (reference utils/transforms.py, utils/np_transforms.py FlipNP and the
 * torchvision ColorJitter / Normalize of utils/config_parsers.py) on gfx950 kernels: from the decoded uint8 pixels of ONE image to its
 * float32 [3, h, w] / int64 [h, w] slice of the batch.
 *
 * A seventh, small library next to the main one, with its own prefix (dau_) and its own binding module (_lib_aug.py).  Every device
 * entry launches on `stream`, never waits for the device and never reads anything back: the choice among the candidate crops is
 * written to the workspace by dau_crop_select and derived from it by the kernels that follow on the same stream.  No floating-point
 * atomics; bitwise the same result from run to run.
 *
 * The arithmetic ("Input augmentation") in the reference's order: flip, resize, pad, crop, colour, normalise.
 *   flip     : the mirrored image is the source; every index rule is evaluated in mirrored coordinates, column k loads src[W-1-k]
 *   image    : PIL's BILINEAR, a separable triangle filter: scale = S/D, sup = max(scale, 1), centre = (o + 0.5) scale, taps k in
 *              [max(trunc(centre - sup + 0.5), 0), min(trunc(centre + sup + 0.5), S)), weights max(0, 1 - |k + 0.5 - centre| / sup)
 *              normalised to sum 1 (all of that in double, the weights then rounded to fp32); both axes in fp32 on the uint8 source
 *              with no rounding in between
 *   label    : PIL's NEAREST evaluated exactly: source index ((2 o + 1) S) / (2 D) in integers; then lut[.]
 *   pad      : the resized image sits at (pt, pl) of an Hc x Wc canvas; outside it the image is 0 and the label `ignore`
 *   crop     : candidate p has its corner at (ci[p], cj[p]) of the canvas; it is acceptable when at least two classes other than
 *              `ignore` occur in it and (double)max_count / (double)sum_count < max_ratio; the first acceptable one wins, else the
 *              last one
 *   colour   : on values in [0, 255], fp32, clamped after every operation, in the order perm[0 .. ncolor): with
 *              L = (299 R + 587 G + 114 B) / 1000
 *                0 brightness x <- clamp(b x)
 *                1 contrast   x <- clamp(m + c (x - m)), m = mean of L over the chosen crop at that point of the chain
 *                2 saturation x <- clamp(L + s (x - L))
 *                3 hue        RGB -> HSV, h <- frac(h + delta), HSV -> RGB
 *   normalise: x / 255, then (x - mean) / std with mean (0.485, 0.456, 0.406), std (0.229, 0.224, 0.225) when `normalise` != 0
 *
 * Limits (dau_supported answers them on the host): uint8 HWC RGB image and uint8 HW label, both contiguous; source, canvas and both
 * outputs each below 2^31 elements; per-axis scale S/D between 1/8 and 8 (at most DAU_MAX_TAPS taps per axis); the resized image
 * inside the canvas, the crop no larger than the canvas and every candidate inside it; 1 <= P <= DAU_MAX_CAND. */
#ifndef DAU_AUG_H
#define DAU_AUG_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DAU_OK 0
#define DAU_EINVAL 1
#define DAU_MAX_CAND 10  /* candidate crops of one plan (the reference's patience) */
#define DAU_MAX_TAPS 18  /* taps of one axis at scale 8: trunc(centre + 8.5) - trunc(centre - 7.5) <= 17, one spare */
#define DAU_WS_INTS 576  /* int32 words of one image's workspace, zero before its first use */
#define DAU_WS_TICKET 32 /* word of the dau_gray_mean ticket (left at zero by every call) */
#define DAU_WS_MEAN 33   /* word that holds m (fp32 bits) */
#define DAU_WS_PART 64   /* first of DAU_MAX_BLOCKS double partial sums (two words each) */
#define DAU_MAX_BLOCKS 256

typedef struct dau_plan {
    int32_t H, W;                  /* source image */
    int32_t rh, rw;                /* resized size */
    int32_t Hc, Wc;                /* padded canvas */
    int32_t pt, pl;                /* where the resized image starts in the canvas */
    int32_t h, w;                  /* crop = output size */
    int32_t flip;
    int32_t P;                     /* candidates */
    int32_t ci[DAU_MAX_CAND], cj[DAU_MAX_CAND];
    int32_t ncolor;                /* colour operations applied, 0 .. 4 */
    int32_t perm[4];               /* their codes in order: 0 brightness, 1 contrast, 2 saturation, 3 hue */
    float b, c, s, delta;
    int32_t normalise;
    int32_t ignore;                /* label of the padding, and the class the crop choice does not count; 0 .. 255 */
    double max_ratio;              /* crop_class_max_ratio; <= 0: none (then P == 1) */
} dau_plan;

int dau_version(void);
const char *dau_last_error(void);

/* Host only (no device is touched): 1 when the kernels take the plan, else 0. */
int dau_supported(const dau_plan *plan);

/* One workgroup per candidate: ws[3 p + {0, 1, 2}] = {acceptable, max_count, sum_count} of candidate p.  lbl: uint8 [H, W];
 * lut: uint8 [256]. */
int dau_crop_select(const uint8_t *lbl, const uint8_t *lut, const dau_plan *plan, int32_t *ws, void *stream);

/* ws[DAU_WS_MEAN] = m of the plan's chain over the chosen crop (needs the verdicts of dau_crop_select when P > 1).  EINVAL when
 * the chain holds no contrast.  img: uint8 [H, W, 3]. */
int dau_gray_mean(const uint8_t *img, const dau_plan *plan, int32_t *ws, void *stream);

/* out_img: float32 [3, h, w], out_lbl: int64 [h, w] of the chosen crop (verdicts, and m when the chain holds contrast, from ws). */
int dau_apply(const uint8_t *img, const uint8_t *lbl, const uint8_t *lut, const dau_plan *plan, const int32_t *ws, float *out_img,
              int64_t *out_lbl, void *stream);

/* ---- the index rules: host arithmetic (csrc/dcl_aug_plan.h), exported for the Python side and its tests ---- */

/* Taps of output index o along an axis resized from S to D: first tap *k0, their number (returned; < 0: bad arguments), and when
 * `cap` >= that number the normalised weights w[0 .. n). */
int dau_plan_taps(int S, int D, int o, int cap, int *k0, float *w);

/* Nearest source index of output index o (< 0: bad arguments). */
int dau_plan_nearest(int S, int D, int o);

#ifdef __cplusplus
}
#endif
#endif
