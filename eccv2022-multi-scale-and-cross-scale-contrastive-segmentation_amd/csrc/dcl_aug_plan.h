// dcl_aug_plan.h -- what dcl_aug.hip, dcl_aug_capi.cpp and the host tests share: every index rule of the input augmentation
// (include/dcl_aug.h), once.  The triangle filter's taps and weights, the exact nearest index, the composition of crop corner, pad
// offset and flip, the choice among the candidates' verdicts, and the plan test.  Host-compilable: plain functions, no HIP (DAU_HD
// is empty unless a HIP compiler reads this, where it lets the kernels call the same code).
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/dcl_aug.h"

#ifdef __HIPCC__
#define DAU_HD __host__ __device__
#else
#define DAU_HD
#endif

void dau_set_error(const char *fmt, ...);

// One axis S -> D of PIL's BILINEAR (Resample.c precompute_coeffs, bilinear_filter), in double as there.
struct DauAxis {
    double scale;   // S / D
    double sup;     // the filter's half width in source pixels: max(scale, 1)
    int S;
};

DAU_HD static inline DauAxis dau_axis(int S, int D)
{
    DauAxis a;
    a.scale = (double)S / (double)D;
    a.sup = a.scale > 1.0 ? a.scale : 1.0;
    a.S = S;
    return a;
}

// taps [k0, k1) of output index o and the sum of their raw weights
DAU_HD static inline double dau_tap_range(const DauAxis a, int o, int *k0, int *k1, double *centre)
{
    const double c = ((double)o + 0.5) * a.scale;
    int lo = (int)(c - a.sup + 0.5), hi = (int)(c + a.sup + 0.5);      // trunc, as C's cast
    if (lo < 0)
        lo = 0;
    if (hi > a.S)
        hi = a.S;
    double sum = 0.0;
    for (int k = lo; k < hi; ++k) {
        const double t = 1.0 - fabs((double)k + 0.5 - c) / a.sup;
        sum += t > 0.0 ? t : 0.0;
    }
    *k0 = lo;
    *k1 = hi;
    *centre = c;
    return sum;
}

// normalised weight of tap k (rounded to fp32 last)
DAU_HD static inline float dau_tap_weight(const DauAxis a, double centre, double sum, int k)
{
    const double t = 1.0 - fabs((double)k + 0.5 - centre) / a.sup;
    return (float)((t > 0.0 ? t : 0.0) / sum);
}

// PIL's NEAREST without its accumulated double: floor((o + 0.5) S / D) in integers
DAU_HD static inline int dau_nearest(int S, int D, int o)
{
    if ((uint64_t)(2u * (uint64_t)D) * (uint64_t)S <= 0xffffffffull)        // (2 o + 1) S < 2 D S fits 32 bits: the cheap division
        return (int)(((uint32_t)(2 * o + 1) * (uint32_t)S) / (uint32_t)(2 * D));
    return (int)(((int64_t)(2 * (int64_t)o + 1) * S) / (2 * (int64_t)D));
}

// column k of the mirrored (or not) image -> column of the stored one
DAU_HD static inline int dau_src_col(int k, int W, int flip) { return flip ? W - 1 - k : k; }

// pixel (y, x) of candidate p's crop -> its position (ry, rx) in the resized image; false: it lies in the padding
DAU_HD static inline bool dau_crop_to_resized(const dau_plan &pl, int p, int y, int x, int *ry, int *rx)
{
    *ry = pl.ci[p] + y - pl.pt;
    *rx = pl.cj[p] + x - pl.pl;
    return *ry >= 0 && *ry < pl.rh && *rx >= 0 && *rx < pl.rw;
}

// the label at (ry, rx) of the resized, mirrored, remapped label map
DAU_HD static inline int dau_label_at(const uint8_t *lbl, const uint8_t *lut, const dau_plan &pl, int ry, int rx)
{
    const int sy = dau_nearest(pl.H, pl.rh, ry);
    const int sx = dau_src_col(dau_nearest(pl.W, pl.rw, rx), pl.W, pl.flip);
    return lut[lbl[(int64_t)sy * pl.W + sx]];
}

// the verdict of one candidate from its histogram's summary (classes = bins other than `ignore` that are not empty): the
// reference's float64 comparison
DAU_HD static inline int dau_verdict(int classes, int max_count, int sum_count, double max_ratio)
{
    return classes > 1 && (double)max_count / (double)sum_count < max_ratio ? 1 : 0;
}

// the chosen candidate from the P verdicts (ws[3 p]): the first acceptable one, else the last
DAU_HD static inline int dau_chosen(const int32_t *ws, int P)
{
    for (int p = 0; p + 1 < P; ++p)
        if (ws[3 * p])
            return p;
    return P - 1;
}

static inline bool dau_scale_ok(int S, int D) { return S >= 1 && D >= 1 && (int64_t)S <= 8 * (int64_t)D && (int64_t)D <= 8 * (int64_t)S; }

static inline bool dau_plan_ok(const dau_plan *p)
{
    if (!p)
        return false;
    const int64_t lim = 1ll << 31;
    if (!dau_scale_ok(p->H, p->rh) || !dau_scale_ok(p->W, p->rw))
        return false;
    if (p->h < 1 || p->w < 1 || p->Hc < 1 || p->Wc < 1 || p->pt < 0 || p->pl < 0)
        return false;
    if ((int64_t)p->pt + p->rh > p->Hc || (int64_t)p->pl + p->rw > p->Wc || p->h > p->Hc || p->w > p->Wc)
        return false;
    if (3 * (int64_t)p->H * p->W >= lim || 3 * (int64_t)p->h * p->w >= lim || (int64_t)p->Hc * p->Wc >= lim)
        return false;
    if (p->P < 1 || p->P > DAU_MAX_CAND || (p->P > 1 && !(p->max_ratio > 0.0)))
        return false;
    for (int i = 0; i < p->P; ++i)
        if (p->ci[i] < 0 || p->cj[i] < 0 || p->ci[i] > p->Hc - p->h || p->cj[i] > p->Wc - p->w)
            return false;
    if (p->ncolor < 0 || p->ncolor > 4 || p->ignore < 0 || p->ignore > 255)
        return false;
    int seen = 0;
    for (int i = 0; i < p->ncolor; ++i) {
        if (p->perm[i] < 0 || p->perm[i] > 3 || (seen >> p->perm[i] & 1))
            return false;
        seen |= 1 << p->perm[i];
    }
    return isfinite(p->b) && isfinite(p->c) && isfinite(p->s) && isfinite(p->delta);
}

// position of contrast in the chain; -1: none
DAU_HD static inline int dau_contrast_pos(const dau_plan &pl)
{
    for (int i = 0; i < pl.ncolor; ++i)
        if (pl.perm[i] == 1)
            return i;
    return -1;
}
