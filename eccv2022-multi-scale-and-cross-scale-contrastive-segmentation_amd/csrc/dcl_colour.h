// dcl_colour.h -- the four colour operations of the input augmentation (include/dcl_aug.h, "colour"), once: dcl_aug.hip applies them
// to the pixel it has just resized, dcl_blur.hip to a pixel of the float32 planes.  fp32 on values in [0, 255], clamped after every
// operation.  Device code only; `Plan` is any struct with the fields perm[4], b, c, s, delta (dau_plan, dbl_colour_plan).
#pragma once
#include <hip/hip_runtime.h>

struct Rgb {
    float r, g, b;
};

__device__ __forceinline__ float clamp255(float v) { return fminf(fmaxf(v, 0.f), 255.f); }

__device__ __forceinline__ float luma(const Rgb v) { return (299.f * v.r + 587.f * v.g + 114.f * v.b) / 1000.f; }

// RGB -> HSV -> RGB with the hue turned by delta; v stays in [0, 255], s and h are ratios
__device__ __forceinline__ Rgb hue_shift(const Rgb v, float delta)
{
    const float maxc = fmaxf(v.r, fmaxf(v.g, v.b)), minc = fminf(v.r, fminf(v.g, v.b));
    const bool eq = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eq ? 1.f : maxc);
    const float d = eq ? 1.f : cr;
    const float rc = (maxc - v.r) / d, gc = (maxc - v.g) / d, bc = (maxc - v.b) / d;
    float h;
    if (maxc == v.r)
        h = bc - gc;
    else if (maxc == v.g)
        h = 2.f + rc - bc;
    else
        h = 4.f + gc - rc;
    h = h / 6.f + 1.f;
    h = h - floorf(h);
    h = h + delta;
    h = h - floorf(h);
    const float h6 = h * 6.f;
    const float fl = floorf(h6);
    const float f = h6 - fl;
    const int i = ((int)fl) % 6;
    const float p = clamp255(maxc * (1.f - s));
    const float q = clamp255(maxc * (1.f - f * s));
    const float t = clamp255(maxc * (1.f - (1.f - f) * s));
    switch (i) {
    case 0: return {maxc, t, p};
    case 1: return {q, maxc, p};
    case 2: return {p, maxc, t};
    case 3: return {p, q, maxc};
    case 4: return {t, p, maxc};
    default: return {maxc, p, q};
    }
}

// operations [first, last) of the plan's chain
template <class Plan>
__device__ __forceinline__ Rgb colour_ops(Rgb v, const Plan &pl, int first, int last, float m)
{
    for (int i = first; i < last; ++i) {
        switch (pl.perm[i]) {
        case 0:
            v = {clamp255(pl.b * v.r), clamp255(pl.b * v.g), clamp255(pl.b * v.b)};
            break;
        case 1:
            v = {clamp255(m + pl.c * (v.r - m)), clamp255(m + pl.c * (v.g - m)), clamp255(m + pl.c * (v.b - m))};
            break;
        case 2: {
            const float L = luma(v);
            v = {clamp255(L + pl.s * (v.r - L)), clamp255(L + pl.s * (v.g - L)), clamp255(L + pl.s * (v.b - L))};
            break;
        }
        default:
            v = hue_shift(v, pl.delta);
            break;
        }
    }
    return v;
}
