// dcl_tta_plan.h -- what dcl_tta.hip, dcl_tta_capi.cpp and the host tests share: the shape test, the Cityscapes image-size rule,
// the sliding-window grid with its separable counts, and (dcl_bilinear.h) the bilinear source index.  Host-compilable: plain
// functions, no HIP.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/dcl_tta.h"
#include "dcl_bilinear.h"

void dtt_set_error(const char *fmt, ...);

static inline bool dtt_shape_ok(int C, int h, int w, int Hm, int Wm, int H, int W)
{
    if (C < 1 || C > DTT_MAX_C || h < 1 || w < 1 || Hm < 1 || Wm < 1 || H < 1 || W < 1)
        return false;
    const int64_t lim = 1ll << 31;
    // (each product of two sizes is below 2^62; the division keeps the third factor from overflowing)
    return (int64_t)h * w < (lim + C - 1) / C && (int64_t)Hm * Wm < (lim + C - 1) / C && (int64_t)H * W < (lim + C - 1) / C;
}

// reference models/TTA_wrapper_CTS.py multi_scale_aug: Python's int() truncates, its `/` is a double division
static inline void dtt_cts_size(int H, int W, int base_size, double scale, int *new_h, int *new_w)
{
    const int long_size = (int)((double)base_size * scale + 0.5);
    if (H > W) {
        *new_h = long_size;
        *new_w = (int)((double)((int64_t)W * long_size) / (double)H + 0.5);
    } else {
        *new_w = long_size;
        *new_h = (int)((double)((int64_t)H * long_size) / (double)W + 0.5);
    }
}

// number of windows along an axis of length n (reference TTA_wrapper_CTS.py forward: rows / cols); < 1 = none
static inline int dtt_window_count(int n, int crop, int stride)
{
    return (int)ceil(1.0 * (double)(n - crop) / (double)stride) + 1;
}

// window r of that axis: [lo, hi)
static inline void dtt_window(int n, int crop, int stride, int r, int *lo, int *hi)
{
    int64_t a = (int64_t)r * stride;
    int64_t b = a + crop < n ? a + crop : n;
    a = b - crop > 0 ? b - crop : 0;
    *lo = (int)a;
    *hi = (int)b;
}

// cnt[i] = number of windows over position i (cnt has n entries); returns the window count
static inline int dtt_window_counts(int n, int crop, int stride, int32_t *cnt)
{
    const int count = dtt_window_count(n, crop, stride);
    for (int i = 0; i < n; ++i)
        cnt[i] = 0;
    for (int r = 0; r < count; ++r) {
        int lo, hi;
        dtt_window(n, crop, stride, r, &lo, &hi);
        for (int i = lo; i < hi; ++i)
            cnt[i] += 1;
    }
    return count;
}
