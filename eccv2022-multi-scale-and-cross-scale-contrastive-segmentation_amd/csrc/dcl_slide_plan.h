// dcl_slide_plan.h -- what dcl_slide.hip, dcl_slide_capi.cpp and the host tests share: the shape test, the PASCAL-Context window
// grid (no shift-back), the cover count of a window table and (dcl_bilinear.h) the bilinear source index.  Host-compilable: plain
// functions, no HIP.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/dcl_slide.h"
#include "dcl_bilinear.h"

void dsw_set_error(const char *fmt, ...);

// a * b * c * d < 2^31 for positive ints, without overflow (every partial product is tested before the next factor)
static inline bool dsw_below_2_31(int64_t a, int64_t b, int64_t c, int64_t d)
{
    const int64_t lim = 1ll << 31;
    int64_t p = a;
    if (p >= lim)
        return false;
    p *= b;
    if (p >= lim)
        return false;
    p *= c;
    if (p >= lim)
        return false;
    p *= d;
    return p < lim;
}

static inline bool dsw_crops_ok(int Cin, int H, int W, int nh, int nw, int R, int Q, int wh, int ww)
{
    if (Cin < 1 || Cin > DSW_MAX_CIN || H < 1 || W < 1 || nh < 1 || nw < 1 || wh < 1 || ww < 1)
        return false;
    if (R < 1 || R > DSW_MAX_WIN || Q < 1 || Q > DSW_MAX_WIN)
        return false;
    return dsw_below_2_31(Cin, H, W, 1) && dsw_below_2_31(2 * R * Q, Cin, wh, ww);
}

static inline bool dsw_gather_ok(int C, int h, int w, int wh, int ww, int R, int Q, int Hc, int Wc)
{
    if (C < 1 || C > DSW_MAX_C || h < 1 || w < 1 || wh < 1 || ww < 1 || Hc < 1 || Wc < 1 || h > wh || w > ww)
        return false;
    if (R < 1 || R > DSW_MAX_WIN || Q < 1 || Q > DSW_MAX_WIN)
        return false;
    return dsw_below_2_31(R * Q, C, h, w) && dsw_below_2_31(C, Hc, Wc, 1);
}

// reference models/TTA_wrapper_PC.py forward: rows / cols of an axis of length n (already padded to the crop); < 1 = none
static inline int dsw_pc_window_count(int n, int crop, int stride)
{
    return (int)ceil(1.0 * (double)(n - crop) / (double)stride) + 1;
}

// window r of that axis: [lo, hi), not shifted back -- the last one may be partial
static inline void dsw_pc_window(int n, int crop, int stride, int r, int *lo, int *hi)
{
    const int64_t a = (int64_t)r * stride;
    const int64_t b = a + crop < n ? a + crop : n;
    *lo = (int)a;
    *hi = (int)b;
}

// cnt[i] = number of windows [lo[r], min(lo[r] + wh, n)) over position i (cnt: n entries or NULL); the smallest count, -1 = bad table
static inline int dsw_cover(int n, int wh, const int *lo, int R, int32_t *cnt)
{
    if (n < 1 || wh < 1 || R < 1 || R > DSW_MAX_WIN || !lo)
        return -1;
    for (int r = 0; r < R; ++r)
        if (lo[r] < 0 || lo[r] >= n)
            return -1;
    int least = R + 1;
    for (int i = 0; i < n; ++i) {
        int c = 0;
        for (int r = 0; r < R; ++r)
            c += (i >= lo[r] && (int64_t)i < (int64_t)lo[r] + wh) ? 1 : 0;
        if (cnt)
            cnt[i] = c;
        least = c < least ? c : least;
    }
    return least;
}
