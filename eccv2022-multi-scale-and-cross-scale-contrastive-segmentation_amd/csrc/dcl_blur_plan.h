// dcl_blur_plan.h -- what dcl_blur.hip, dcl_blur_capi.cpp and the host tests share: the host arithmetic of libdcl_blur.so
// (include/dcl_blur.h), once.  The box of a radius, the limits, the tile walk of a pass in LDS and the reflected row.
// Host-compilable: plain functions, no HIP (DBL_HD is empty unless a HIP compiler reads this).
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/dcl_blur.h"

#ifdef __HIPCC__
#define DBL_HD __host__ __device__
#else
#define DBL_HD
#endif

void dbl_set_error(const char *fmt, ...);

// PIL's _gaussian_blur_radius(R, passes = 3) and the two weights of ImagingLineBoxBlur, in double; the weights rounded to fp32 last
struct DblBox {
    int l;          // whole taps on either side of the centre
    float ww, fw;   // weight of the 2 l + 1 inner taps, and of the two outer ones
};

static inline DblBox dbl_box_of(int radius)
{
    const double s2 = (double)radius * (double)radius / 3.0;
    const double L = sqrt(12.0 * s2 + 1.0);
    const double l = floor((L - 1.0) / 2.0);
    const double a = (2.0 * l + 1.0) * (l * (l + 1.0) - 3.0 * s2) / (6.0 * (s2 - (l + 1.0) * (l + 1.0)));
    const double fr = l + a;
    const double ww = 1.0 / (2.0 * fr + 1.0);
    DblBox b;
    b.l = (int)l;
    b.ww = (float)ww;
    b.fw = (float)((1.0 - (2.0 * l + 1.0) * ww) / 2.0);
    return b;
}

static inline bool dbl_blur_ok(int C, int h, int w, int radius)
{
    return radius >= 1 && radius <= DBL_MAX_RADIUS && C >= 1 && C <= DBL_MAX_CHANNELS && h >= 1 && w >= 1 &&
           (int64_t)C * h * w < (1ll << 31);
}

static inline bool dbl_pad_ok(int C, int h, int w, int top, int bottom)
{
    return C >= 1 && C <= DBL_MAX_CHANNELS && h >= 1 && w >= 1 && top >= 0 && bottom >= 0 && top <= h - 1 && bottom <= h - 1 &&
           (int64_t)C * ((int64_t)h + top + bottom) * w < (1ll << 31);
}

// The three passes of one axis on a tile.  A tile of T outputs that starts at t0 of an axis of length n is staged with a halo of
// 3 (l + 1) on either side: local index j holds global index t0 - 3 (l + 1) + j.  Pass p = 1, 2, 3 is evaluated on the local range
// [p (l + 1), T + (6 - p) (l + 1)) and only where the global index lies inside the axis; every tap it reads, clamped to [0, n - 1],
// then lies in the range of pass p - 1 (p = 0: the staged values).
DBL_HD static inline int dbl_halo(int l) { return 3 * (l + 1); }
DBL_HD static inline int dbl_ext(int T, int l) { return T + 2 * dbl_halo(l); }
DBL_HD static inline int dbl_pass_lo(int p, int l) { return p * (l + 1); }
DBL_HD static inline int dbl_pass_hi(int p, int T, int l) { return T + (6 - p) * (l + 1); }
// local index of the tap d of global index g
DBL_HD static inline int dbl_tap(int g, int d, int n, int base)
{
    int k = g + d;
    k = k < 0 ? 0 : k;
    k = k > n - 1 ? n - 1 : k;
    return k - base;
}

// source row of output row y of dbl_pad_rows
DBL_HD static inline int dbl_reflect_row(int y, int top, int h)
{
    int r = y - top;
    if (r < 0)
        r = -r;
    if (r > h - 1)
        r = 2 * (h - 1) - r;
    return r;
}
