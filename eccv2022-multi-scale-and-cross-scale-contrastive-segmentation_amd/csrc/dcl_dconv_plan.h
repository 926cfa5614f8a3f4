// dcl_dconv_plan.h -- what dcl_dconv.hip and dcl_dconv_capi.cpp share: the shape test, the live-tap mask, the slab count of the
// weight gradient, the workspace and fragment sizes, the error text.
#pragma once
#include <stdint.h>

#include "../../include/dcl_dconv.h"

__attribute__((visibility("hidden"))) void ddc_set_error(const char *fmt, ...);      // not part of the C ABI

static inline int64_t ddc_r256(int64_t x) { return (x + 255) / 256 * 256; }
static inline int ddc_ceil_div(int a, int b) { return (a + b - 1) / b; }

static inline bool ddc_channels_ok(int C) { return C >= 16 && C <= DDC_MAX_C && C % 16 == 0; }

static inline bool ddc_shape_ok(int N, int Ci, int Co, int H, int W, int d)
{
    if (N < 1 || N > DDC_MAX_N || H < 1 || W < 1 || d < 1 || d > DDC_MAX_D || !ddc_channels_ok(Ci) || !ddc_channels_ok(Co))
        return false;
    const int64_t lim = 1ll << 31, hw = (int64_t)H * W;
    if (hw >= lim)
        return false;
    return (int64_t)N * Ci * hw < lim && (int64_t)N * Co * hw < lim && 9ll * Co * Ci < lim;
}

// bit 3 ky + kx: tap (ky, kx) reaches the image from at least one pixel
static inline unsigned ddc_live_mask(int H, int W, int d)
{
    if (H < 1 || W < 1 || d < 1)
        return 0;
    unsigned m = 0;
    for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx)
            if ((ky == 1 || d < H) && (kx == 1 || d < W))
                m |= 1u << (3 * ky + kx);
    return m;
}

static inline int ddc_popcount9(unsigned m)
{
    int n = 0;
    for (int t = 0; t < 9; ++t)
        n += (m >> t) & 1;
    return n;
}

static inline int64_t ddc_wgrad_units(int N, int H, int W)
{
    return (int64_t)N * (((int64_t)H * W + DDC_WG_CHUNK_P - 1) / DDC_WG_CHUNK_P);
}

// units of one slab
static inline int64_t ddc_slab_units(int N, int Ci, int Co, int H, int W, int d)
{
    const int64_t units = ddc_wgrad_units(N, H, W);
    const int64_t tiles = (int64_t)ddc_ceil_div(Co, DDC_WG_TILE) * ddc_ceil_div(Ci, DDC_WG_TILE) * ddc_popcount9(ddc_live_mask(H, W, d));
    int64_t want = (DDC_WG_TARGET + tiles - 1) / tiles;
    if (want < 1)
        want = 1;
    if (want > DDC_MAX_SLABS)
        want = DDC_MAX_SLABS;
    int64_t most = units / DDC_SLAB_MIN_UNITS;
    if (most < 1)
        most = 1;
    if (want > most)
        want = most;
    return (units + want - 1) / want;
}

static inline int ddc_slab_count(int N, int Ci, int Co, int H, int W, int d)
{
    const int64_t units = ddc_wgrad_units(N, H, W), per = ddc_slab_units(N, Ci, Co, H, W, d);
    return (int)((units + per - 1) / per);      // then no slab is left empty
}

static inline int64_t ddc_ws_bytes(int op, int N, int Ci, int Co, int H, int W, int d)
{
    if (!ddc_shape_ok(N, Ci, Co, H, W, d))
        return -1;
    switch (op) {
    case DDC_OP_FWD:
    case DDC_OP_DGRAD: return 256;
    case DDC_OP_WGRAD:
        return 512 + ddc_r256(4ll * ddc_slab_count(N, Ci, Co, H, W, d) * ddc_popcount9(ddc_live_mask(H, W, d)) * Co * Ci);
    }
    return -1;
}

static inline int64_t ddc_pack_bytes(int Co, int Ci, int transposed)
{
    if (!ddc_channels_ok(Ci) || !ddc_channels_ok(Co))
        return -1;
    const int rows = transposed ? Ci : Co, cols = transposed ? Co : Ci;
    return 36ll * ((rows + 31) / 32 * 32) * cols;
}
