// dcl_conv_plan.h -- host side of the direct f16x3 convolution for both libraries that launch conv_body: the automatic tile and the
// ConvArgs set-up.  dcl_conv3x3.hip plans with its tuning switch (dcl_conv3x3_set_min_workgroups), dcl_convbwd.hip with the default.
#pragma once
#include "dcl_conv_body.h"

constexpr int DCL_CONV_MIN_WGS = 96;    // automatic tile: fewest workgroups a launch may have before the rows per wave are halved.
// 192 (one round of 256 CUs three quarters full) until round 4; 96 since: the 192 / 384-channel branch convolutions then run as 96
// workgroups with twice the rows per wave -- 22-33 % less CU-time per launch at 55 % more latency -- and leave the rest of the chip to
// the other branches' kernels: step 90.7 -> 89.7 ms over three alternating pairs (profiles/r04_ab_conv_min_wgs.json)

// (R, P) = channel tiles x rows per wave of a launch; tile_r / tile_p > 0 force them
static inline void conv_auto_tile(int N, int Cout, int Ho, int Wo, int nchunk, int stride, int phases, int onetap, int tile_r, int tile_p,
                                  int min_wgs, int &R, int &P)
{
    const int mtiles = (Cout + 31) / 32;
    if (phases == 2) {
        // merged parity classes: 4 R P accumulator tiles per wave, at most 12 (16 spill) -- (3, 1), (2, 1), (1, 2 | 1); tiles run
        // over the STORED gradient, ceil(Ho / 2) x ceil(Wo / 2)
        R = mtiles % 3 == 0 ? 3 : (mtiles == 1 ? 1 : 2);
        P = R == 1 ? 2 : 1;
        auto wgs = [&](int p) {
            return (long)(((Wo + 1) / 2 + TW - 1) / TW) * (((Ho + 1) / 2 + 4 * p - 1) / (4 * p)) * N * ((mtiles + R - 1) / R);
        };
        while (P > 1 && wgs(P) < min_wgs)
            P >>= 1;
        if (tile_r > 0 && tile_p > 0 && 4 * tile_r * tile_p <= 12)
            R = tile_r, P = tile_p;
        return;
    }
    R = tile_r, P = tile_p;
    if (stride == 2)
        P = 1;
    if (R <= 0 || P <= 0 || (stride == 2 && tile_r <= 0)) {
        // measured on the four BasicBlock shapes of HRNet-W48 at batch 12 (tools/bench_conv3x3.py --tiles):
        // channel tiles per wave in threes when that leaves no padded tile, else pairs; the most rows per wave
        // that still give ~one workgroup per CU; tiny images fall back to single-tile waves to get enough
        // workgroups.
        R = (mtiles % 3 == 0 || mtiles >= 20) ? 3 : (mtiles == 1 ? 1 : 2);     // >= 20 tiles: one padded tile is < 5 %
        if (mtiles == 5 && stride == 1 && !onetap)
            R = 3;      // five tiles pad to six either way, and the (3, P) wave runs 324 P / 4 MFMAs per staged chunk against 216:
                        // the head's 720 -> 144 data gradient (45 chunks), (2, 4) tile 4.17 ms = 0.21 of the roofline
        auto wgs = [&](int r, int p) {
            if (phases)
                return (long)(((Wo + 1) / 2 + TW - 1) / TW) * (((Ho + 1) / 2 + 4 * p - 1) / (4 * p)) * N *
                       ((mtiles + r - 1) / r) * 4;
            return (long)((Wo + TW - 1) / TW) * ((Ho + 4 * p - 1) / (4 * p)) * N * ((mtiles + r - 1) / r);
        };
        P = stride == 2 ? 1 : 4;
        while (P > 1 && wgs(R, P) < min_wgs)
            P >>= 1;
        if (R == 2 && P == 4 && stride == 1 && !phases && nchunk <= 4)
            P = 2;              // the (2, 2) tile runs two workgroups per CU (k_conv3x3_o2): 81 vs 100 us at 48 channels;
                                // a short K loop is mostly prologue / epilogue, which two co-resident workgroups
                                // hide.  With a long one (the 512-channel decoder convolutions of UPerNet) the (2, 4)
                                // tile's reuse of the weight fragments wins: 415 vs 386 TFLOP/s
        if (P == 1 && wgs(R, P) < 128)
            R = 1;
    }
}

// tensors and shape of a plain launch: 3x3, input stored as it is read (up = 1), no parity classes; the caller adjusts the
// geometry fields for stride 2 / zero-inserted inputs / one tap and then sets the tile grid
static inline void conv_fill_args(ConvArgs &a, const float *x, int N, int Cin, int H, int W, const void *wp, int Cout, const float *xamax,
                                  int xcount, const float *wamax, const float *addend, const float *bias, float *y,
                                  const float *pre_sc, const float *pre_sh)
{
    a.x = x;
    a.wp = (const uint4 *)wp;
    a.y = y;
    a.addend = addend;
    a.bias = bias;
    a.xamax = xamax;
    a.wamax = wamax;
    a.xcount = xcount;
    a.N = N;
    a.Cin = Cin;
    a.Cout = Cout;
    a.H = a.Hs = a.Ho = H;
    a.W = a.Ws = a.Wo = W;
    a.up = 1;
    a.phases = 0;
    a.onetap = 0;
    a.nchunk = (Cin + 15) / 16;
    a.pre_sc = pre_sc;
    a.pre_sh = pre_sh;
}

// tile grid of the (R, P) tile; returns the workgroup count
// (phases: tiles over one parity class of the output, ceil(Ho / 2) x ceil(Wo / 2) pixels, four classes per tile)
static inline unsigned conv_fill_grid(ConvArgs &a, int R, int P)
{
    a.tiles_x = ((a.phases ? (a.Wo + 1) / 2 : a.Wo) + TW - 1) / TW;
    a.tiles_y = ((a.phases ? (a.Ho + 1) / 2 : a.Ho) + 4 * P - 1) / (4 * P);
    const int mtiles = (a.Cout + 31) / 32;
    a.groups = (mtiles + R - 1) / R;
    return (unsigned)(a.tiles_x * a.tiles_y * a.N * a.groups * (a.phases == 1 ? 4 : 1));
}
