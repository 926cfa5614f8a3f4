// dcl_convbwd_plan.h -- the launch plan of libdcl_convbwd.so (include/dcl_convbwd.h): data-gradient tile and grid from
// dcl_conv_plan.h, weight-gradient plan from dcl_wgrad_plan.h for the workgroups the tiles leave free.  Read by the host entries
// (dcl_convbwd_capi.cpp) and by the launch (dcl_convbwd.hip): one value decides what is launched and what `part` must hold.
#pragma once
#include "dcl_conv_plan.h"
#include "dcl_wgrad_plan.h"
#include "../../include/dcl_convbwd.h"

__attribute__((visibility("hidden"))) void dcb_set_error(const char *fmt, ...);      // not part of the C ABI

constexpr int DCB_CUS = 256;            // compute units = workgroups of one round (both bodies run one workgroup per CU)

struct DcbPlan {
    int ok;                 // 0: shape / tile not taken
    int R, P;               // data-gradient tile
    unsigned nd, nd8;       // data-gradient workgroups; rounded up to a multiple of 8, so that the weight-gradient workgroups behind
                            // them keep id & 7 = XCD in their own numbering (the padding workgroups leave at once)
    int target;             // workgroups the weight gradient was planned for
    WgradPlan w;
};

static inline DcbPlan dcb_make_plan(int N, int Cin, int Cout, int H, int W, int tile_r, int tile_p, int wg_target)
{
    DcbPlan d = {};
    if (N <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || (Cin & 15) || (Cout & 15) || (W & 7))
        return d;
    if ((size_t)8 * H * W + (size_t)H * W >= ((size_t)1 << 31) || (size_t)(Cin > Cout ? Cin : Cout) * H * W * 4 >= ((size_t)1 << 32))
        return d;           // the bodies' 32-bit offsets
    if (wg_target != 0 && (wg_target < 32 || wg_target > DCB_CUS || (wg_target & 7)))
        return d;
    // data gradient: the convolution of gy (Cout channels) that produces Cin channels
    conv_auto_tile(N, Cin, H, W, Cout / 16, 1, 0, 0, tile_r, tile_p, DCL_CONV_MIN_WGS, d.R, d.P);
    if (d.R != 3 || (d.P != 4 && d.P != 2))
        return d;
    const long nd = (long)((W + TW - 1) / TW) * ((H + 4 * d.P - 1) / (4 * d.P)) * N * (((Cin + 31) / 32 + d.R - 1) / d.R);
    if (nd > (1 << 20))
        return d;
    d.nd = (unsigned)nd;
    d.nd8 = (d.nd + 7u) & ~7u;
    const int free_cus = DCB_CUS - (int)d.nd8;
    d.target = wg_target ? wg_target : (free_cus >= DCB_CUS / 2 ? free_cus : DCB_CUS);
    // (wave form: four waves per workgroup, an eighth of the workgroups per XCD)
    d.w = wgrad_plan_stride1(N, Cin, Cout, H, W, 1, WgradTune{}, d.target, d.target / 2);
    if (d.w.family != WGRAD_DMA || d.w.nco != 3 || d.w.nci != 1 || (!d.w.wave_mode && d.w.rect_mode))
        return d;
    d.ok = 1;
    return d;
}

// the automatic plan serves the shape, and the tiles leave at least half the chip to the weight gradient
static inline bool dcb_shape_ok(int N, int Cin, int Cout, int H, int W)
{
    const DcbPlan d = dcb_make_plan(N, Cin, Cout, H, W, 0, 0, 0);
    return d.ok && DCB_CUS - (int)d.nd8 >= DCB_CUS / 2;
}
