// dcl_wgrad_plan.h -- host side of the 3x3 weight gradient for both libraries that launch it: the launch plan of the stride-1
// kernels (k_wgrad3x3, k_wgrad3x3d) and the kernel arguments made from it.  dcl_wgrad3x3.hip plans with its tuning switches
// (dcl_wgrad3x3_set_*), dcl_convbwd.hip with their defaults and the workgroups its data-gradient tiles leave free.
#pragma once
#include "dcl_wgrad.h"

// The tuning switches of the plan; the defaults are the product's.
struct WgradTune {
    int tile_nco = 0, tile_nci = 0;     // tiles per wave (dcl_wgrad3x3_set_tile), 0 = automatic
    int force_nx = 0;                   // pixel splits per tile pair (0 = automatic)
    int variant = -1;                   // 0 = MFMA-order operand loads (dcl_wgrad3x3.hip), -1 / 2 = LDS-DMA staging (dcl_wgrad3x3d.hip)
    int wave_band = 0;                  // wave form: rows per column of the traversal (0 = whole strips: the default -- 32-row bands
                                        // re-use the halo lines in L2 but pay a column prologue every 32 rows: 2.01 vs 1.91 ms on the head)
    int strip_group = 1;                // waves of a workgroup on adjacent strips (WgradArgs::grp)
    int wave_mode = 2;                  // 129 .. 256 tile pairs of the (3, 1) tile: pixel splits dealt out to waves (dcl_wgrad3x3d.hip);
                                        // 2 = a workgroup's waves take the same split of four neighbouring pairs, 1 = four splits of a pair
};

// (A third variant -- workgroups handing the dY rows of a co group to each other through LDS, optional stream-K partition
// -- reached the same kernel times as the LDS-DMA kernel with slabs four times the size and lost in the training step; it
// was retired from the library in round 3: tools/probes/retired/dcl_wgrad3x3s.hip.)
// per-wave kernel: operands staged by LDS-DMA (dcl_wgrad3x3d.hip) unless variant 0 asks for the direct loads; the direct
// loads also serve tensors beyond the DMA kernel's 32-bit offsets and the zero-inserted stride-2 form
static inline bool wgrad_use_dma(const WgradTune &t, int C, int H, int W)
{
    return t.variant != 0 && (size_t)C * H * W * 4 < ((size_t)1 << 32);
}

// The launch plan of the stride-1 kernels (stride 2: the zero-inserted form on k_wgrad3x3).  wg_target: workgroups the launch aims
// at (pixel splits = target / tile pairs) -- 256, one per CU, or what another kernel of the same launch leaves free; xcd_waves:
// waves per XCD the wave form deals its jobs to (128 = all of them; its grid is 8 * xcd_waves / 4 workgroups).
static inline WgradPlan wgrad_plan_stride1(int N, int Cin, int Cout, int H, int W, int stride, const WgradTune &t, int wg_target,
                                           int xcd_waves)
{
    WgradPlan p = {};
    const int cot = Cout / 16, cit = Cin / 16;
    // Tiles per wave, measured on the HRNet-W48 shapes at batch 12 (tools/wgrad_tiles.py, and bench.py with
    // DCL_WGRAD_TILE: the step decides, the slabs of the larger tiles cost HBM traffic that the standalone timing does not
    // show): three co tiles x one ci tile wherever the co tiles divide by three (48 ... 720 channels: step 122.3 ms
    // against 122.8 with (2, 2) at 192 and (3, 2) at 384 channels); else the four-tile wave (2, 2), (2, 1), (1, 2), (1, 1).
    if (cot % 3 == 0) {
        p.nco = 3;
        p.nci = 1;
    } else {
        p.nco = (cot % 2 == 0) ? 2 : 1;
        p.nci = (cit % 2 == 0) ? 2 : 1;
    }
    if (t.tile_nco > 0 && cot % t.tile_nco == 0)
        p.nco = t.tile_nco;
    if (t.tile_nci > 0)
        p.nci = t.tile_nci;
    if (p.nco * p.nci > 4)      // a forced ci count beside three co tiles: no six-tile wave (as dcl_wgrad_s2_plan)
        p.nci = 1;
    const bool dma = stride == 1 && wgrad_use_dma(t, Cin > Cout ? Cin : Cout, H, W);
    p.family = dma && dcl_wgrad_dma_supported(p.nco, p.nci) ? WGRAD_DMA : WGRAD_DIRECT;
    p.ncig = (cit + p.nci - 1) / p.nci;
    p.npairs = (cot / p.nco) * p.ncig;
    p.units = N * ((W + 31) / 32);          // columns: (image, 32-pixel strip), H input rows each
    // One workgroup (4 waves = 4 splits of one pair) per CU is all that fits (a wave owns most of its SIMD's
    // registers): at most 256 workgroups, or the stragglers run as a second round and double the kernel time.
    int nx = wg_target / p.npairs;
    if (t.force_nx > 0)
        nx = t.force_nx;
    if (nx < 1)
        nx = 1;         // more tile pairs than CUs (head convolution): one pixel split; finer splits were tried and
                        // lose (3 splits fill the last round better but take 26 ms against 12.5 ms)
    p.S = 4 * nx;
    if ((long long)p.S > (long long)p.units * H)
        p.S = p.units * H;
    // one workgroup per pair and CUs left over: the splits go to single waves, S = 128 / (pairs of one XCD) of them (with
    // fewer than 128 waves per XCD a workgroup per pair does not fit in one round at all: any S >= 1 there)
    const int sw = xcd_waves / ((p.npairs + 7) / 8);
    const bool wm = dma && t.wave_mode && t.force_nx == 0 && p.npairs > 128 && p.npairs <= 256 && (sw > 4 || (xcd_waves < 128 && sw >= 1)) &&
                    dcl_wgrad_dma_wave_mode_supported(p.nco, p.nci) && (long long)sw <= (long long)p.units * H;
    if (wm)
        p.S = sw;
    p.wave_mode = wm ? t.wave_mode : 0;
    p.band = (wm && t.wave_band > 0 && H % t.wave_band == 0 && H > t.wave_band) ? t.wave_band : H;
    p.nx = (p.S + 3) / 4;                                    // workgroups per pair (4 splits each)
    // adjacent strips for the waves of a workgroup (dcl_wgrad3x3d.hip): unclamped split count, strips in fours / pairs
    p.grp = 1;
    if (t.strip_group && !wm && p.S == 4 * p.nx && p.S >= 4) {
        const int strips = (W + 31) / 32;
        p.grp = (strips % 4 == 0) ? 4 : ((strips % 2 == 0) ? 2 : 1);
    }
    p.grid = (unsigned)(p.npairs * p.nx);        // exactly the populated workgroups, <= 256 whenever pairs <= 256
    p.rect_i = p.ncig >= 16 ? 16 : (p.ncig >= 8 ? 8 : (p.ncig >= 4 ? 4 : (p.ncig >= 2 ? 2 : 1)));
    p.rect_c = 32 / p.rect_i;
    p.rect_mode = p.npairs > 128 ? 1 : 0;
    if (p.rect_mode) {
        const int ncog = p.npairs / p.ncig;
        const int units_r = ((ncog + p.rect_c - 1) / p.rect_c) * ((p.ncig + p.rect_i - 1) / p.rect_i) * p.nx;
        p.grid = (unsigned)(((units_r + 7) / 8) * 8 * 32);
    }
    if (wm)
        p.grid = (unsigned)(2 * xcd_waves);     // 8 XCDs x xcd_waves / 4 workgroups
    p.slabs = wm ? p.S : p.nx;                  // one slab per wave-level split, or per workgroup (4 splits)
    return p;
}

// kernel arguments of a planned launch
static inline void wgrad_fill_args(WgradArgs &a, const WgradPlan &p, const float *x, const float *dy, float *part, const float *xamax,
                                   int xcount, const float *gamax, int gcount, int N, int Cin, int Cout, int H, int W, int stride,
                                   const float *pre_sc, const float *pre_sh)
{
    a.x = x;
    a.dy = dy;
    a.part = part;
    a.xamax = xamax;
    a.gamax = gamax;
    a.xcount = xcount;
    a.gcount = gcount;
    a.N = N;
    a.Cin = Cin;
    a.Cout = Cout;
    a.H = H;
    a.W = W;
    a.Hd = stride == 2 ? (H - 1) / 2 + 1 : H;
    a.Wd = stride == 2 ? W / 2 : W;
    a.strips = (W + 31) / 32;
    a.nseg = 1;
    a.pre_sc = pre_sc;
    a.pre_sh = pre_sh;
    a.units = p.units;
    a.S = p.S;
    a.ncig = p.ncig;
    a.npairs = p.npairs;
    a.nx = p.nx;
    a.rect_c = p.rect_c;
    a.rect_i = p.rect_i;
    a.rect_mode = p.rect_mode;
    a.wave_mode = p.wave_mode;
    a.band = p.band;
    a.grp = p.grp;
}
