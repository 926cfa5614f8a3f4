// dcl_wgrad.h -- what the weight-gradient kernels share (dcl_wgrad3x3.hip, dcl_wgrad3x3d.hip, dcl_wgrad3x3_s2.hip): the launch
// arguments and the launch plan on the host side, and the device pieces every kernel is built from -- operand scales, the
// workgroup -> (tile pair, pixel split) decode, the PRE map, the LDS combine of the four waves and the slab store.
#pragma once
#include "dcl_f16x3.h"

struct WgradArgs {
    const float *x, *dy;
    float *part;                 // [S][9][Cout][Cin]
    const float *xamax, *gamax;
    int xcount, gcount;
    int N, Cin, Cout, H, W;
    int Hd, Wd;                  // stored size of dy (= H, W; or the even samples of a zero-inserted dy: stride 2)
    int strips, nseg, units, S, ncig, npairs, nx;
    int rect_c, rect_i, rect_mode;  // many pairs: pair-grid rectangle that shares an XCD (rect_c * rect_i = 32)
    int wave_mode;               // 1: S pixel splits per pair dealt out to WAVES (k_wgrad3x3d<.., true>), one slab per split
    int band;                    // rows per column of the traversal (H, or a divisor of H: wave form, see k_wgrad3x3d)
    int grp;                     // 1 | 2 | 4: the waves of a workgroup walk `grp` ADJACENT strips over the same rows (k_wgrad3x3d)
    const float *pre_sc, *pre_sh;   // k_wgrad3x3d PRE forms: the operand is relu(x * pre_sc[ci] + pre_sh[ci]); NULL otherwise
};

// The launch plan of dcl_wgrad3x3_f16x3 / dcl_wgrad3x3_pre_f16x3 for one shape (wgrad_plan, dcl_wgrad3x3.hip): what is launched,
// what dcl_wgrad3x3_splits tells the caller to allocate and what the slab reduction sums are all read from this one value.
enum WgradFamily {
    WGRAD_DIRECT,       // k_wgrad3x3: operands loaded in MFMA order (stride 2: zero-inserted dy)
    WGRAD_DMA,          // k_wgrad3x3d: stride 1, LDS-DMA staging
    WGRAD_S2,           // k_wgrad3x3_s2: stride 2 over the output pixels, operands loaded in MFMA order
    WGRAD_S2_DMA        // k_wgrad3x3_s2d: the same with the x rows staged by LDS-DMA
};
struct WgradPlan {
    WgradFamily family;
    int nco, nci;                   // 16 x 16 tiles per wave
    int ncig, npairs;               // ci groups; (co group, ci group) pairs
    int units, S, nx;               // columns (image, strip); pixel splits; workgroups per pair
    int wave_mode, band, grp;       // as in WgradArgs
    int rect_c, rect_i, rect_mode;
    unsigned grid;
    int slabs;                      // slabs of `part` the kernel writes
};

// dcl_wgrad3x3d.hip: the stride-1 kernel with LDS-DMA operand staging; same grid, slabs and arguments as k_wgrad3x3
inline bool dcl_wgrad_dma_supported(int nco, int nci) { return nco >= 1 && nco <= 3 && nci >= 1 && nci <= 2 && nco * nci <= 4; }
inline bool dcl_wgrad_dma_wave_mode_supported(int nco, int nci) { return nco == 3 && nci == 1; }
int dcl_wgrad_dma_launch(const WgradArgs &a, int nco, int nci, dim3 grid, hipStream_t s);
// dcl_wgrad3x3_s2.hip: the output-pixel formulation of stride 2.  The plan fills tile, splits, grid, slabs and family; the launch
// takes tensors, amax slots and the PRE map from `a` (kernel only: the caller sums the slabs).
bool dcl_wgrad_s2_supported(int H, int W);
void dcl_wgrad_s2_set_dma(int on);
void dcl_wgrad_s2_plan(int N, int Cin, int Cout, int H, int W, int force_nco, int force_nci, WgradPlan &p);
int dcl_wgrad_s2_launch(const WgradArgs &a, const WgradPlan &p, hipStream_t s);

// every dispatch chain of the family ends in this: no instantiated kernel matched the tile
#define DCL_WGRAD_NO_KERNEL(name, nco, nci)                                          \
    do {                                                                             \
        dcl_set_error("%s: no %s kernel for the (%d, %d) tile", __func__, name, nco, nci); \
        return DCL_EUNSUPPORTED;                                                     \
    } while (0)

// Accumulator clear of f32x4 acc[NCO][NCI][NT].  A macro, not a function, on purpose: with the array handed to an (inlined)
// function the register allocation of k_wgrad3x3, k_wgrad3x3_s2 and k_wgrad1x1d comes out differently (+-4 .. 12 VGPRs); expanded
// in place the kernels compile to what they were (profiles/wgrad_shared_pieces_isa.txt).
#define DCL_WGRAD_CLEAR(acc, NT)                              \
    _Pragma("unroll") for (int t_ = 0; t_ < NCO; ++t_)        \
    _Pragma("unroll") for (int u_ = 0; u_ < NCI; ++u_)        \
    _Pragma("unroll") for (int k_ = 0; k_ < (NT); ++k_)       \
        (acc)[t_][u_][k_] = f32x4{0.f, 0.f, 0.f, 0.f}

namespace {

// Operand scales sx, sg from the producers' partial maxima (xcount / gcount slots), reduced over the workgroup; wm = 8 floats of
// LDS.  Holds a __syncthreads(): all four waves call it exactly once.
template <class Args>
__device__ __forceinline__ void wgrad_scales(const Args &a, float *wm, float &sx, float &sg)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float mx = 0.f, mg = 0.f;
    for (int i = tid; i < a.xcount; i += 256)
        mx = fmaxf(mx, a.xamax[i]);
    for (int i = tid; i < a.gcount; i += 256)
        mg = fmaxf(mg, a.gamax[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        mg = fmaxf(mg, __shfl_xor(mg, o, 64));
    }
    if (lane == 0) {
        wm[wave] = mx;
        wm[4 + wave] = mg;
    }
    __syncthreads();
    sx = pow2_scale(fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3])));
    sg = pow2_scale(fmaxf(fmaxf(wm[4], wm[5]), fmaxf(wm[6], wm[7])));
}

// The decodes take the workgroup id `bid` from the caller (blockIdx.x; the fused backward kernel of dcl_convbwd.hip puts the
// weight-gradient workgroups behind its data-gradient tiles and hands in the id counted from the first of them).
// XCD-aware decode of the 1-D grid: consecutive workgroup ids go round-robin over the 8 XCDs, so
// id = xcd + 8 * (pair + npairs * hi) puts every (co group, ci group) pair of one pixel split on the SAME XCD,
// next to each other in dispatch order -- they stream the same dy / x rows, which then come out of that
// XCD's L2 instead of being fetched once per pair.
template <class Args>
__device__ __forceinline__ void wgrad_decode_flat(const Args &a, const unsigned bid, int &pair, int &xsplit)
{
    const int nx8 = a.nx & ~7, main_blocks = nx8 * a.npairs;
    if ((int)bid < main_blocks) {
        const int xcd = bid & 7, rest = bid >> 3;
        pair = rest % a.npairs;
        xsplit = (rest / a.npairs) * 8 + xcd;
    } else {                                // the nx % 8 left-over pixel splits, in plain order
        const int rest = bid - main_blocks;
        pair = rest % a.npairs;
        xsplit = nx8 + rest / a.npairs;
    }
}

// Many tile pairs, one pixel split (large channel counts, a.rect_mode): every workgroup streams ALL pixels, so what
// matters is which workgroups share an L2 while they do.  The (co group x ci group) grid is cut into
// rectangles of rect_c x rect_i = 32 pairs -- they read rect_c + rect_i operand row sets instead of 64 --
// and rectangle q of XCD k takes the ids k + 8 * (32 q .. 32 q + 31): one XCD (32 CUs), adjacent dispatch
// slots.  (Head convolution, 15 x 45 pairs: FETCH_SIZE 28.0 GiB -> 16.5 GiB per launch, 12.9 -> 12.5 ms.)
// False: padding of the last rectangles (the whole workgroup leaves).
__device__ __forceinline__ bool wgrad_decode_rect(const WgradArgs &a, const unsigned bid, int &pair, int &xsplit)
{
    const int xcd = bid & 7, slot = bid >> 3;
    const int unit = (slot >> 5) * 8 + xcd, idx = slot & 31;       // unit = (pixel split, rectangle)
    const int ncog = a.npairs / a.ncig, rects_i = (a.ncig + a.rect_i - 1) / a.rect_i;
    const int nrect = ((ncog + a.rect_c - 1) / a.rect_c) * rects_i;
    const int rect = unit % nrect;
    xsplit = unit / nrect;
    const int cg = (rect / rects_i) * a.rect_c + idx / a.rect_i, ci = (rect % rects_i) * a.rect_i + idx % a.rect_i;
    if (xsplit >= a.nx || cg >= ncog || ci >= a.ncig)
        return false;
    pair = cg * a.ncig + ci;
    return true;
}

// Wave-dealt form (a.wave_mode, k_wgrad3x3d WAVE): XCD x owns a contiguous run of pairs, its 128 waves take (pair, split) jobs in
// order -- wave_mode 2: pair fastest, 1: split fastest.  A wave without a job gets an empty run of pair 0 (wsplit = a.S).
__device__ __forceinline__ void wgrad_decode_wave(const WgradArgs &a, const unsigned bid, int wave, int &pair, int &xsplit, int &wsplit)
{
    const int xcd = bid & 7, base = a.npairs >> 3, rem = a.npairs & 7;
    const int mine = base + (xcd < rem ? 1 : 0), first = xcd * base + min(xcd, rem);
    const int job = (int)(bid >> 3) * 4 + wave;
    const int pl = a.wave_mode == 2 ? job % mine : job / a.S, sp = a.wave_mode == 2 ? job / mine : job - pl * a.S;
    xsplit = 0;
    if (a.wave_mode == 2 ? sp < a.S : pl < mine) {
        pair = first + pl;
        wsplit = sp;
    } else {                                // no job for this wave (it still meets the barrier of the scales)
        pair = 0;
        wsplit = a.S;
    }
}

// the last ci group is ragged when the tile count is not a multiple of NCI
template <int NCI>
__device__ __forceinline__ void wgrad_ci_ok(bool (&ci_ok)[NCI], int ci0, int Cin)
{
#pragma unroll
    for (int u = 0; u < NCI; ++u)
        ci_ok[u] = ci0 + 16 * u < Cin;
}

// PRE: the input operand is relu(x * pre_sc[ci] + pre_sh[ci]), the producer norm's map.  A lane converts values of ONE input
// channel per ci tile (row j of the tile): two registers per tile, one fma + one max per value in front of the split.
template <int NCI, bool PRE>
struct WgradPreMap {
    float psc[NCI], psh[NCI];
    __device__ __forceinline__ WgradPreMap(const float *pre_sc, const float *pre_sh, const bool (&ci_ok)[NCI], int ci0, int j)
    {
#pragma unroll
        for (int u = 0; u < NCI; ++u) {
            const int ch = ci_ok[u] ? ci0 + 16 * u + j : ci0 + j;
            psc[u] = PRE ? pre_sc[ch] : 1.f;
            psh[u] = PRE ? pre_sh[ch] : 0.f;
        }
    }
    __device__ __forceinline__ float operator()(float v, int u) const
    {
        return PRE ? fmaxf(__builtin_fmaf(v, psc[u], psh[u]), 0.f) : v;
    }
};

// slab `slab` of part, [tap][co][ci], scaled back by 1 / (sx sg); accumulator register q of lane (q4, j) is (co = 4 q4 + q, ci = j) of its tile
template <int NCO, int NCI, int NT>
__device__ __forceinline__ void wgrad_store_slab(const f32x4 (&acc)[NCO][NCI][NT], float *part, int slab, int Cout, int Cin, int co0,
                                                 int ci0, const bool (&ci_ok)[NCI], int q4, int j, float sx, float sg)
{
    const float inv = 1.0f / (sx * sg);
    float *out = part + (size_t)slab * NT * Cout * Cin;
#pragma unroll
    for (int t = 0; t < NCO; ++t)
#pragma unroll
        for (int u = 0; u < NCI; ++u)
#pragma unroll
            for (int k = 0; k < NT; ++k)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int co = co0 + 16 * t + 4 * q4 + q, ci = ci0 + 16 * u + j;
                    if (ci_ok[u])
                        out[((size_t)k * Cout + co) * Cin + ci] = acc[t][u][k][q] * inv;
                }
}

// The four waves of a workgroup hold partial sums of the SAME (co, ci) tiles: they are combined through LDS (red) in the fixed
// order (w0 + w1) + (w2 + w3).  True for wave 0, which then holds the sum; the other waves are done.
template <int NCO, int NCI, int NT>
__device__ __forceinline__ bool wgrad_combine(f32x4 (&acc)[NCO][NCI][NT], float (*red)[NCO * NCI * NT * 4][64], int wave, int lane)
{
    auto put = [&](int b) {
#pragma unroll
        for (int t = 0; t < NCO; ++t)
#pragma unroll
            for (int u = 0; u < NCI; ++u)
#pragma unroll
                for (int k = 0; k < NT; ++k)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        red[b][((t * NCI + u) * NT + k) * 4 + q][lane] = acc[t][u][k][q];
    };
    auto add = [&](int b) {
#pragma unroll
        for (int t = 0; t < NCO; ++t)
#pragma unroll
            for (int u = 0; u < NCI; ++u)
#pragma unroll
                for (int k = 0; k < NT; ++k)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        acc[t][u][k][q] += red[b][((t * NCI + u) * NT + k) * 4 + q][lane];
    };
    if (wave & 1)
        put(wave >> 1);
    __syncthreads();
    if (!(wave & 1))
        add(wave >> 1);
    __syncthreads();
    if (wave == 2)
        put(0);
    __syncthreads();
    if (wave != 0)
        return false;
    add(0);
    return true;
}

// one slab per workgroup: the combine, then wave 0 stores the sum
template <int NCO, int NCI, int NT>
__device__ __forceinline__ void wgrad_reduce_store(f32x4 (&acc)[NCO][NCI][NT], float (*red)[NCO * NCI * NT * 4][64], int wave, int lane,
                                                   float *part, int slab, int Cout, int Cin, int co0, int ci0,
                                                   const bool (&ci_ok)[NCI], int q4, int j, float sx, float sg)
{
    if (wgrad_combine(acc, red, wave, lane))
        wgrad_store_slab(acc, part, slab, Cout, Cin, co0, ci0, ci_ok, q4, j, sx, sg);
}

}  // namespace
