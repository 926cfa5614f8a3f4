// dcl_wgrad3x3.hip -- weight gradient of the 3x3 / stride 1 / pad 1 convolution on the f16 matrix pipe with
// fp32-equivalent arithmetic (f16x3: hi.hi + hi.lo + lo.hi of split-f16 operands, f32 accumulation).
//
//   dw[co, ci, ky, kx] = sum_{n, y, x} dy[n, co, y, x] * x[n, ci, y + ky - 1, x + kx - 1]
//
// GEMM view per tap: D[co][ci] += dY[co][pixel] * X_tap[pixel][ci], K = pixels.  In NCHW both operands have the K
// dimension (pixels of a row) contiguous, which is exactly what v_mfma_f32_16x16x32_f16 wants from a lane:
// lane (q, i) supplies 8 consecutive k for row / column i.  So there is NO LDS staging at all: every lane loads
// its 8 (+2 halo) f32 pixels straight from global memory (32-byte runs, 128-byte lines shared by the four
// k-octets of a wave), scales, splits into f16 (hi, lo) in registers and feeds the MFMA.  The three kx-shifted B
// fragments of an input row are three windows of the same 10 split values.
//
// One wave = NCO x NCI tiles of 16 x 16 (co x ci) x 9 taps of accumulators, walking down a 32-pixel-wide strip:
// per input row r it loads X[r] (B, 3 kx windows) and keeps dY rows r-1, r, r+1 (A) in registers -- row r pairs
// with dY row r + 1 - ky for tap row ky -- so each loaded fragment feeds 9 * NCO (B) or 9 * NCI (A) MFMAs x 3.
// The flat (image, strip, row) sequence is cut into S contiguous runs, one per wave; the four waves of a workgroup
// combine their partial dw through LDS in a fixed order and write one slab, k_wgrad_reduce sums the slabs in fixed
// order (deterministic, no float atomics).
#include <type_traits>

#include "dcl_common.h"
#include "dcl_wgrad.h"
#include "dcl_wgrad_plan.h"
#include "dcl_wgrad_reduce.h"

namespace {

// UPS: dy is the gradient of a STRIDE-2 convolution, i.e. the stride-1 formulation sees it zero-inserted at odd
// coordinates: row y of the virtual dy is row y / 2 of the stored one for even y (else zero), and an octet of 8
// virtual pixels is 4 stored values interleaved with zeros.
template <int NCO, int NCI, bool UPS>
__global__ __launch_bounds__(256, 1) void k_wgrad3x3(WgradArgs a)
{
    static_assert(NCO * NCI <= 4, "four tiles per wave at most (six spilled in the main loop)");
    __shared__ float wm[8];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q4 = lane >> 4, j = lane & 15;

    float sx, sg;
    wgrad_scales(a, wm, sx, sg);
    int pair, xsplit;
    if (a.rect_mode) {
        if (!wgrad_decode_rect(a, blockIdx.x, pair, xsplit))
            return;
    } else
        wgrad_decode_flat(a, blockIdx.x, pair, xsplit);
    const int split = xsplit * 4 + wave;           // a wave past the last split gets an empty run and adds zeros
    const int cog = pair / a.ncig, cig = pair - cog * a.ncig;
    const int co0 = cog * NCO * 16, ci0 = cig * NCI * 16;
    const size_t plane = (size_t)a.H * a.W;
    bool ci_ok[NCI];
    wgrad_ci_ok(ci_ok, ci0, a.Cin);

    f32x4 acc[NCO][NCI][9];
    DCL_WGRAD_CLEAR(acc, 9);

    // this split's share of the flat (image, strip, input row) sequence: rows [t0, t1), walked column by column
    const long long T = (long long)a.units * a.H;              // units = images x strips (columns)
    long long t = min(T, T * split / a.S);
    const long long t1 = min(T, T * (split + 1) / a.S);
    while (t < t1) {
        const int col = (int)(t / a.H);
        const int r0 = (int)(t - (long long)col * a.H);
        const int r1 = (int)min((long long)a.H, r0 + (t1 - t));
        t += r1 - r0;
        const int strip = col % a.strips;
        const int n = col / a.strips;
        const int px = strip * 32 + 8 * q4;
        // Loads are unconditional from clamped (always valid) addresses and masked through the operand scale
        // (0 instead of s) when they are converted one iteration later: a branch around a load would make the
        // compiler wait for it at the join, i.e. before the MFMAs it is supposed to overlap.
        const bool oct_ok = px < a.W;
        const int pxc = oct_ok ? px : a.W - 8;
        const int dl = (oct_ok && px > 0) ? -1 : 0, dr = px + 8 < a.W ? 8 : 7;     // halo offsets from the CLAMPED base
        const float sx_c = oct_ok ? sx : 0.f;                       // elements 1..8 of the B window
        const float sx_l = (oct_ok && px > 0) ? sx : 0.f;           // left halo (outside the image at x = -1)
        const float sx_r = (px + 8 < a.W) ? sx : 0.f;               // right halo
        const size_t dplane = (size_t)a.Hd * a.Wd;
        const float *ap = a.dy + ((size_t)n * a.Cout + co0 + j) * dplane + (UPS ? pxc / 2 : pxc);
        const float *bp = a.x + ((size_t)n * a.Cin + ci0 + j) * plane + pxc;     // + u * 16 * plane + r * W

        auto load_A = [&](int y, f32x4 (&dst)[NCO][2], float &scale) {
            if (UPS) {
                scale = (oct_ok && y >= 0 && !(y & 1) && (y >> 1) < a.Hd) ? sg : 0.f;
                const int yc = min(max(y >> 1, 0), a.Hd - 1);
#pragma unroll
                for (int t2 = 0; t2 < NCO; ++t2)
                    dst[t2][0] = *(const f32x4 *)(ap + (size_t)t2 * 16 * dplane + (size_t)yc * a.Wd);
            } else {
                scale = (oct_ok && y >= 0 && y < a.H) ? sg : 0.f;
                const int yc = min(max(y, 0), a.H - 1);
#pragma unroll
                for (int t2 = 0; t2 < NCO; ++t2) {
                    const float *p = ap + (size_t)t2 * 16 * dplane + (size_t)yc * a.W;
                    dst[t2][0] = *(const f32x4 *)p;
                    dst[t2][1] = *(const f32x4 *)(p + 4);
                }
            }
        };
        auto load_B = [&](int r, f32x4 (&dst)[NCI][2], float (&l)[NCI], float (&rr)[NCI]) {
            const int rc = min(r, a.H - 1);
#pragma unroll
            for (int u = 0; u < NCI; ++u) {
                const float *p = bp + (size_t)(ci_ok[u] ? u : 0) * 16 * plane + (size_t)rc * a.W;
                dst[u][0] = *(const f32x4 *)p;
                dst[u][1] = *(const f32x4 *)(p + 4);
                l[u] = p[dl];
                rr[u] = p[dr];
            }
        };
        auto cvt_A = [&](const f32x4 (&src)[NCO][2], float scale, half8 (&dst)[NCO][2]) {
#pragma unroll
            for (int t2 = 0; t2 < NCO; ++t2) {
                unsigned h[4], l[4];
                if (UPS) {
                    // (a0, 0, a1, 0, a2, 0, a3, 0): one split value in the low half of every pair
                    split1(src[t2][0].x, scale, h[0], l[0]);
                    split1(src[t2][0].y, scale, h[1], l[1]);
                    split1(src[t2][0].z, scale, h[2], l[2]);
                    split1(src[t2][0].w, scale, h[3], l[3]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        h[e] &= 0xffffu;
                        l[e] &= 0xffffu;
                    }
                    dst[t2][0] = as_half8(u32x4{h[0], h[1], h[2], h[3]});
                    dst[t2][1] = as_half8(u32x4{l[0], l[1], l[2], l[3]});
                    continue;
                }
                split2(src[t2][0].x, src[t2][0].y, scale, h[0], l[0]);
                split2(src[t2][0].z, src[t2][0].w, scale, h[1], l[1]);
                split2(src[t2][1].x, src[t2][1].y, scale, h[2], l[2]);
                split2(src[t2][1].z, src[t2][1].w, scale, h[3], l[3]);
                dst[t2][0] = as_half8(u32x4{h[0], h[1], h[2], h[3]});
                dst[t2][1] = as_half8(u32x4{l[0], l[1], l[2], l[3]});
            }
        };
        // the three kx windows of an input row are windows of the same 10 split values w[-1 .. 8]: kx = 0 and
        // kx = 2 share the pairing (w-1,w0)(w1,w2)...(w7,w8); kx = 1 is the 16-bit funnel shift of neighbours
        auto cvt_B = [&](const f32x4 (&src)[NCI][2], const float (&l)[NCI], const float (&rr)[NCI],
                         half8 (&dst)[3][NCI][2]) {
#pragma unroll
            for (int u = 0; u < NCI; ++u) {
                const float sc = ci_ok[u] ? sx_c : 0.f, sl = ci_ok[u] ? sx_l : 0.f, sr = ci_ok[u] ? sx_r : 0.f;
                unsigned h[5], q[5];
                // the halo values have their own scale (0 outside the image): split them alone, then merge
                unsigned hl, ql, hr, qr, hm, qm;
                split1(l[u], sl, hl, ql);                            // w-1
                split1(src[u][0].x, sc, hm, qm);                     // w0
                h[0] = __builtin_amdgcn_perm(hm, hl, 0x05040100u);   // (lo16(hl), lo16(hm))
                q[0] = __builtin_amdgcn_perm(qm, ql, 0x05040100u);
                split2(src[u][0].y, src[u][0].z, sc, h[1], q[1]);
                split2(src[u][0].w, src[u][1].x, sc, h[2], q[2]);
                split2(src[u][1].y, src[u][1].z, sc, h[3], q[3]);
                split1(src[u][1].w, sc, hm, qm);                     // w7
                split1(rr[u], sr, hr, qr);                           // w8
                h[4] = __builtin_amdgcn_perm(hr, hm, 0x05040100u);
                q[4] = __builtin_amdgcn_perm(qr, qm, 0x05040100u);
                u32x4 w0h = {h[0], h[1], h[2], h[3]}, w0l = {q[0], q[1], q[2], q[3]};
                u32x4 w2h = {h[1], h[2], h[3], h[4]}, w2l = {q[1], q[2], q[3], q[4]};
                unsigned a1h[4], a1l[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a1h[e] = __builtin_amdgcn_alignbit(h[e + 1], h[e], 16);
                    a1l[e] = __builtin_amdgcn_alignbit(q[e + 1], q[e], 16);
                }
                u32x4 w1h = {a1h[0], a1h[1], a1h[2], a1h[3]}, w1l = {a1l[0], a1l[1], a1l[2], a1l[3]};
                dst[0][u][0] = as_half8(w0h);
                dst[0][u][1] = as_half8(w0l);
                dst[1][u][0] = as_half8(w1h);
                dst[1][u][1] = as_half8(w1l);
                dst[2][u][0] = as_half8(w2h);
                dst[2][u][1] = as_half8(w2l);
            }
        };

        // Software pipeline, unrolled by six so that every register array is indexed statically and nothing is
        // copied between iterations.  dY rows live in a ring of three slots (row y in slot (y - r0 + 1) % 3), X rows
        // in two sets.  Step i (input row r = r0 + i):
        //   1. MFMAs of tap row ky = 2 (dY row r - 1, the oldest slot),
        //   2. the raw values loaded one step ago are split into f16 pairs: dY row r + 2 into that slot, X row
        //      r + 1 into the other B set -- VALU work that overlaps the remaining MFMAs,
        //   3. the loads of dY row r + 3 / X row r + 2 are issued into the raw registers just consumed,
        //   4. MFMAs of tap rows ky = 1, 0 (dY rows r, r + 1).
        half8 A[3][NCO][2], B[2][3][NCI][2];
        f32x4 rawA[NCO][2], rawB[NCI][2];
        float rawL[NCI], rawR[NCI], rawS;
        {
            f32x4 p0[NCO][2], p1[NCO][2], p2[NCO][2], q0[NCI][2];
            float s0, s1, s2, l0[NCI], rr0[NCI];
            load_A(r0 - 1, p0, s0);
            load_A(r0, p1, s1);
            load_A(r0 + 1, p2, s2);
            load_B(r0, q0, l0, rr0);
            load_A(r0 + 2, rawA, rawS);
            load_B(r0 + 1, rawB, rawL, rawR);
            cvt_A(p0, s0, A[0]);
            cvt_A(p1, s1, A[1]);
            cvt_A(p2, s2, A[2]);
            cvt_B(q0, l0, rr0, B[0]);
        }
        auto mfma_row = [&](auto SLOT, auto BSET, auto KY) {
            constexpr int slot = decltype(SLOT)::value, bs = decltype(BSET)::value, ky = decltype(KY)::value;
            // pass-major: all tiles hi.hi, then all hi.lo, then all lo.hi -- the three MFMAs of one accumulator are
            // 9 NCI instructions apart and each accumulates in place (dst == srcC)
#pragma unroll
            for (int pass = 0; pass < 3; ++pass)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                    for (int t2 = 0; t2 < NCO; ++t2)
#pragma unroll
                        for (int u = 0; u < NCI; ++u)
                            acc[t2][u][ky * 3 + kx] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                                A[slot][t2][pass == 2 ? 1 : 0], B[bs][kx][u][pass == 1 ? 1 : 0],
                                acc[t2][u][ky * 3 + kx], 0, 0, 0);
        };
        auto step = [&](auto PH, int r) {
            constexpr int ph = decltype(PH)::value;
            using I = std::integral_constant<int, ph % 3>;             // slot of dY row r - 1
            using I1 = std::integral_constant<int, (ph + 1) % 3>;      // row r
            using I2 = std::integral_constant<int, (ph + 2) % 3>;      // row r + 1
            using BS = std::integral_constant<int, ph % 2>;
            mfma_row(I{}, BS{}, std::integral_constant<int, 2>{});
            cvt_A(rawA, rawS, A[ph % 3]);
            cvt_B(rawB, rawL, rawR, B[(ph + 1) % 2]);
            // the loads stay between the two MFMA groups (left alone the scheduler sinks them to their use, one
            // step later, and the wave eats the memory latency every row)
            __builtin_amdgcn_sched_barrier(0);
            load_A(r + 3, rawA, rawS);
            load_B(r + 2, rawB, rawL, rawR);
            __builtin_amdgcn_sched_barrier(0);
            mfma_row(I1{}, BS{}, std::integral_constant<int, 1>{});
            mfma_row(I2{}, BS{}, std::integral_constant<int, 0>{});
        };
        int r = r0;
        for (; r + 6 <= r1; r += 6) {
            step(std::integral_constant<int, 0>{}, r);
            step(std::integral_constant<int, 1>{}, r + 1);
            step(std::integral_constant<int, 2>{}, r + 2);
            step(std::integral_constant<int, 3>{}, r + 3);
            step(std::integral_constant<int, 4>{}, r + 4);
            step(std::integral_constant<int, 5>{}, r + 5);
        }
        if (r < r1)
            step(std::integral_constant<int, 0>{}, r);
        if (r + 1 < r1)
            step(std::integral_constant<int, 1>{}, r + 1);
        if (r + 2 < r1)
            step(std::integral_constant<int, 2>{}, r + 2);
        if (r + 3 < r1)
            step(std::integral_constant<int, 3>{}, r + 3);
        if (r + 4 < r1)
            step(std::integral_constant<int, 4>{}, r + 4);
    }

    // one slab per workgroup: [xsplit][tap][co][ci]
    __shared__ float red[2][NCO * NCI * 36][64];
    wgrad_reduce_store(acc, red, wave, lane, a.part, xsplit, a.Cout, a.Cin, co0, ci0, ci_ok, q4, j, sx, sg);
}

}  // namespace

static WgradTune g_tune;                        // tuning overrides (dcl_wgrad3x3_set_*): tile, splits, variant, wave form, strip groups
static int g_wg_target = 256;                   // workgroups a launch aims at (pixel splits = target / tile pairs): one per CU;
                                                // tuning hook dcl_wgrad3x3_set_workgroup_target for in-step A/B runs, where the
                                                // launch shares the chip with the other branches' kernels
static int g_s2_native = 1;     // stride 2: 1 = output-pixel formulation (dcl_wgrad3x3_s2.hip), 0 = zero-inserted dy

// The one launch plan: every decision between the shape and the launch is taken here, once (stride 1: dcl_wgrad_plan.h).
static WgradPlan wgrad_plan(int N, int Cin, int Cout, int H, int W, int stride)
{
    if (stride == 2 && g_s2_native && dcl_wgrad_s2_supported(H, W)) {
        WgradPlan p = {};
        dcl_wgrad_s2_plan(N, Cin, Cout, H, W, g_tune.tile_nco, g_tune.tile_nci, p);
        return p;
    }
    return wgrad_plan_stride1(N, Cin, Cout, H, W, stride, g_tune, g_wg_target, 128);
}

extern "C" int dcl_wgrad3x3_set_tile(int nco, int nci)
{
    // only tiles with an instantiated kernel (the six-tile wave (3, 2) spilled: retired)
    if (nco < 0 || nco > 3 || nci < 0 || nci > 2 || (nco == 3 && nci == 2))
        return DCL_EINVAL;
    g_tune.tile_nco = nco;
    g_tune.tile_nci = nci;
    return 0;
}

extern "C" int dcl_wgrad3x3_set_variant(int variant)
{
    if (variant < -1 || variant > 2 || variant == 1)     // 1 was the retired kernel
        return DCL_EINVAL;
    g_tune.variant = variant;
    dcl_wgrad_s2_set_dma(variant != 0);      // the stride-2 kernel's LDS-DMA form follows the same switch
    return 0;
}

extern "C" int dcl_wgrad3x3_set_workgroup_target(int n)
{
    g_wg_target = n >= 32 ? n : 256;
    return 0;
}

extern "C" int dcl_wgrad3x3_set_splits(int nx)
{
    g_tune.force_nx = nx > 0 ? nx : 0;
    return 0;
}

extern "C" int dcl_wgrad3x3_set_wave_mode(int on)
{
    g_tune.wave_mode = on < 0 ? 0 : on;
    return 0;
}

extern "C" int dcl_wgrad3x3_set_wave_band(int rows)
{
    g_tune.wave_band = rows > 0 ? rows : 0;
    return 0;
}

extern "C" int dcl_wgrad3x3_set_strip_group(int on)
{
    g_tune.strip_group = on ? 1 : 0;
    return 0;
}

extern "C" int dcl_wgrad3x3_set_stride2(int native)
{
    if (native < 0 || native > 2)
        return DCL_EINVAL;
    g_s2_native = native ? 1 : 0;
    dcl_wgrad_s2_set_dma(native != 2);       // 2: the round-4 kernel (every operand loaded in MFMA order)
    return 0;
}

extern "C" int dcl_wgrad3x3_splits(int N, int Cin, int Cout, int H, int W, int stride)
{
    if (N <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || (Cin & 15) || (Cout & 15) || stride < 1 || stride > 2)
        return 0;
    return wgrad_plan(N, Cin, Cout, H, W, stride).slabs;
}

static int wgrad3x3_impl(const float *x, const float *dy, int N, int Cin, int Cout, int H, int W, const float *xamax, int xcount,
                         const float *gamax, int gcount, int stride, float *part, float *dw, void *stream, const float *pre_sc,
                         const float *pre_sh);

extern "C" int dcl_wgrad3x3_f16x3(const float *x, const float *dy, int N, int Cin, int Cout, int H, int W,
                                  const float *xamax, int xcount, const float *gamax, int gcount, int stride,
                                  float *part, float *dw, void *stream)
{
    return wgrad3x3_impl(x, dy, N, Cin, Cout, H, W, xamax, xcount, gamax, gcount, stride, part, dw, stream, nullptr, nullptr);
}

// 1 when dcl_wgrad3x3_pre_f16x3 serves the shape: stride 1 on the LDS-DMA kernel, stride 2 on the output-pixel formulation
// (the slab count is dcl_wgrad3x3_splits(..., stride))
extern "C" int dcl_wgrad3x3_pre_supported(int N, int Cin, int Cout, int H, int W, int stride)
{
    if (N <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || (Cin & 15) || (Cout & 15) || (W & 7))
        return 0;
    if (stride != 1 && stride != 2)
        return 0;
    return wgrad_plan(N, Cin, Cout, H, W, stride).family != WGRAD_DIRECT ? 1 : 0;
}

// The weight gradient of conv2d(relu(x * pre_sc[ci] + pre_sh[ci]), w, padding = 1) for the output gradient dy: x is the RAW
// tensor in front of the norm, xamax the absmax slots of the mapped tensor (dcl_bn_finalize_pre); see k_wgrad3x3d, PRE.
extern "C" int dcl_wgrad3x3_pre_f16x3(const float *x, const float *dy, int N, int Cin, int Cout, int H, int W,
                                      const float *xamax, int xcount, const float *gamax, int gcount, const float *pre_sc,
                                      const float *pre_sh, int stride, float *part, float *dw, void *stream)
{
    DCL_CHECK_ARG(pre_sc && pre_sh, "null pointer");
    if (!dcl_wgrad3x3_pre_supported(N, Cin, Cout, H, W, stride)) {
        dcl_set_error("dcl_wgrad3x3_pre_f16x3: no kernel with the map for this shape / stride");
        return DCL_EUNSUPPORTED;
    }
    return wgrad3x3_impl(x, dy, N, Cin, Cout, H, W, xamax, xcount, gamax, gcount, stride, part, dw, stream, pre_sc, pre_sh);
}

static int wgrad3x3_impl(const float *x, const float *dy, int N, int Cin, int Cout, int H, int W, const float *xamax, int xcount,
                         const float *gamax, int gcount, int stride, float *part, float *dw, void *stream, const float *pre_sc,
                         const float *pre_sh)
{
    DCL_CHECK_ARG(stride == 1 || stride == 2, "stride must be 1 or 2");
    DCL_CHECK_ARG(x && dy && xamax && gamax && part && dw, "null pointer");
    DCL_CHECK_ARG(N > 0 && H > 0 && W > 0 && xcount > 0 && gcount > 0, "bad shape");
    DCL_CHECK_ARG(Cin > 0 && Cout > 0 && (Cin & 15) == 0 && (Cout & 15) == 0, "channel counts must be multiples of 16");
    DCL_CHECK_ARG((W & 7) == 0, "W must be a multiple of 8");
    DCL_CHECK_ARG(((((uintptr_t)x) | ((uintptr_t)dy)) & 15) == 0, "tensors must be 16-byte aligned");
    const WgradPlan p = wgrad_plan(N, Cin, Cout, H, W, stride);
    WgradArgs a;
    wgrad_fill_args(a, p, x, dy, part, xamax, xcount, gamax, gcount, N, Cin, Cout, H, W, stride, pre_sc, pre_sh);
    const dim3 grid(p.grid);
    hipStream_t s = (hipStream_t)stream;
    if (p.family == WGRAD_S2 || p.family == WGRAD_S2_DMA) {
        if (const int rc = dcl_wgrad_s2_launch(a, p, s))
            return rc;
    } else if (p.family == WGRAD_DMA) {
        if (const int rc = dcl_wgrad_dma_launch(a, p.nco, p.nci, grid, s))
            return rc;
    } else {
#define DCL_WG_CASE(o, i)                                                        \
    if (p.nco == o && p.nci == i) {                                              \
        if (stride == 2)                                                         \
            hipLaunchKernelGGL((k_wgrad3x3<o, i, true>), grid, dim3(256), 0, s, a);  \
        else                                                                     \
            hipLaunchKernelGGL((k_wgrad3x3<o, i, false>), grid, dim3(256), 0, s, a); \
    } else
        DCL_WG_CASE(2, 2)
        DCL_WG_CASE(1, 2)
        DCL_WG_CASE(3, 1)
        DCL_WG_CASE(2, 1)
        DCL_WG_CASE(1, 1)
        DCL_WGRAD_NO_KERNEL("k_wgrad3x3", p.nco, p.nci);
#undef DCL_WG_CASE
        dcl_note_kernel("k_wgrad3x3<%d,%d,%s>", p.nco, p.nci, stride == 2 ? "true" : "false");
    }
    DCL_LAUNCH_CHECK();
    launch_wgrad_reduce(part, p.slabs, Cout, Cin, dw, s);
    DCL_LAUNCH_CHECK();
    return 0;
}
