// dcl_wgrad3x3d_body.h -- the workgroup body of the stride-1 weight gradient with LDS-DMA operand staging (wgrad3x3d_body), for
// the translation units that instantiate it: dcl_wgrad3x3d.hip (k_wgrad3x3d, the kernel of dcl_wgrad3x3_f16x3) and dcl_convbwd.hip
// (k_conv3x3_bwd: the same workgroups behind the data-gradient tiles of one launch).  The caller owns the LDS -- `smem`,
// wgrad3x3d_lds_bytes() bytes aligned to 1024, and `wm`, 8 floats -- and hands in the workgroup id.  Design notes: head of
// dcl_wgrad3x3d.hip.
#pragma once
#include <type_traits>

#include "dcl_common.h"
#include "dcl_wgrad.h"

// Bound probes (DCL_WG_PROBE, dcl_f16x3.h): bit 1 = no MFMAs
#define DCL_WMFMA(A, B, C) ((DCL_WG_PROBE & 1) ? (C) : __builtin_amdgcn_mfma_f32_16x16x32_f16((A), (B), (C), 0, 0, 0))

namespace {

constexpr int APIECES = 9, BPIECES = 11;          // 16-byte pieces per staged row: 8 (+ 2 halo) + 1 pad
#ifndef DCL_WG_SPREAD
#define DCL_WG_SPREAD 1
#endif
constexpr bool g_wgrad_spread = DCL_WG_SPREAD != 0;      // LDS-DMA instructions dealt out among the MFMAs (see step())

// LDS of one workgroup: the four waves' staging rings (three slots of NI KiB each), reused for the combine of the four waves
template <int NCO, int NCI, bool WAVE>
constexpr int wgrad3x3d_lds_bytes()
{
    constexpr int NIA = (NCO * 16 * APIECES + 63) / 64, NIB = (NCI * 16 * BPIECES + 63) / 64, NI = NIA + NIB;
    constexpr int STAGEB = 4 * 3 * NI * 1024;
    constexpr int REDB = WAVE ? 0 : 2 * NCO * NCI * 36 * 64 * 4;
    return STAGEB > REDB ? STAGEB : REDB;
}

// WAVE = true (a.wave_mode): between 129 and 256 tile pairs a workgroup per pair leaves CUs empty (the head's 144 -> 720
// launch: 135 pairs on 256 CUs) and a second workgroup per pair would run as a second round.  Here the S = 128 / ceil(pairs / 8)
// pixel splits of a pair go to single WAVES: XCD x owns a contiguous run of pairs (~pairs / 8 of them: neighbours share their dY
// channel rows in that XCD's L2), its 128 waves (32 workgroups of the 256-workgroup grid) take (pair, split) jobs in order --
// wave_mode 2: pair fastest, so the four waves of a workgroup walk the same pixels for four neighbouring pairs (shared dY rows
// hit in the CU's L1: 1.89 ms against 1.99 with split fastest, 2.83 with a workgroup per pair on 12 x (144 -> 720) x 128 x 256) --
// and a wave writes its own slab (no LDS reduction: the four waves of a workgroup belong to different pairs).
//
// PRE: x is the RAW output z of the convolution in front of a training-mode norm and the operand is relu(z sc[ci] + sh[ci]) --
// the weight gradient of the BasicBlock's conv2 (reference models/HRNet.py:77-93) without the normalised tensor in memory
// (dcl_conv3x3_pre.hip has the forward).  A lane converts values of ONE input channel per ci tile (row j of the tile), so the
// map costs two registers per tile and one fma + one max per value in front of the split; the halo values and the pixels past
// the row end are masked through the operand scale, i.e. after the map.
template <int NCO, int NCI, bool WAVE, bool PRE>
__device__ __forceinline__ void wgrad3x3d_body(const WgradArgs &a, const unsigned bid, unsigned char *smem, float *wm)
{
    constexpr int NIA = (NCO * 16 * APIECES + 63) / 64, NIB = (NCI * 16 * BPIECES + 63) / 64, NI = NIA + NIB;
    constexpr int NS = 3;                                   // ring slots: rows are fetched two steps ahead
    constexpr int SLOTB = NI * 1024, STAGEB = 4 * NS * SLOTB;
    static_assert(NCO * NCI <= 4, "four tiles per wave at most (six spilled in the main loop)");
    constexpr int NREG = NCO * NCI * 36;
    constexpr int SMEMB = wgrad3x3d_lds_bytes<NCO, NCI, WAVE>();
    static_assert(SMEMB >= STAGEB && SMEMB + 64 <= 160 * 1024, "LDS");
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q4 = lane >> 4, j = lane & 15;

    // operand scales from the producers' partial maxima -- computed AFTER the first rows are in flight (a wave with an
    // empty run does it right away: every wave passes the barrier inside exactly once)
    float sx = 0.f, sg = 0.f;
    bool have_scales = false;
    auto scales = [&]() {
        wgrad_scales(a, wm, sx, sg);
        have_scales = true;
    };
    // workgroup -> (tile pair, pixel split): as k_wgrad3x3
    int pair, xsplit, wsplit = 0;
    if (WAVE)
        wgrad_decode_wave(a, bid, wave, pair, xsplit, wsplit);
    else if (a.rect_mode) {
        if (!wgrad_decode_rect(a, bid, pair, xsplit))
            return;
    } else
        wgrad_decode_flat(a, bid, pair, xsplit);
    const int split = WAVE ? wsplit : xsplit * 4 + wave;
    const int cog = pair / a.ncig, cig = pair - cog * a.ncig;
    const int co0 = cog * NCO * 16, ci0 = cig * NCI * 16;
    const size_t plane = (size_t)a.H * a.W;
    bool ci_ok[NCI];
    wgrad_ci_ok(ci_ok, ci0, a.Cin);
    const WgradPreMap<NCI, PRE> pre(a.pre_sc, a.pre_sh, ci_ok, ci0, j);

    // staging geometry of this lane, per DMA instruction m: which (tile, row, piece) of the slot image it carries
    // (piece = 64 m + lane in [tile][row][piece] order; the tail of the last instruction repeats piece 0)
    unsigned chanA[NIA], chanB[NIB];        // byte offset of the lane's channel row from the image's channel 0
    int pieceA[NIA], pieceB[NIB];           // first pixel of its piece relative to the strip (A: 0 .. 28, B: -4 .. 32)
#pragma unroll
    for (int m = 0; m < NIA; ++m) {
        int P = 64 * m + lane;
        if (P >= NCO * 16 * APIECES)
            P = 0;
        const int row = P / APIECES, pc = min(P - row * APIECES, APIECES - 2);     // (tile, row) flat; pad -> last piece
        chanA[m] = (unsigned)((size_t)(co0 + row) * plane * 4);
        pieceA[m] = 4 * pc;
    }
#pragma unroll
    for (int m = 0; m < NIB; ++m) {
        int P = 64 * m + lane;
        if (P >= NCI * 16 * BPIECES)
            P = 0;
        const int row = P / BPIECES, pc = min(P - row * BPIECES, BPIECES - 2);
        const int u = row >> 4;
        const int ch = (ci0 + 16 * u < a.Cin) ? ci0 + row : ci0 + (row & 15);       // ragged last ci group: tile 0 again
        chanB[m] = (unsigned)((size_t)ch * plane * 4);
        pieceB[m] = 4 * pc - 4;
    }
    const unsigned lds0 = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) unsigned char *)smem +
                          (unsigned)wave * (NS * SLOTB);
    const unsigned char *my = smem + wave * (NS * SLOTB);
    // MFMA-order read offsets inside a slot: lane (q4, j) reads pixels 8 q4 .. 8 q4 + 7 of row j
    const unsigned ardo = (unsigned)(j * APIECES + 2 * q4) * 16;
    const unsigned brdo = (unsigned)(NIA * 1024 + (j * BPIECES + 1 + 2 * q4) * 16);

    f32x4 acc[NCO][NCI][9];
    DCL_WGRAD_CLEAR(acc, 9);

    // Which rows: split `split` of S over the columns (image, strip) x H rows -- or, a.grp = G > 1 (workgroup form only), the G
    // waves w % G of a workgroup take G ADJACENT strips over the SAME rows (sub-range w / G of the workgroup's share of the
    // "super-columns" (image, G strips)).  An x row piece with its halo touches three 128-byte lines, two of them the neighbouring
    // strips' own: with the neighbours in the same CU at the same time they are L1 / L2 hits instead of a second and third fetch
    // through the fabric (FETCH_SIZE of the 64 -> 64 launch was 2.05x the tensors: 1 + 3 lines per dY + x row against 1 + 1).
    const int G = WAVE ? 1 : a.grp;
    const long long T = (long long)(a.units / G) * a.H;
    const int q = G > 1 ? xsplit * (4 / G) + wave / G : split, Sq = G > 1 ? a.nx * (4 / G) : a.S;
    long long t = min(T, T * q / Sq);
    const long long t1 = min(T, T * (q + 1) / Sq);
    if (t >= t1)
        scales();
    // a.band < H (wave form): a column is `band` rows of a strip and the strips of an image follow each other band by band, so
    // that the halo lines of an x row -- the neighbouring strips' own lines -- are touched again `band` row steps later, while
    // the XCD's L2 still has them, not H row steps later
    const int RB = a.band, nb = a.H / RB;
    while (t < t1) {
        const int colb = (int)(t / RB);                         // (image, band, strip) or, one band, (image, strip)
        const int rr0 = (int)(t - (long long)colb * RB);
        const int len = (int)min((long long)(RB - rr0), t1 - t);
        t += len;
        const int sgs = a.strips / G;
        const int strip = (colb % sgs) * G + (G > 1 ? wave % G : 0);
        const int band = (colb / sgs) % nb;
        const int n = colb / (sgs * nb);
        const int r0 = band * RB + rr0, r1 = r0 + len;
        const int px0 = strip * 32, px = px0 + 8 * q4;
        const bool oct_ok = px < a.W;
        float sx_c, sx_l, sx_r;                                 // set once the scales are known (below)
        // per-lane source offsets of this column (pieces clamped into the row: what falls outside is masked by the scales)
        unsigned offA[NIA], offB[NIB];
#pragma unroll
        for (int m = 0; m < NIA; ++m)
            offA[m] = chanA[m] + 4u * (unsigned)min(max(px0 + pieceA[m], 0), a.W - 4);
#pragma unroll
        for (int m = 0; m < NIB; ++m)
            offB[m] = chanB[m] + 4u * (unsigned)min(max(px0 + pieceB[m], 0), a.W - 4);
        const float *dyn = a.dy + (size_t)n * a.Cout * plane, *xn = a.x + (size_t)n * a.Cin * plane;

        // group g = (dY row g + 1, X row g) -> ring slot s
        auto dma_group = [&](int g, int s) {
            const float *ab = uniform_ptr(dyn + (size_t)min(max(g + 1, 0), a.H - 1) * a.W);
            const float *bb = uniform_ptr(xn + (size_t)min(max(g, 0), a.H - 1) * a.W);
            const unsigned dst = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)s * SLOTB);
#pragma unroll
            for (int m = 0; m < NIA; ++m)
                dma16(ab, offA[m], dst + m * 1024);
#pragma unroll
            for (int m = 0; m < NIB; ++m)
                dma16(bb, offB[m], dst + (NIA + m) * 1024);
        };
        auto read_A = [&](int s, f32x4 (&dst)[NCO][2]) {
            const unsigned char *p = my + s * SLOTB + ardo;
#pragma unroll
            for (int t2 = 0; t2 < NCO; ++t2) {
                dst[t2][0] = *(const f32x4 *)(p + t2 * (16 * APIECES * 16));
                dst[t2][1] = *(const f32x4 *)(p + t2 * (16 * APIECES * 16) + 16);
            }
        };
        auto read_B = [&](int s, f32x4 (&dst)[NCI][2], float (&l)[NCI], float (&rr)[NCI]) {
            const unsigned char *p = my + s * SLOTB + brdo;
#pragma unroll
            for (int u = 0; u < NCI; ++u) {
                const unsigned char *pu = p + u * (16 * BPIECES * 16);
                dst[u][0] = *(const f32x4 *)pu;
                dst[u][1] = *(const f32x4 *)(pu + 16);
                l[u] = *(const float *)(pu - 4);
                rr[u] = *(const float *)(pu + 32);
            }
        };
        auto cvt_A = [&](int y, const f32x4 (&src)[NCO][2], half8 (&dst)[NCO][2]) {
            const float scale = (oct_ok && y >= 0 && y < a.H) ? sg : 0.f;
#pragma unroll
            for (int t2 = 0; t2 < NCO; ++t2) {
                unsigned h[4], l[4];
                split2(src[t2][0].x, src[t2][0].y, scale, h[0], l[0]);
                split2(src[t2][0].z, src[t2][0].w, scale, h[1], l[1]);
                split2(src[t2][1].x, src[t2][1].y, scale, h[2], l[2]);
                split2(src[t2][1].z, src[t2][1].w, scale, h[3], l[3]);
                dst[t2][0] = as_half8(u32x4{h[0], h[1], h[2], h[3]});
                dst[t2][1] = as_half8(u32x4{l[0], l[1], l[2], l[3]});
            }
        };
        auto cvt_B = [&](const f32x4 (&src)[NCI][2], const float (&l)[NCI], const float (&rr)[NCI],
                         half8 (&dst)[3][NCI][2]) {
#pragma unroll
            for (int u = 0; u < NCI; ++u) {
                const float sc = ci_ok[u] ? sx_c : 0.f, sl = ci_ok[u] ? sx_l : 0.f, sr = ci_ok[u] ? sx_r : 0.f;
                unsigned h[5], q[5];
                unsigned hl, ql, hr, qr, hm, qm;
                split1(pre(l[u], u), sl, hl, ql);
                split1(pre(src[u][0].x, u), sc, hm, qm);
                h[0] = __builtin_amdgcn_perm(hm, hl, 0x05040100u);
                q[0] = __builtin_amdgcn_perm(qm, ql, 0x05040100u);
                split2(pre(src[u][0].y, u), pre(src[u][0].z, u), sc, h[1], q[1]);
                split2(pre(src[u][0].w, u), pre(src[u][1].x, u), sc, h[2], q[2]);
                split2(pre(src[u][1].y, u), pre(src[u][1].z, u), sc, h[3], q[3]);
                split1(pre(src[u][1].w, u), sc, hm, qm);
                split1(pre(rr[u], u), sr, hr, qr);
                h[4] = __builtin_amdgcn_perm(hr, hm, 0x05040100u);
                q[4] = __builtin_amdgcn_perm(qr, qm, 0x05040100u);
                unsigned a1h[4], a1l[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a1h[e] = __builtin_amdgcn_alignbit(h[e + 1], h[e], 16);
                    a1l[e] = __builtin_amdgcn_alignbit(q[e + 1], q[e], 16);
                }
                dst[0][u][0] = as_half8(u32x4{h[0], h[1], h[2], h[3]});
                dst[0][u][1] = as_half8(u32x4{q[0], q[1], q[2], q[3]});
                dst[1][u][0] = as_half8(u32x4{a1h[0], a1h[1], a1h[2], a1h[3]});
                dst[1][u][1] = as_half8(u32x4{a1l[0], a1l[1], a1l[2], a1l[3]});
                dst[2][u][0] = as_half8(u32x4{h[1], h[2], h[3], h[4]});
                dst[2][u][1] = as_half8(u32x4{q[1], q[2], q[3], q[4]});
            }
        };

        // Column start: groups r0 - 2 (dY row r0 - 1 only), r0 - 1, r0 fill the ring and are converted; then groups
        // r0 + 1, r0 + 2 are put in flight.  Steady state, step i (X row r = r0 + i, ph = i % 6):
        //   wait until group r + 1 (issued two steps ago) has landed; read it out of slot (i + 1) % 3,
        //   MFMAs of tap row ky = 2 (dY row r - 1); underneath, dY row r + 2 / X row r + 1 are split into fragments,
        //   group r + 3 is issued into slot i % 3 (group r's, read one step ago),
        //   MFMAs of tap rows ky = 1, 0.
        half8 A[3][NCO][2], B[2][3][NCI][2];
        vm_wait<0>();                          // nothing of the previous column is still landing in the ring
        dma_group(r0 - 2, 0);
        dma_group(r0 - 1, 1);
        dma_group(r0, 2);
        if (!have_scales)
            scales();
        sx_c = oct_ok ? sx : 0.f;
        sx_l = (oct_ok && px > 0) ? sx : 0.f;
        sx_r = (px + 8 < a.W) ? sx : 0.f;
        vm_wait<0>();
        {
            f32x4 ra[NCO][2], rb[NCI][2];
            float rl[NCI], rr[NCI];
            read_A(0, ra);
            cvt_A(r0 - 1, ra, A[0]);
            read_A(1, ra);
            cvt_A(r0, ra, A[1]);
            read_A(2, ra);
            read_B(2, rb, rl, rr);
            cvt_A(r0 + 1, ra, A[2]);
            cvt_B(rb, rl, rr, B[0]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the ring has been read: its slots may be refilled
        dma_group(r0 + 1, 1);
        dma_group(r0 + 2, 2);

        auto mfma_row = [&](auto SLOT, auto BSET, auto KY) {
            constexpr int slot = decltype(SLOT)::value, bs = decltype(BSET)::value, ky = decltype(KY)::value;
#pragma unroll
            for (int pass = 0; pass < 3; ++pass)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                    for (int t2 = 0; t2 < NCO; ++t2)
#pragma unroll
                        for (int u = 0; u < NCI; ++u)
                            acc[t2][u][ky * 3 + kx] = DCL_WMFMA(A[slot][t2][pass == 2 ? 1 : 0], B[bs][kx][u][pass == 1 ? 1 : 0],
                                acc[t2][u][ky * 3 + kx]);
        };
        auto step = [&](auto PH, int r) {
            constexpr int ph = decltype(PH)::value;
            using I = std::integral_constant<int, ph % 3>;             // register slot of dY row r - 1
            using I1 = std::integral_constant<int, (ph + 1) % 3>;
            using I2 = std::integral_constant<int, (ph + 2) % 3>;
            using BS = std::integral_constant<int, ph % 2>;
            f32x4 ra[NCO][2], rb[NCI][2];
            float rl[NCI], rr[NCI];
            vm_wait<NI>();                                            // group r + 1 is in LDS (group r + 2 may be landing)
            read_A((ph + 1) % 3, ra);
            read_B((ph + 1) % 3, rb, rl, rr);
            mfma_row(I{}, BS{}, std::integral_constant<int, 2>{});
            cvt_A(r + 2, ra, A[ph % 3]);
            cvt_B(rb, rl, rr, B[(ph + 1) % 2]);
            // Group r + 3 goes into slot ph % 3 (group r's, read one step ago).  Its NI LDS-DMA instructions are dealt out
            // one per (pass, kx) sub-block of the remaining two tap rows (18 sub-blocks of NCO x NCI MFMAs), each fenced
            // so that it stays there: as ONE block between the tap rows (~5 NI scalar + vector-memory instructions) they were
            // issued with the matrix pipe idle -- probe builds: time(no DMA) = 0.80 x time(product) on the BasicBlock shapes.
            __builtin_amdgcn_sched_barrier(0);
            if (!g_wgrad_spread) {
                dma_group(r + 3, ph % 3);
                __builtin_amdgcn_sched_barrier(0);
                mfma_row(I1{}, BS{}, std::integral_constant<int, 1>{});
                mfma_row(I2{}, BS{}, std::integral_constant<int, 0>{});
            } else {
                const int g3 = r + 3;
                const float *ab = uniform_ptr(dyn + (size_t)min(max(g3 + 1, 0), a.H - 1) * a.W);
                const float *bb = uniform_ptr(xn + (size_t)min(max(g3, 0), a.H - 1) * a.W);
                const unsigned dst = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(ph % 3) * SLOTB);
                static_assert(NI <= 18, "one DMA instruction per sub-block");
#pragma unroll
                for (int sb = 0; sb < 18; ++sb) {
                    const int kyi = sb / 9, pass = (sb % 9) / 3, kx = sb % 3;      // tap row ky = 1, then ky = 0
#pragma unroll
                    for (int t2 = 0; t2 < NCO; ++t2)
#pragma unroll
                        for (int u = 0; u < NCI; ++u) {
                            if (kyi == 0)
                                acc[t2][u][3 + kx] = DCL_WMFMA(A[(ph + 1) % 3][t2][pass == 2 ? 1 : 0],
                                                               B[ph % 2][kx][u][pass == 1 ? 1 : 0], acc[t2][u][3 + kx]);
                            else
                                acc[t2][u][kx] = DCL_WMFMA(A[(ph + 2) % 3][t2][pass == 2 ? 1 : 0],
                                                           B[ph % 2][kx][u][pass == 1 ? 1 : 0], acc[t2][u][kx]);
                        }
                    if (sb < NIA)
                        dma16(ab, offA[sb], dst + sb * 1024);
                    else if (sb < NI)
                        dma16(bb, offB[sb - NIA], dst + sb * 1024);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
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
    vm_wait<0>();

    if (WAVE) {                                 // one slab per wave: the four waves of a workgroup belong to different pairs
        if (split < a.S)
            wgrad_store_slab(acc, a.part, split, a.Cout, a.Cin, co0, ci0, ci_ok, q4, j, sx, sg);
        return;
    }
    __syncthreads();                            // every wave is done with its staging ring: reuse it for the reduction
    wgrad_reduce_store(acc, (float(*)[NREG][64])smem, wave, lane, a.part, xsplit, a.Cout, a.Cin, co0, ci0, ci_ok, q4, j, sx, sg);
}

}  // namespace
