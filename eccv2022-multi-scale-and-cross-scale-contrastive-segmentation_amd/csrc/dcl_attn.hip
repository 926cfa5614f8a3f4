// dcl_attn.hip -- global multi-head self-attention, forward and backward, on the f16 matrix cores at fp32-equivalent accuracy
// (split-f16: hi.hi + hi.lo + lo.hi, f32 accumulation) and without an N x N tensor (include/dcl_attn.h; reference
// models/Transformers.py:27-44).  The score layout is that of dcl_winattn_mfma.hip with a streaming loop over 32-token tiles:
//
//   forward, dq   (a workgroup owns 128 queries, a wave 32 of them, along its LANES; the keys stream)
//       S^T = K Q^T      keys along the accumulator registers (v_mfma_f32_32x32x16_f16 C layout: register r of lane l = row
//                        8 (r / 4) + 4 (l / 32) + r % 4, column l % 32): the row max / sum of a query are in-lane reductions plus one
//                        cross-lane step (l ^ 32).
//       O^T = V^T P^T    P^T never leaves the registers: registers 8 s .. 8 s + 7 of the score tile ARE the B fragment of k-step s
//                        once the contraction index is taken in the order kappa(s, half, t) = 16 s + 8 (t / 4) + 4 half + t % 4.
//       dQ^T = K^T dS^T  the same with dS^T = P^T (dP^T - delta), dP^T = V dO^T.
//   dk, dv        (a workgroup owns 128 keys, a wave 32 of them, along its lanes; the queries stream)
//       S = Q K^T, dP = dO V^T    queries along the registers, so that  dV^T = dO^T P  and  dK^T = Q^T dS  contract over them.
//
// Streamed tiles are staged ONCE per workgroup and split to hi / lo f16 on the way into LDS, in the two forms the products read:
//   F1  [channel / 8][token]    16-byte units: 8 consecutive channels of a token, the A fragment of a product over the channels
//   F2  [2 s + half][channel]   16-byte units: the 8 tokens kappa(s, half, 0..7) of a channel, the A fragment of a product over tokens
// The wave's own tokens (its B fragments over the channels) stay in registers.  Operand scales: powers of two from the absmax of
// q, k, v, dout per (image, head) (k_amax, integer atomicMax on the bits of non-negative floats); P takes 2^14 (P <= 1); dS a
// running power of two per wave that only ever decreases, the accumulator being rescaled when it moves (an f16 pair keeps 22 bits
// of every value down to 2^-16 of the scale's absmax, so earlier, smaller tiles lose nothing that counts).
// Tails: tokens >= N and channels >= D are never loaded (zeros are staged), their scores are -inf / their probabilities 0.
#include <math.h>

#include "dcl_f16x3.h"
#include "dcl_attn_plan.h"

namespace {

constexpr int NTHR = 256;             // four waves
constexpr int F1S = 33;               // token stride of an F1 tile in 16-byte units (32 + 1: conflict-free staging stores)
constexpr float P_SCALE = 16384.f;

struct AttnArgs {
    const float *qkv, *out, *lse_in, *dout, *delta_in;
    float *o, *lse, *dqkv, *delta;
    int *amax;                        // [B * heads][4]: bits of absmax q, k, v, dout
    int B, N, heads, D, C;
    float scale;
};

#define AMFMA(A, B, C) __builtin_amdgcn_mfma_f32_32x32x16_f16(as_half8(A), as_half8(B), (C), 0, 0, 0)

__device__ __forceinline__ float uniform(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// e^x for x <= 0 to about one ulp: the rounding error of x log2(e) is carried into the result (v_exp_f32 alone would leave
// |x| 2^-24 of relative error, which counts for the peaky rows); 0 below the f32 range, -inf included.
__device__ __forceinline__ float exp_acc(float x)
{
    const float L2E = 1.44269502e+0f, L2E_LO = 1.92596299e-8f;
    const float r = x * L2E;
    float e = fmaf(x, L2E, -r);
    e = fmaf(x, L2E_LO, e);
    const float p = exp2f(r);
    return r < -140.f ? 0.f : fmaf(p, e * 0.693147181f, p);
}

// (wide heads: the staging loops stay rolled -- unrolled, their loads in flight take the registers the wave's own fragments and
// accumulators need, and the kernels spill)
constexpr int stage_unroll(int DT) { return DT <= 4 ? 4 : 1; }

// ---- staging of a 32-token tile (tokens tok0 .., rows of stride rs floats starting at base) into LDS ------------------------
template <int DT>
__device__ __forceinline__ void stage_f1(u32x4 *Xh, u32x4 *Xl, const float *base, size_t rs, int tok0, int N, int D, float sc)
{
    constexpr int C8 = 4 * DT, UN = stage_unroll(DT);
#pragma unroll UN
    for (int u0 = 0; u0 < 32 * C8; u0 += NTHR) {
        const int u = u0 + (int)threadIdx.x;
        if (32 * C8 % NTHR != 0 && u >= 32 * C8)
            break;
        const int tok = u / C8, c8 = u - tok * C8;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (tok0 + tok < N && 8 * c8 < D) {
            const float *p = base + (size_t)(tok0 + tok) * rs + 8 * c8;
            const f32x4 a = *(const f32x4 *)p, b = *(const f32x4 *)(p + 4);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        }
        u32x4 hi, lo;
        split8(v, sc, hi, lo);
        Xh[c8 * F1S + tok] = hi;
        Xl[c8 * F1S + tok] = lo;
    }
}

template <int DT>
__device__ __forceinline__ void stage_f2(u32x4 *Xh, u32x4 *Xl, const float *base, size_t rs, int tok0, int N, int D, float sc)
{
    constexpr int Dp = 32 * DT, UN = stage_unroll(DT);
#pragma unroll UN
    for (int u0 = 0; u0 < 4 * Dp; u0 += NTHR) {
        const int u = u0 + (int)threadIdx.x;
        if (4 * Dp % NTHR != 0 && u >= 4 * Dp)
            break;
        const int g = u / Dp, ch = u - g * Dp;
        const int t0 = tok0 + 16 * (g >> 1) + 4 * (g & 1);
        float v[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int tok = t0 + 8 * (t >> 2) + (t & 3);
            v[t] = (tok < N && ch < D) ? base[(size_t)tok * rs + ch] : 0.f;
        }
        u32x4 hi, lo;
        split8(v, sc, hi, lo);
        Xh[u] = hi;
        Xl[u] = lo;
    }
}

// the wave's own 32 tokens (token `tok` on this lane) as B fragments over the channels: k-step ks holds channels 16 ks + 8 half ..
template <int DT>
__device__ __forceinline__ void own_frags(u32x4 (&xh)[2 * DT], u32x4 (&xl)[2 * DT], const float *base, size_t rs, int tok, int N,
                                          int D, float sc, int half)
{
#pragma unroll
    for (int ks = 0; ks < 2 * DT; ++ks) {
        const int ch = 16 * ks + 8 * half;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (tok < N && ch < D) {
            const float *p = base + (size_t)tok * rs + ch;
            const f32x4 a = *(const f32x4 *)p, b = *(const f32x4 *)(p + 4);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        }
        split8(v, sc, xh[ks], xl[ks]);
    }
}

// acc[32 x 32] = A (F1 tile in LDS: rows = its tokens) . B (own fragments: columns = this wave's tokens), over the channels
template <int DT>
__device__ __forceinline__ f32x16 prod_f1(const u32x4 *Ah, const u32x4 *Al, const u32x4 (&bh)[2 * DT], const u32x4 (&bl)[2 * DT],
                                          int half, int l32)
{
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r)
        acc[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 2 * DT; ++ks) {
        const u32x4 ah = Ah[(2 * ks + half) * F1S + l32], al = Al[(2 * ks + half) * F1S + l32];
        acc = AMFMA(ah, bl[ks], acc);
        acc = AMFMA(al, bh[ks], acc);
        acc = AMFMA(ah, bh[ks], acc);
    }
    return acc;
}

// a decreasing power-of-two scale for the tiles of dS: lower it (and the accumulators with it) when a tile's absmax asks for it
template <int AT>
__device__ __forceinline__ void lower_scale(float &sds, float tile_amax, f32x16 (&acc)[AT])
{
    const float am = uniform(wave_max(tile_amax));
    if (am > 0.f) {
        const float t = pow2_scale(am);
        if (t < sds) {
            const float f = t / sds;
#pragma unroll
            for (int a = 0; a < AT; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    acc[a][r] *= f;
            sds = t;
        }
    }
}

constexpr float SDS_START = 1.2676506e30f;      // 2^100: the largest pow2_scale

// ---- absmax of q, k, v (or dout) per (image, head) ------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHR) void k_attn_amax(const float *x, int N, int rs, int heads, int D, int part_stride, int slot0,
                                                    int *amax)
{
    const int bh = blockIdx.y, b = bh / heads, hd = bh - b * heads, part = blockIdx.z;
    const float *p = x + (size_t)b * N * rs + (size_t)part * part_stride + hd * D;
    const int t0 = blockIdx.x * 128, nt = min(128, N - t0), d4 = D / 4;
    float m = 0.f;
    for (int i = threadIdx.x; i < nt * d4; i += NTHR) {
        const int tok = i / d4, c = i - tok * d4;
        const f32x4 v = *(const f32x4 *)(p + (size_t)(t0 + tok) * rs + 4 * c);
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0)
        atomicMax(amax + bh * 4 + slot0 + part, __float_as_int(m));
}

// ---- delta[b, h, n] = sum_d dout[b, n, h D + d] out[b, n, h D + d] ------------------------------------------------------------------
__global__ __launch_bounds__(NTHR) void k_attn_delta(AttnArgs a)
{
    const int i = blockIdx.x * NTHR + threadIdx.x, b = blockIdx.y;
    if (i >= a.N * a.heads)
        return;
    const int n = i / a.heads, hd = i - n * a.heads;
    const size_t off = ((size_t)b * a.N + n) * a.C + hd * a.D;
    float s = 0.f;
    for (int d = 0; d < a.D; d += 4) {
        const f32x4 x = *(const f32x4 *)(a.dout + off + d), y = *(const f32x4 *)(a.out + off + d);
        s = fmaf(x.x, y.x, s);
        s = fmaf(x.y, y.y, s);
        s = fmaf(x.z, y.z, s);
        s = fmaf(x.w, y.w, s);
    }
    a.delta[((size_t)b * a.heads + hd) * a.N + n] = s;
}

// ---- forward -------------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(NTHR) void k_attn_fwd(AttnArgs a)
{
    extern __shared__ u32x4 lds[];
    constexpr int Dp = 32 * DT, C8 = 4 * DT;
    u32x4 *Kh = lds, *Kl = Kh + C8 * F1S, *Vh = Kl + C8 * F1S, *Vl = Vh + 4 * Dp;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, l32 = lane & 31;
    const int bh = blockIdx.y, b = bh / a.heads, hd = bh - b * a.heads;
    const int N = a.N, D = a.D;
    const size_t rs = 3 * (size_t)a.C;
    const float *qb = a.qkv + (size_t)b * N * rs + hd * D, *kb = qb + a.C, *vb = kb + a.C;
    const float sq = pow2_scale(__int_as_float(a.amax[bh * 4 + 0])), sk = pow2_scale(__int_as_float(a.amax[bh * 4 + 1])),
                sv = pow2_scale(__int_as_float(a.amax[bh * 4 + 2]));
    const int q0 = blockIdx.x * 128 + wave * 32, q = q0 + l32;
    const bool active = q0 < N;                                   // wave-uniform

    u32x4 qh[2 * DT], ql[2 * DT];
    own_frags<DT>(qh, ql, qb, rs, q, N, D, sq, h);
    split_to_mfma_fence();
    f32x16 ot[DT];
#pragma unroll
    for (int ct = 0; ct < DT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            ot[ct][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const float c = a.scale / (sq * sk);
    const int ntiles = (N + 31) / 32;

    for (int kt = 0; kt < ntiles; ++kt) {
        __syncthreads();                                          // the previous tile's reads are done
        stage_f1<DT>(Kh, Kl, kb, rs, kt * 32, N, D, sk);
        stage_f2<DT>(Vh, Vl, vb, rs, kt * 32, N, D, sv);
        __syncthreads();
        if (!active)
            continue;
        f32x16 st = prod_f1<DT>(Kh, Kl, qh, ql, h, l32);          // S^T, unscaled
        // online softmax over the keys of this lane's query
        float mt = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = kt * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
            const float s = key < N ? st[r] * c : -INFINITY;
            st[r] = s;
            mt = fmaxf(mt, s);
        }
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float m_new = fmaxf(m_run, mt);
        const float alpha = exp_acc(m_run - m_new);               // 0 at the first tile (m_run = -inf)
        float lt = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = exp_acc(st[r] - m_new);
            st[r] = p;
            lt += p;
        }
        l_run = l_run * alpha + lt;                               // (the two halves of a query are added at the end)
        m_run = m_new;
        if (__any(alpha != 1.f)) {                                // rescale only when a max of the wave moved
#pragma unroll
            for (int ct = 0; ct < DT; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    ot[ct][r] *= alpha;
        }
        // O^T += V^T P^T
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            float pp[8];
#pragma unroll
            for (int t = 0; t < 8; ++t)
                pp[t] = st[8 * s + t];
            u32x4 ph, pl;
            split8(pp, P_SCALE, ph, pl);
            split_to_mfma_fence();
#pragma unroll
            for (int ct = 0; ct < DT; ++ct) {
                const u32x4 vh = Vh[(2 * s + h) * Dp + 32 * ct + l32], vl = Vl[(2 * s + h) * Dp + 32 * ct + l32];
                ot[ct] = AMFMA(vh, pl, ot[ct]);
                ot[ct] = AMFMA(vl, ph, ot[ct]);
                ot[ct] = AMFMA(vh, ph, ot[ct]);
            }
        }
    }
    if (!active)
        return;
    const float l = l_run + __shfl_xor(l_run, 32, 64);
    if (q < N) {
        if (h == 0)
            a.lse[(size_t)bh * N + q] = m_run + logf(l);
        const float inv = (1.0f / l) * (1.0f / (sv * P_SCALE));
        float *op = a.o + ((size_t)b * N + q) * a.C + hd * D;
#pragma unroll
        for (int ct = 0; ct < DT; ++ct)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ch = 32 * ct + 8 * g + 4 * h;
                if (ch < D)
                    *(f32x4 *)(op + ch) = f32x4{ot[ct][4 * g] * inv, ot[ct][4 * g + 1] * inv, ot[ct][4 * g + 2] * inv,
                                                ot[ct][4 * g + 3] * inv};
            }
    }
}

// channel tiles [ct0, ct0 + AT) of acc^T[channel][this lane's token] -> columns col0 + channel of the token's row
template <int AT>
__device__ __forceinline__ void store_rows(const f32x16 (&acc)[AT], float m1, float m2, float *row, int ct0, int DT, int D, int h)
{
#pragma unroll
    for (int t = 0; t < AT; ++t) {
        if (ct0 + t >= DT)
            continue;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int ch = 32 * (ct0 + t) + 8 * g + 4 * h;
            if (ch < D)
                *(f32x4 *)(row + ch) = f32x4{acc[t][4 * g] * m1 * m2, acc[t][4 * g + 1] * m1 * m2, acc[t][4 * g + 2] * m1 * m2,
                                             acc[t][4 * g + 3] * m1 * m2};
        }
    }
}

// ---- backward, dq: query-block-owned, the keys stream; blockIdx.z picks AT of the DT channel tiles of dq ------------------------------
template <int DT, int AT>
__global__ __launch_bounds__(NTHR) void k_attn_bwd_dq(AttnArgs a)
{
    extern __shared__ u32x4 lds[];
    constexpr int Dp = 32 * DT, C8 = 4 * DT;
    u32x4 *Kh = lds, *Kl = Kh + C8 * F1S, *Vh = Kl + C8 * F1S, *Vl = Vh + C8 * F1S, *Th = Vl + C8 * F1S, *Tl = Th + 4 * Dp;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, l32 = lane & 31;
    const int bh = blockIdx.y, b = bh / a.heads, hd = bh - b * a.heads;
    const int N = a.N, D = a.D, ct0 = blockIdx.z * AT;
    const size_t rs = 3 * (size_t)a.C;
    const float *qb = a.qkv + (size_t)b * N * rs + hd * D, *kb = qb + a.C, *vb = kb + a.C;
    const float *gb = a.dout + (size_t)b * N * a.C + hd * D;
    const float sq = pow2_scale(__int_as_float(a.amax[bh * 4 + 0])), sk = pow2_scale(__int_as_float(a.amax[bh * 4 + 1])),
                sv = pow2_scale(__int_as_float(a.amax[bh * 4 + 2])), sg = pow2_scale(__int_as_float(a.amax[bh * 4 + 3]));
    const int q0 = blockIdx.x * 128 + wave * 32, q = q0 + l32;
    const bool active = q0 < N;

    u32x4 qh[2 * DT], ql[2 * DT], gh[2 * DT], gl[2 * DT];
    own_frags<DT>(qh, ql, qb, rs, q, N, D, sq, h);
    own_frags<DT>(gh, gl, gb, (size_t)a.C, q, N, D, sg, h);
    split_to_mfma_fence();
    const float lse_q = q < N ? a.lse_in[(size_t)bh * N + q] : 0.f, del_q = q < N ? a.delta_in[(size_t)bh * N + q] : 0.f;
    f32x16 acc[AT];
#pragma unroll
    for (int t = 0; t < AT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            acc[t][r] = 0.f;
    float sds = SDS_START;
    const float c = a.scale / (sq * sk), cP = 1.0f / (sv * sg);
    const int ntiles = (N + 31) / 32;

    for (int kt = 0; kt < ntiles; ++kt) {
        __syncthreads();
        stage_f1<DT>(Kh, Kl, kb, rs, kt * 32, N, D, sk);
        stage_f1<DT>(Vh, Vl, vb, rs, kt * 32, N, D, sv);
        stage_f2<DT>(Th, Tl, kb, rs, kt * 32, N, D, sk);
        __syncthreads();
        if (!active)
            continue;
        f32x16 st = prod_f1<DT>(Kh, Kl, qh, ql, h, l32);          // S^T = K Q^T
        const f32x16 dp = prod_f1<DT>(Vh, Vl, gh, gl, h, l32);    // dP^T = V dO^T
        float dsmax = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = kt * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
            const float p = (key < N && q < N) ? exp_acc(st[r] * c - lse_q) : 0.f;
            const float ds = p * (dp[r] * cP - del_q);
            st[r] = ds;
            dsmax = fmaxf(dsmax, fabsf(ds));
        }
        lower_scale<AT>(sds, dsmax, acc);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            float pp[8];
#pragma unroll
            for (int t = 0; t < 8; ++t)
                pp[t] = st[8 * s + t];
            u32x4 dh, dl;
            split8(pp, sds, dh, dl);
            split_to_mfma_fence();
#pragma unroll
            for (int t = 0; t < AT; ++t) {
                if (ct0 + t >= DT)
                    continue;
                const u32x4 xh = Th[(2 * s + h) * Dp + 32 * (ct0 + t) + l32], xl = Tl[(2 * s + h) * Dp + 32 * (ct0 + t) + l32];
                acc[t] = AMFMA(xh, dl, acc[t]);                   // dQ^T += K^T dS^T
                acc[t] = AMFMA(xl, dh, acc[t]);
                acc[t] = AMFMA(xh, dh, acc[t]);
            }
        }
    }
    if (active && q < N)
        store_rows<AT>(acc, a.scale / sk, 1.0f / sds, a.dqkv + ((size_t)b * N + q) * rs + hd * D, ct0, DT, D, h);
}

// ---- backward, dk and dv: key-block-owned, the queries stream; blockIdx.z picks AT of the DT channel tiles -----------------------------
template <int DT, int AT>
__global__ __launch_bounds__(NTHR) void k_attn_bwd_dkv(AttnArgs a)
{
    extern __shared__ u32x4 lds[];
    constexpr int Dp = 32 * DT, C8 = 4 * DT;
    u32x4 *Qh = lds, *Ql = Qh + C8 * F1S, *Gh = Ql + C8 * F1S, *Gl = Gh + C8 * F1S;
    u32x4 *QTh = Gl + C8 * F1S, *QTl = QTh + 4 * Dp, *GTh = QTl + 4 * Dp, *GTl = GTh + 4 * Dp;
    float *Ls = (float *)(GTl + 4 * Dp), *Ds = Ls + 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, l32 = lane & 31;
    const int bh = blockIdx.y, b = bh / a.heads, hd = bh - b * a.heads;
    const int N = a.N, D = a.D, ct0 = blockIdx.z * AT;
    const size_t rs = 3 * (size_t)a.C;
    const float *qb = a.qkv + (size_t)b * N * rs + hd * D, *kb = qb + a.C, *vb = kb + a.C;
    const float *gb = a.dout + (size_t)b * N * a.C + hd * D;
    const float sq = pow2_scale(__int_as_float(a.amax[bh * 4 + 0])), sk = pow2_scale(__int_as_float(a.amax[bh * 4 + 1])),
                sv = pow2_scale(__int_as_float(a.amax[bh * 4 + 2])), sg = pow2_scale(__int_as_float(a.amax[bh * 4 + 3]));
    const int k0 = blockIdx.x * 128 + wave * 32, key = k0 + l32;
    const bool active = k0 < N;

    u32x4 kh[2 * DT], kl[2 * DT], vh[2 * DT], vl[2 * DT];
    own_frags<DT>(kh, kl, kb, rs, key, N, D, sk, h);
    own_frags<DT>(vh, vl, vb, rs, key, N, D, sv, h);
    split_to_mfma_fence();
    f32x16 accK[AT], accV[AT];
#pragma unroll
    for (int t = 0; t < AT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            accK[t][r] = 0.f;
            accV[t][r] = 0.f;
        }
    float sds = SDS_START;
    const float c = a.scale / (sq * sk), cP = 1.0f / (sv * sg);
    const int ntiles = (N + 31) / 32;

    for (int qt = 0; qt < ntiles; ++qt) {
        __syncthreads();
        stage_f1<DT>(Qh, Ql, qb, rs, qt * 32, N, D, sq);
        stage_f1<DT>(Gh, Gl, gb, (size_t)a.C, qt * 32, N, D, sg);
        stage_f2<DT>(QTh, QTl, qb, rs, qt * 32, N, D, sq);
        stage_f2<DT>(GTh, GTl, gb, (size_t)a.C, qt * 32, N, D, sg);
        if (threadIdx.x < 32) {
            const int tok = qt * 32 + (int)threadIdx.x;
            Ls[threadIdx.x] = tok < N ? a.lse_in[(size_t)bh * N + tok] : 0.f;
            Ds[threadIdx.x] = tok < N ? a.delta_in[(size_t)bh * N + tok] : 0.f;
        }
        __syncthreads();
        if (!active)
            continue;
        f32x16 st = prod_f1<DT>(Qh, Ql, kh, kl, h, l32);          // S = Q K^T: queries along the registers
        f32x16 dp = prod_f1<DT>(Gh, Gl, vh, vl, h, l32);          // dP = dO V^T
        float dsmax = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 ll = *(const f32x4 *)(Ls + 8 * g + 4 * h), dd = *(const f32x4 *)(Ds + 8 * g + 4 * h);
            const float lv[4] = {ll.x, ll.y, ll.z, ll.w}, dv[4] = {dd.x, dd.y, dd.z, dd.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 4 * g + e, qtok = qt * 32 + 8 * g + 4 * h + e;
                const float p = (qtok < N && key < N) ? exp_acc(st[r] * c - lv[e]) : 0.f;
                const float ds = p * (dp[r] * cP - dv[e]);
                st[r] = p;
                dp[r] = ds;
                dsmax = fmaxf(dsmax, fabsf(ds));
            }
        }
        lower_scale<AT>(sds, dsmax, accK);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            float pp[8], dd[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                pp[t] = st[8 * s + t];
                dd[t] = dp[8 * s + t];
            }
            u32x4 ph, pl, dh, dl;
            split8(pp, P_SCALE, ph, pl);
            split8(dd, sds, dh, dl);
            split_to_mfma_fence();
#pragma unroll
            for (int t = 0; t < AT; ++t) {
                if (ct0 + t >= DT)
                    continue;
                const int u = (2 * s + h) * Dp + 32 * (ct0 + t) + l32;
                const u32x4 xh = GTh[u], xl = GTl[u], yh = QTh[u], yl = QTl[u];
                accV[t] = AMFMA(xh, pl, accV[t]);                 // dV^T += dO^T P
                accV[t] = AMFMA(xl, ph, accV[t]);
                accV[t] = AMFMA(xh, ph, accV[t]);
                accK[t] = AMFMA(yh, dl, accK[t]);                 // dK^T += Q^T dS
                accK[t] = AMFMA(yl, dh, accK[t]);
                accK[t] = AMFMA(yh, dh, accK[t]);
            }
        }
    }
    if (active && key < N) {
        float *row = a.dqkv + ((size_t)b * N + key) * rs + hd * D;
        store_rows<AT>(accK, a.scale / sq, 1.0f / sds, row + a.C, ct0, DT, D, h);
        store_rows<AT>(accV, 1.0f / sg, 1.0f / P_SCALE, row + 2 * a.C, ct0, DT, D, h);
    }
}

constexpr size_t lds_fwd(int DT) { return 16 * (size_t)(2 * 4 * DT * F1S + 2 * 4 * 32 * DT); }
constexpr size_t lds_dq(int DT) { return 16 * (size_t)(4 * 4 * DT * F1S + 2 * 4 * 32 * DT); }
constexpr size_t lds_dkv(int DT) { return 16 * (size_t)(4 * 4 * DT * F1S + 4 * 4 * 32 * DT) + 256; }
// channel tiles of the gradients one launch plane (blockIdx.z) accumulates: what the register file holds next to the wave's own
// fragments (512 registers at one wave per SIMD)
constexpr int at_dq(int DT) { return DT <= 4 ? DT : 4; }
constexpr int at_dkv(int DT) { return DT <= 4 ? DT : (DT <= 6 ? 3 : 2); }

template <typename K>
int launch(K kern, dim3 grid, size_t lds, hipStream_t st, const AttnArgs &a, const char *what)
{
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            dat_set_error("%s: hipFuncSetAttribute(MaxDynamicSharedMemorySize = %d): %s", what, (int)lds, hipGetErrorString(e));
            return (int)e;
        }
    }
    hipLaunchKernelGGL(kern, grid, dim3(NTHR), lds, st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        dat_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return DAT_OK;
}

int common_args(const void *qkv, const void *x1, const void *x2, int B, int N, int heads, int D, void *ws, int64_t ws_bytes,
                int backward, DatLayout *lay, const char *what)
{
    if (!dat_layout(B, N, heads, D, backward, lay)) {
        dat_set_error("%s: shape not taken (dat_supported)", what);
        return DAT_EINVAL;
    }
    if (!qkv || !x1 || !x2 || !ws) {
        dat_set_error("%s: null pointer", what);
        return DAT_EINVAL;
    }
    if (((uintptr_t)qkv | (uintptr_t)x1 | (uintptr_t)x2) % 16 != 0 || (uintptr_t)ws % 256 != 0) {
        dat_set_error("%s: tensors must be 16-byte aligned, the workspace 256-byte aligned", what);
        return DAT_EINVAL;
    }
    if (ws_bytes < lay->bytes) {
        dat_set_error("%s: workspace of %lld bytes, %lld needed", what, (long long)ws_bytes, (long long)lay->bytes);
        return DAT_EINVAL;
    }
    return DAT_OK;
}

int amax_launch(const float *x, int B, int N, int heads, int D, int rs, int parts, int slot0, int *amax, hipStream_t st,
                const char *what)
{
    hipLaunchKernelGGL(k_attn_amax, dim3((unsigned)((N + 127) / 128), (unsigned)(B * heads), (unsigned)parts), dim3(NTHR), 0, st, x,
                       N, rs, heads, D, heads * D, slot0, amax);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        dat_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return DAT_OK;
}

}  // namespace

#define DAT_FOR_DT(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)

extern "C" int dat_attn_fwd(const float *qkv, int B, int N, int heads, int D, float scale, void *workspace, int64_t workspace_bytes,
                            float *out, float *lse, void *stream)
{
    DatLayout lay;
    int rc = common_args(qkv, out, lse, B, N, heads, D, workspace, workspace_bytes, 0, &lay, __func__);
    if (rc != DAT_OK)
        return rc;
    hipStream_t st = (hipStream_t)stream;
    AttnArgs a = {};
    a.qkv = qkv; a.o = out; a.lse = lse;
    a.amax = (int *)((char *)workspace + lay.amax);
    a.B = B; a.N = N; a.heads = heads; a.D = D; a.C = heads * D; a.scale = scale;
    hipError_t e = hipMemsetAsync(a.amax, 0, 16 * (size_t)B * heads, st);
    if (e != hipSuccess) {
        dat_set_error("%s: hipMemsetAsync: %s", __func__, hipGetErrorString(e));
        return (int)e;
    }
    if ((rc = amax_launch(qkv, B, N, heads, D, 3 * a.C, 3, 0, a.amax, st, __func__)) != DAT_OK)
        return rc;
    const dim3 grid((unsigned)((N + 127) / 128), (unsigned)(B * heads));
    switch ((D + 31) / 32) {
#define X(DT_) case DT_: return launch(k_attn_fwd<DT_>, grid, lds_fwd(DT_), st, a, __func__);
        DAT_FOR_DT(X)
#undef X
    }
    return DAT_EINVAL;
}

extern "C" int dat_attn_bwd(const float *qkv, const float *out, const float *lse, const float *dout, int B, int N, int heads, int D,
                            float scale, void *workspace, int64_t workspace_bytes, float *dqkv, void *stream)
{
    DatLayout lay;
    int rc = common_args(qkv, out, dout, B, N, heads, D, workspace, workspace_bytes, 1, &lay, __func__);
    if (rc != DAT_OK)
        return rc;
    if (!lse || !dqkv || (uintptr_t)dqkv % 16 != 0) {
        dat_set_error("%s: lse / dqkv null or dqkv not 16-byte aligned", __func__);
        return DAT_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    AttnArgs a = {};
    a.qkv = qkv; a.out = out; a.lse_in = lse; a.dout = dout; a.dqkv = dqkv;
    a.amax = (int *)((char *)workspace + lay.amax);
    a.delta = (float *)((char *)workspace + lay.delta);
    a.delta_in = a.delta;
    a.B = B; a.N = N; a.heads = heads; a.D = D; a.C = heads * D; a.scale = scale;
    hipError_t e = hipMemsetAsync(a.amax, 0, 16 * (size_t)B * heads, st);
    if (e != hipSuccess) {
        dat_set_error("%s: hipMemsetAsync: %s", __func__, hipGetErrorString(e));
        return (int)e;
    }
    if ((rc = amax_launch(qkv, B, N, heads, D, 3 * a.C, 3, 0, a.amax, st, __func__)) != DAT_OK)
        return rc;
    if ((rc = amax_launch(dout, B, N, heads, D, a.C, 1, 3, a.amax, st, __func__)) != DAT_OK)
        return rc;
    hipLaunchKernelGGL(k_attn_delta, dim3((unsigned)(((int64_t)N * heads + NTHR - 1) / NTHR), (unsigned)B), dim3(NTHR), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) {
        dat_set_error("%s: launch failed: %s", __func__, hipGetErrorString(e));
        return (int)e;
    }
    const unsigned gx = (unsigned)((N + 127) / 128), gy = (unsigned)(B * heads);
    switch ((D + 31) / 32) {
#define X(DT_)                                                                                                                   \
    case DT_:                                                                                                                    \
        rc = launch(k_attn_bwd_dkv<DT_, at_dkv(DT_)>, dim3(gx, gy, (DT_ + at_dkv(DT_) - 1) / at_dkv(DT_)), lds_dkv(DT_), st, a,  \
                    __func__);                                                                                                   \
        if (rc != DAT_OK)                                                                                                        \
            return rc;                                                                                                           \
        return launch(k_attn_bwd_dq<DT_, at_dq(DT_)>, dim3(gx, gy, (DT_ + at_dq(DT_) - 1) / at_dq(DT_)), lds_dq(DT_), st, a,     \
                      __func__);
        DAT_FOR_DT(X)
#undef X
    }
    return DAT_EINVAL;
}
