// dcl_ocr.hip -- the OCR context core (include/dcl_ocr.h): spatial gather and object attention, forward and backward.
//
// All four heavy products have one small dimension (K <= 256 classes) and one long one (N pixels).  A workgroup of 256 threads,
// seen as 16 x 16 (ty, tx), owns a tile of NT = 64 pixels with all classes, padded to KP = 16 KI, as one fp32 matrix M[KP][64] in
// LDS (row stride MS = 68 floats: float4 reads stay aligned and the 16 rows of one class step fall into distinct banks).  Three
// routines do the work, all plain fp32 FMA from LDS-staged operands:
//   scores   acc[k][n] = sum_c W(k, c) X[c][n]      thread: classes ty + 16 i, pixels 4 tx .. 4 tx + 3; C in steps of 16
//   apply    O[c][n]   = f sum_k M[k][n] V(c, k)    thread: channels c0 + ty + 16 j, the same pixels; 64 channels, K in steps of 16
//   reduce_n acc[k][c] += sum_n M[k][n] A[c][n]     thread: classes ty + 16 i, channels c0 + tx + 16 j; one 64-channel chunk
// W and V are the small per-image matrices (dctx, key, val), read with two strides so that neither is ever transposed in memory.
// Sums over N (ctx, dval, dkey) are per-split partials in registers over a fixed range of tiles, written to the workspace and
// added in split order by k_sum_splits: no atomics, bitwise reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <initializer_list>

#include "dcl_ocr_plan.h"

namespace {

constexpr int NTHR = 256;
constexpr int NT = DCO_TILE_N;     // pixels of a tile
constexpr int CH = DCO_CHUNK_C;    // channels of a chunk
constexpr int MS = 68;             // row stride of the 64-pixel LDS matrices
constexpr int CC = 16;             // reduction step of scores / apply
constexpr int WS = 20;             // row stride of the 16-wide operand tiles (W, V)
constexpr int RED = 1024;          // floats of the small reduction / statistics area

constexpr int stage_floats(int KI) { return (2 * KI * 16 * WS + CC * MS) > CH * MS ? (2 * KI * 16 * WS + CC * MS) : CH * MS; }
constexpr size_t lds_bytes(int KI) { return sizeof(float) * (size_t)(KI * 16 * MS + stage_floats(KI) + RED); }

struct Lds {
    float *M, *stage, *red;
};

template <int KI>
__device__ inline Lds carve(float *base)
{
    Lds l;
    l.M = base;
    l.stage = base + KI * 16 * MS;
    l.red = l.stage + stage_floats(KI);
    return l;
}

// four pixels n0 + col .. + 3 of a row of N floats; zero beyond N
__device__ inline float4 load_px4(const float *row, int N, int n, bool vec)
{
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vec) {
        if (n < N)
            v = *reinterpret_cast<const float4 *>(row + n);
    } else {
        if (n < N) v.x = row[n];
        if (n + 1 < N) v.y = row[n + 1];
        if (n + 2 < N) v.z = row[n + 2];
        if (n + 3 < N) v.w = row[n + 3];
    }
    return v;
}

__device__ inline void store_px4(float *row, int N, int n, bool vec, float4 v)
{
    if (vec) {
        if (n < N)
            *reinterpret_cast<float4 *>(row + n) = v;
    } else {
        if (n < N) row[n] = v.x;
        if (n + 1 < N) row[n + 1] = v.y;
        if (n + 2 < N) row[n + 2] = v.z;
        if (n + 3 < N) row[n + 3] = v.w;
    }
}

__device__ inline void fma4(float (&a)[4], float w, const float4 &x)
{
    a[0] = fmaf(w, x.x, a[0]);
    a[1] = fmaf(w, x.y, a[1]);
    a[2] = fmaf(w, x.z, a[2]);
    a[3] = fmaf(w, x.w, a[3]);
}

// acc[i][p] = sum_c W(ty + 16 i, c) X[c][n0 + 4 tx + p]; W(k, c) = W[k wsk + c wsc], zero for k >= K.  C % 16 == 0.
// SUB: acc[i][p] = sum_c W(k, c) (X[c][n] - S(k, c)) instead, S laid out as W: the difference is taken BEFORE the product, so that
// where X[., n] is close to S(k, .) the sum keeps the accuracy of its small terms.
template <int KI, bool SUB = false>
__device__ inline void scores(float (&acc)[KI][4], const float *W, int wsk, int wsc, int K, const float *X, int C, int N, int n0,
                              bool vec, float *stage, const float *S = nullptr)
{
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    float *Wl = stage, *Sl = stage + KI * 16 * WS, *Xl = stage + 2 * KI * 16 * WS;
#pragma unroll
    for (int i = 0; i < KI; ++i)
        acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.f;
#pragma unroll 1
    for (int c0 = 0; c0 < C; c0 += CC) {
        __syncthreads();
        for (int e = t; e < KI * 16 * CC; e += NTHR) {
            int k, cc;
            if (wsc == 1) {
                cc = e & 15;
                k = e >> 4;
            } else {
                k = e % (KI * 16);
                cc = e / (KI * 16);
            }
            Wl[k * WS + cc] = k < K ? W[(size_t)k * wsk + (size_t)(c0 + cc) * wsc] : 0.f;
            if (SUB)
                Sl[k * WS + cc] = k < K ? S[(size_t)k * wsk + (size_t)(c0 + cc) * wsc] : 0.f;
        }
        *reinterpret_cast<float4 *>(&Xl[ty * MS + tx * 4]) = load_px4(X + (size_t)(c0 + ty) * N, N, n0 + tx * 4, vec);
        __syncthreads();
#pragma unroll
        for (int cc = 0; cc < CC; cc += 4) {
            const float4 x0 = *reinterpret_cast<const float4 *>(&Xl[(cc + 0) * MS + tx * 4]);
            const float4 x1 = *reinterpret_cast<const float4 *>(&Xl[(cc + 1) * MS + tx * 4]);
            const float4 x2 = *reinterpret_cast<const float4 *>(&Xl[(cc + 2) * MS + tx * 4]);
            const float4 x3 = *reinterpret_cast<const float4 *>(&Xl[(cc + 3) * MS + tx * 4]);
#pragma unroll
            for (int i = 0; i < KI; ++i) {
                const float4 w = *reinterpret_cast<const float4 *>(&Wl[(ty + 16 * i) * WS + cc]);
                if (SUB) {
                    const float4 m = *reinterpret_cast<const float4 *>(&Sl[(ty + 16 * i) * WS + cc]);
                    fma4(acc[i], w.x, make_float4(x0.x - m.x, x0.y - m.x, x0.z - m.x, x0.w - m.x));
                    fma4(acc[i], w.y, make_float4(x1.x - m.y, x1.y - m.y, x1.z - m.y, x1.w - m.y));
                    fma4(acc[i], w.z, make_float4(x2.x - m.z, x2.y - m.z, x2.z - m.z, x2.w - m.z));
                    fma4(acc[i], w.w, make_float4(x3.x - m.w, x3.y - m.w, x3.z - m.w, x3.w - m.w));
                } else {
                    fma4(acc[i], w.x, x0);
                    fma4(acc[i], w.y, x1);
                    fma4(acc[i], w.z, x2);
                    fma4(acc[i], w.w, x3);
                }
            }
        }
    }
}

// O[c][n0 + 4 tx + p] = f sum_k M[k][4 tx + p] V(c, k) for every c < C; V(c, k) = V[c vsc + k vsk].  (Starts with a barrier: M
// may have been written just before.)
template <int KI>
__device__ inline void apply(const float *M, const float *V, int vsc, int vsk, int K, int C, float f, float *O, int N, int n0,
                             bool vec, float *stage)
{
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    float *Vl = stage;
#pragma unroll 1
    for (int c0 = 0; c0 < C; c0 += CH) {
        float acc[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0.f;
#pragma unroll 1
        for (int k0 = 0; k0 < KI * 16; k0 += CC) {
            __syncthreads();
            for (int e = t; e < CH * CC; e += NTHR) {
                int c, kk;
                if (vsk == 1) {
                    kk = e & 15;
                    c = e >> 4;
                } else {
                    c = e & 63;
                    kk = e >> 6;
                }
                Vl[c * WS + kk] = (c0 + c < C && k0 + kk < K) ? V[(size_t)(c0 + c) * vsc + (size_t)(k0 + kk) * vsk] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < CC; kk += 4) {
                const float4 m0 = *reinterpret_cast<const float4 *>(&M[(k0 + kk + 0) * MS + tx * 4]);
                const float4 m1 = *reinterpret_cast<const float4 *>(&M[(k0 + kk + 1) * MS + tx * 4]);
                const float4 m2 = *reinterpret_cast<const float4 *>(&M[(k0 + kk + 2) * MS + tx * 4]);
                const float4 m3 = *reinterpret_cast<const float4 *>(&M[(k0 + kk + 3) * MS + tx * 4]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float4 v = *reinterpret_cast<const float4 *>(&Vl[(ty + 16 * j) * WS + kk]);
                    fma4(acc[j], v.x, m0);
                    fma4(acc[j], v.y, m1);
                    fma4(acc[j], v.z, m2);
                    fma4(acc[j], v.w, m3);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + ty + 16 * j;
            if (c < C)
                store_px4(O + (size_t)c * N, N, n0 + tx * 4, vec,
                          make_float4(f * acc[j][0], f * acc[j][1], f * acc[j][2], f * acc[j][3]));
        }
    }
}

// acc[i][j] += sum_n M[ty + 16 i][n] A[c0 + tx + 16 j][n0 + n]; rows c >= C and pixels >= N read as zero.  (Starts with a barrier.)
template <int KI>
__device__ inline void reduce_n(float (&acc)[KI][4], const float *M, const float *A, int C, int c0, int N, int n0, bool vec,
                                float *stage)
{
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    float *Al = stage;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int r = ty + 16 * u, c = c0 + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < C)
            v = load_px4(A + (size_t)c * N, N, n0 + tx * 4, vec);
        *reinterpret_cast<float4 *>(&Al[r * MS + tx * 4]) = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int n = 0; n < NT; n += 4) {
        float4 a[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            a[j] = *reinterpret_cast<const float4 *>(&Al[(tx + 16 * j) * MS + n]);
#pragma unroll
        for (int i = 0; i < KI; ++i) {
            const float4 m = *reinterpret_cast<const float4 *>(&M[(ty + 16 * i) * MS + n]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float s = acc[i][j];
                s = fmaf(m.x, a[j].x, s);
                s = fmaf(m.y, a[j].y, s);
                s = fmaf(m.z, a[j].z, s);
                s = fmaf(m.w, a[j].w, s);
                acc[i][j] = s;
            }
        }
    }
}

// M[k][n] := softmax over k < K of M[k][n] for each of the 64 pixel columns; rows K .. 16 KI - 1 := 0.  Ends with a barrier.
template <int KI>
__device__ inline void softmax_k(float *M, int K, float *red)
{
    const int t = threadIdx.x, n = t & 63, part = t >> 6;
    __syncthreads();
    float mx = -INFINITY;
    for (int k = part; k < K; k += 4)
        mx = fmaxf(mx, M[k * MS + n]);
    red[part * 64 + n] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[n], red[64 + n]), fmaxf(red[128 + n], red[192 + n]));
    __syncthreads();
    float sum = 0.f;
    for (int k = part; k < K; k += 4) {
        const float e = expf(M[k * MS + n] - mx);
        M[k * MS + n] = e;
        sum += e;
    }
    red[part * 64 + n] = sum;
    __syncthreads();
    const float inv = 1.0f / (((red[n] + red[64 + n]) + red[128 + n]) + red[192 + n]);
    for (int k = part; k < K; k += 4)
        M[k * MS + n] *= inv;
    for (int k = K + part; k < KI * 16; k += 4)
        M[k * MS + n] = 0.f;
    __syncthreads();
}

// the range of tiles of one split
__device__ inline void split_range(int N, int nsplit, int split, int *first, int *last)
{
    const int tiles = (N + NT - 1) / NT, per = (tiles + nsplit - 1) / nsplit;
    *first = split * per;
    *last = min(tiles, *first + per);
}

// ---- gather --------------------------------------------------------------------------------------------------------------------

// stats[b, k] = (max_n z, sum_n exp(z - max)), z = scale * logits.  grid (K, B)
__global__ __launch_bounds__(NTHR) void k_gather_stats(const float *logits, int K, int N, float scale, float *stats)
{
    __shared__ float red[NTHR];
    const int t = threadIdx.x, k = blockIdx.x, b = blockIdx.y;
    const float *row = logits + ((size_t)b * K + k) * N;
    float mx = -INFINITY;
    for (int n = t; n < N; n += NTHR)
        mx = fmaxf(mx, scale * row[n]);
    red[t] = mx;
    __syncthreads();
    for (int s = NTHR / 2; s > 0; s >>= 1) {
        if (t < s)
            red[t] = fmaxf(red[t], red[t + s]);
        __syncthreads();
    }
    mx = red[0];
    __syncthreads();
    float sum = 0.f;
    for (int n = t; n < N; n += NTHR)
        sum += expf(scale * row[n] - mx);
    red[t] = sum;
    __syncthreads();
    for (int s = NTHR / 2; s > 0; s >>= 1) {
        if (t < s)
            red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) {
        stats[((size_t)b * K + k) * 2] = mx;
        stats[((size_t)b * K + k) * 2 + 1] = red[0];
    }
}

struct GatherArgs {
    const float *x, *logits, *stats, *dctx, *ctx;
    float *part, *dx, *dlogits;
    int C, K, N, nsplit, vec;
    float scale;
};

// red[k] = max, red[256 + k] = 1 / sum of class k of image b
__device__ inline void load_stats(const float *stats, int b, int K, float *red)
{
    const int t = threadIdx.x;
    if (t < K) {
        red[t] = stats[((size_t)b * K + t) * 2];
        red[256 + t] = 1.0f / stats[((size_t)b * K + t) * 2 + 1];
    }
}

// partial ctx of one split and one channel chunk.  grid (nsplit, B, chunks)
template <int KI>
__global__ __launch_bounds__(NTHR) void k_gather_fwd(GatherArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Lds l = carve<KI>(lds);
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int split = blockIdx.x, b = blockIdx.y, c0 = blockIdx.z * CH;
    const int C = a.C, K = a.K, N = a.N;
    const float *xb = a.x + (size_t)b * C * N, *lb = a.logits + (size_t)b * K * N;
    load_stats(a.stats, b, K, l.red);
    float acc[KI][4];
#pragma unroll
    for (int i = 0; i < KI; ++i)
        acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.f;
    int first, last;
    split_range(N, a.nsplit, split, &first, &last);
#pragma unroll 1
    for (int tile = first; tile < last; ++tile) {
        const int n0 = tile * NT;
        __syncthreads();
        for (int e = t; e < KI * 16 * NT; e += NTHR) {
            const int k = e >> 6, n = e & 63;
            float p = 0.f;
            if (k < K && n0 + n < N)
                p = expf(a.scale * lb[(size_t)k * N + n0 + n] - l.red[k]) * l.red[256 + k];
            l.M[k * MS + n] = p;
        }
        reduce_n<KI>(acc, l.M, xb, C, c0, N, n0, a.vec, l.stage);
    }
    float *pb = a.part + ((size_t)b * a.nsplit + split) * K * C;
#pragma unroll
    for (int i = 0; i < KI; ++i) {
        const int k = ty + 16 * i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + tx + 16 * j;
            if (k < K && c < C)
                pb[(size_t)k * C + c] = acc[i][j];
        }
    }
}

// dlogits and dx of one pixel tile.  grid (tiles, B)
template <int KI>
__global__ __launch_bounds__(NTHR) void k_gather_bwd(GatherArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Lds l = carve<KI>(lds);
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int n0 = blockIdx.x * NT, b = blockIdx.y;
    const int C = a.C, K = a.K, N = a.N;
    const float *xb = a.x + (size_t)b * C * N, *lb = a.logits + (size_t)b * K * N, *db = a.dctx + (size_t)b * K * C;
    load_stats(a.stats, b, K, l.red);
    // g[k][n] = sum_c dctx[k, c] (x[c, n] - ctx[k, c]) = (sum_c dctx x) - dot[k]: at a pixel that owns its class x is close to ctx,
    // and the difference of two separately rounded sums would lose what the softmax's own backward keeps
    float g[KI][4];
    scores<KI, true>(g, db, C, 1, K, xb, C, N, n0, a.vec, l.stage, a.ctx + (size_t)b * K * C);   // (its barriers publish red)
#pragma unroll
    for (int i = 0; i < KI; ++i) {
        const int k = ty + 16 * i;
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < K) {
            const float4 z = load_px4(lb + (size_t)k * N, N, n0 + tx * 4, a.vec);
            const float mx = l.red[k], inv = l.red[256 + k];
            const int n = n0 + tx * 4;
            p.x = n < N ? expf(a.scale * z.x - mx) * inv : 0.f;
            p.y = n + 1 < N ? expf(a.scale * z.y - mx) * inv : 0.f;
            p.z = n + 2 < N ? expf(a.scale * z.z - mx) * inv : 0.f;
            p.w = n + 3 < N ? expf(a.scale * z.w - mx) * inv : 0.f;
            store_px4(a.dlogits + ((size_t)b * K + k) * N, N, n, a.vec,
                      make_float4(a.scale * p.x * g[i][0], a.scale * p.y * g[i][1], a.scale * p.z * g[i][2], a.scale * p.w * g[i][3]));
        }
        *reinterpret_cast<float4 *>(&l.M[k * MS + tx * 4]) = p;
    }
    apply<KI>(l.M, db, 1, C, K, C, 1.0f, a.dx + (size_t)b * C * N, N, n0, a.vec, l.stage);
}

// out[b, e] = f sum_s part[b, s, e] in the order of s.  grid (ceil(E / 256), B)
__global__ __launch_bounds__(NTHR) void k_sum_splits(const float *part, size_t image_stride, size_t split_stride, int nsplit, int E,
                                                     float f, float *out)
{
    const int e = blockIdx.x * NTHR + threadIdx.x, b = blockIdx.y;
    if (e >= E)
        return;
    const float *p = part + (size_t)b * image_stride + e;
    float s = 0.f;
    for (int i = 0; i < nsplit; ++i)
        s += p[(size_t)i * split_stride];
    out[(size_t)b * E + e] = f * s;
}

// ---- object attention ----------------------------------------------------------------------------------------------------------

struct AttnArgs {
    const float *q, *key, *val, *dout;
    float *out, *dq, *part;
    int Ck, K, N, nsplit, vec;
    float s;
};

// M := a = softmax_K(s q^T key) of the tile.  Ends with a barrier.
template <int KI>
__device__ inline void attn_probs(const AttnArgs &a, int b, int n0, const Lds &l)
{
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    float acc[KI][4];
    scores<KI>(acc, a.key + (size_t)b * a.Ck * a.K, 1, a.K, a.K, a.q + (size_t)b * a.Ck * a.N, a.Ck, a.N, n0, a.vec, l.stage);
#pragma unroll
    for (int i = 0; i < KI; ++i)
        *reinterpret_cast<float4 *>(&l.M[(ty + 16 * i) * MS + tx * 4]) =
            make_float4(a.s * acc[i][0], a.s * acc[i][1], a.s * acc[i][2], a.s * acc[i][3]);
    softmax_k<KI>(l.M, a.K, l.red);
}

// with a in M: dP = dout^T val in registers, then dS[k][n] = a (dP - sum_k a dP) in ds (the thread's own elements of M)
template <int KI>
__device__ inline void attn_dscores(const AttnArgs &a, int b, int n0, const Lds &l, float (&ds)[KI][4])
{
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    scores<KI>(ds, a.val + (size_t)b * a.Ck * a.K, 1, a.K, a.K, a.dout + (size_t)b * a.Ck * a.N, a.Ck, a.N, n0, a.vec, l.stage);
    float part[4] = {0.f, 0.f, 0.f, 0.f};
    float4 pr[KI];
#pragma unroll
    for (int i = 0; i < KI; ++i) {
        pr[i] = *reinterpret_cast<const float4 *>(&l.M[(ty + 16 * i) * MS + tx * 4]);
        part[0] = fmaf(pr[i].x, ds[i][0], part[0]);
        part[1] = fmaf(pr[i].y, ds[i][1], part[1]);
        part[2] = fmaf(pr[i].z, ds[i][2], part[2]);
        part[3] = fmaf(pr[i].w, ds[i][3], part[3]);
    }
    __syncthreads();
    *reinterpret_cast<float4 *>(&l.red[ty * 64 + tx * 4]) = make_float4(part[0], part[1], part[2], part[3]);
    __syncthreads();
    float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int y = 0; y < 16; ++y) {
        const float4 r = *reinterpret_cast<const float4 *>(&l.red[y * 64 + tx * 4]);
        d.x += r.x;
        d.y += r.y;
        d.z += r.z;
        d.w += r.w;
    }
#pragma unroll
    for (int i = 0; i < KI; ++i) {
        ds[i][0] = pr[i].x * (ds[i][0] - d.x);
        ds[i][1] = pr[i].y * (ds[i][1] - d.y);
        ds[i][2] = pr[i].z * (ds[i][2] - d.z);
        ds[i][3] = pr[i].w * (ds[i][3] - d.w);
    }
}

template <int KI>
__device__ inline void put_own(float *M, const float (&v)[KI][4])
{
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
#pragma unroll
    for (int i = 0; i < KI; ++i)
        *reinterpret_cast<float4 *>(&M[(ty + 16 * i) * MS + tx * 4]) = make_float4(v[i][0], v[i][1], v[i][2], v[i][3]);
}

// grid (tiles, B)
template <int KI>
__global__ __launch_bounds__(NTHR) void k_attn_fwd(AttnArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Lds l = carve<KI>(lds);
    const int n0 = blockIdx.x * NT, b = blockIdx.y;
    attn_probs<KI>(a, b, n0, l);
    apply<KI>(l.M, a.val + (size_t)b * a.Ck * a.K, a.K, 1, a.K, a.Ck, 1.0f, a.out + (size_t)b * a.Ck * a.N, a.N, n0, a.vec, l.stage);
}

// grid (tiles, B)
template <int KI>
__global__ __launch_bounds__(NTHR) void k_attn_dq(AttnArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Lds l = carve<KI>(lds);
    const int n0 = blockIdx.x * NT, b = blockIdx.y;
    attn_probs<KI>(a, b, n0, l);
    float ds[KI][4];
    attn_dscores<KI>(a, b, n0, l, ds);
    put_own<KI>(l.M, ds);
    apply<KI>(l.M, a.key + (size_t)b * a.Ck * a.K, a.K, 1, a.K, a.Ck, a.s, a.dq + (size_t)b * a.Ck * a.N, a.N, n0, a.vec, l.stage);
}

// partial dval and dkey of one split and one channel chunk.  grid (nsplit, B, chunks)
template <int KI>
__global__ __launch_bounds__(NTHR) void k_attn_dkv(AttnArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Lds l = carve<KI>(lds);
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int split = blockIdx.x, b = blockIdx.y, c0 = blockIdx.z * CH;
    const int Ck = a.Ck, K = a.K, N = a.N;
    float accv[KI][4], acck[KI][4];
#pragma unroll
    for (int i = 0; i < KI; ++i) {
        accv[i][0] = accv[i][1] = accv[i][2] = accv[i][3] = 0.f;
        acck[i][0] = acck[i][1] = acck[i][2] = acck[i][3] = 0.f;
    }
    int first, last;
    split_range(N, a.nsplit, split, &first, &last);
#pragma unroll 1
    for (int tile = first; tile < last; ++tile) {
        const int n0 = tile * NT;
        __syncthreads();                                    // the previous tile's last reduce_n has read M
        attn_probs<KI>(a, b, n0, l);
        float ds[KI][4];
        attn_dscores<KI>(a, b, n0, l, ds);
        reduce_n<KI>(accv, l.M, a.dout + (size_t)b * Ck * N, Ck, c0, N, n0, a.vec, l.stage);
        __syncthreads();
        put_own<KI>(l.M, ds);
        reduce_n<KI>(acck, l.M, a.q + (size_t)b * Ck * N, Ck, c0, N, n0, a.vec, l.stage);
    }
    float *pv = a.part + ((size_t)b * a.nsplit + split) * 2 * Ck * K, *pk = pv + (size_t)Ck * K;
#pragma unroll
    for (int i = 0; i < KI; ++i) {
        const int k = ty + 16 * i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + tx + 16 * j;
            if (k < K && c < Ck) {
                pv[(size_t)c * K + k] = accv[i][j];
                pk[(size_t)c * K + k] = acck[i][j];
            }
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------

int ki_of(int K)
{
    const int need = (K + 15) / 16;
    const int have[] = {1, 2, 4, 8, 10, 16};
    for (int v : have)
        if (need <= v)
            return v;
    return 0;
}

// One instance per kernel (the kernel is a template argument), so that the opt-in to more than 48 KB of LDS is made once per kernel
// and device instead of on every launch of every training step.
template <auto kern, typename Args>
int launch(dim3 grid, size_t lds, hipStream_t st, const Args &a, const char *what)
{
    if (lds > 48 * 1024) {
        static std::atomic<uint64_t> done{0};          // bit d: set for device d
        int d = 0;
        (void)hipGetDevice(&d);
        const uint64_t bit = d >= 0 && d < 64 ? (uint64_t)1 << d : 0;
        if (!(done.load(std::memory_order_relaxed) & bit) || !bit) {
            const hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) {
                dco_set_error("%s: hipFuncSetAttribute(MaxDynamicSharedMemorySize = %d): %s", what, (int)lds, hipGetErrorString(e));
                return (int)e;
            }
            done.fetch_or(bit, std::memory_order_relaxed);
        }
    }
    hipLaunchKernelGGL(kern, grid, dim3(NTHR), lds, st, a);
    return DCO_OK;
}

int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        dco_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return DCO_OK;
}

bool aligned16(std::initializer_list<const void *> ps)
{
    for (const void *p : ps)
        if (!p || (uintptr_t)p % 16 != 0)
            return false;
    return true;
}

int common_args(int op, int B, int C, int K, int N, const void *ws, int64_t ws_bytes, bool tensors_ok, const char *what)
{
    const int64_t need = dco_ws_bytes(op, B, C, K, N);
    if (need < 0) {
        dco_set_error("%s: shape not taken (dco_supported)", what);
        return DCO_EINVAL;
    }
    if (!tensors_ok) {
        dco_set_error("%s: a tensor is null or not 16-byte aligned", what);
        return DCO_EINVAL;
    }
    if (ws_bytes < need) {
        dco_set_error("%s: workspace of %lld bytes, %lld needed", what, (long long)ws_bytes, (long long)need);
        return DCO_EINVAL;
    }
    if (need > 0 && (!ws || (uintptr_t)ws % 256 != 0)) {
        dco_set_error("%s: the workspace must be 256-byte aligned", what);
        return DCO_EINVAL;
    }
    return DCO_OK;
}

}  // namespace

#define DCO_FOR_KI(X) X(1) X(2) X(4) X(8) X(10) X(16)

extern "C" int dco_gather_fwd(const float *x, const float *logits, int B, int C, int K, int N, float scale, void *workspace,
                              int64_t workspace_bytes, float *ctx, float *stats, void *stream)
{
    int rc = common_args(DCO_OP_GATHER_FWD, B, C, K, N, workspace, workspace_bytes, aligned16({x, logits, ctx, stats}), __func__);
    if (rc != DCO_OK)
        return rc;
    hipStream_t st = (hipStream_t)stream;
    GatherArgs a = {};
    a.x = x; a.logits = logits; a.stats = stats; a.part = (float *)workspace;
    a.C = C; a.K = K; a.N = N; a.nsplit = dco_split_count(B, C, N); a.vec = N % 4 == 0; a.scale = scale;
    hipLaunchKernelGGL(k_gather_stats, dim3((unsigned)K, (unsigned)B), dim3(NTHR), 0, st, logits, K, N, scale, stats);
    if ((rc = launched(__func__)) != DCO_OK)
        return rc;
    const dim3 grid((unsigned)a.nsplit, (unsigned)B, (unsigned)dco_chunks(C));
    switch (ki_of(K)) {
#define X(KI_) case KI_: rc = launch<k_gather_fwd<KI_>>(grid, lds_bytes(KI_), st, a, __func__); break;
        DCO_FOR_KI(X)
#undef X
    default: rc = DCO_EINVAL;
    }
    if (rc != DCO_OK || (rc = launched(__func__)) != DCO_OK)
        return rc;
    const int E = K * C;
    hipLaunchKernelGGL(k_sum_splits, dim3((unsigned)((E + NTHR - 1) / NTHR), (unsigned)B), dim3(NTHR), 0, st, (const float *)a.part,
                       (size_t)a.nsplit * E, (size_t)E, a.nsplit, E, 1.0f, ctx);
    return launched(__func__);
}

extern "C" int dco_gather_bwd(const float *x, const float *logits, const float *ctx, const float *stats, const float *dctx, int B,
                              int C, int K, int N, float scale, void *workspace, int64_t workspace_bytes, float *dx, float *dlogits,
                              void *stream)
{
    int rc = common_args(DCO_OP_GATHER_BWD, B, C, K, N, workspace, workspace_bytes,
                         aligned16({x, logits, ctx, stats, dctx, dx, dlogits}), __func__);
    if (rc != DCO_OK)
        return rc;
    hipStream_t st = (hipStream_t)stream;
    GatherArgs a = {};
    a.x = x; a.logits = logits; a.stats = stats; a.dctx = dctx; a.ctx = ctx; a.dx = dx; a.dlogits = dlogits;
    a.C = C; a.K = K; a.N = N; a.vec = N % 4 == 0; a.scale = scale;
    const dim3 grid((unsigned)dco_tiles(N), (unsigned)B);
    switch (ki_of(K)) {
#define X(KI_) case KI_: rc = launch<k_gather_bwd<KI_>>(grid, lds_bytes(KI_), st, a, __func__); break;
        DCO_FOR_KI(X)
#undef X
    default: rc = DCO_EINVAL;
    }
    return rc != DCO_OK ? rc : launched(__func__);
}

extern "C" int dco_attn_fwd(const float *q, const float *key, const float *val, int B, int Ck, int K, int N, float s,
                            void *workspace, int64_t workspace_bytes, float *out, void *stream)
{
    int rc = common_args(DCO_OP_ATTN_FWD, B, Ck, K, N, workspace, workspace_bytes, aligned16({q, key, val, out}), __func__);
    if (rc != DCO_OK)
        return rc;
    hipStream_t st = (hipStream_t)stream;
    AttnArgs a = {};
    a.q = q; a.key = key; a.val = val; a.out = out;
    a.Ck = Ck; a.K = K; a.N = N; a.vec = N % 4 == 0; a.s = s;
    const dim3 grid((unsigned)dco_tiles(N), (unsigned)B);
    switch (ki_of(K)) {
#define X(KI_) case KI_: rc = launch<k_attn_fwd<KI_>>(grid, lds_bytes(KI_), st, a, __func__); break;
        DCO_FOR_KI(X)
#undef X
    default: rc = DCO_EINVAL;
    }
    return rc != DCO_OK ? rc : launched(__func__);
}

extern "C" int dco_attn_bwd(const float *q, const float *key, const float *val, const float *dout, int B, int Ck, int K, int N,
                            float s, void *workspace, int64_t workspace_bytes, float *dq, float *dkey, float *dval, void *stream)
{
    int rc = common_args(DCO_OP_ATTN_BWD, B, Ck, K, N, workspace, workspace_bytes, aligned16({q, key, val, dout, dq, dkey, dval}),
                         __func__);
    if (rc != DCO_OK)
        return rc;
    hipStream_t st = (hipStream_t)stream;
    AttnArgs a = {};
    a.q = q; a.key = key; a.val = val; a.dout = dout; a.dq = dq; a.part = (float *)workspace;
    a.Ck = Ck; a.K = K; a.N = N; a.nsplit = dco_split_count(B, Ck, N); a.vec = N % 4 == 0; a.s = s;
    const dim3 grid((unsigned)dco_tiles(N), (unsigned)B);
    const dim3 grid2((unsigned)a.nsplit, (unsigned)B, (unsigned)dco_chunks(Ck));
    switch (ki_of(K)) {
#define X(KI_)                                                                                \
    case KI_:                                                                                 \
        rc = launch<k_attn_dq<KI_>>(grid, lds_bytes(KI_), st, a, __func__);                   \
        if (rc == DCO_OK && (rc = launched(__func__)) == DCO_OK)                              \
            rc = launch<k_attn_dkv<KI_>>(grid2, lds_bytes(KI_), st, a, __func__);             \
        break;
        DCO_FOR_KI(X)
#undef X
    default: rc = DCO_EINVAL;
    }
    if (rc != DCO_OK || (rc = launched(__func__)) != DCO_OK)
        return rc;
    const int E = Ck * K;
    const dim3 gs((unsigned)((E + NTHR - 1) / NTHR), (unsigned)B);
    hipLaunchKernelGGL(k_sum_splits, gs, dim3(NTHR), 0, st, (const float *)a.part, (size_t)a.nsplit * 2 * E, (size_t)2 * E,
                       a.nsplit, E, 1.0f, dval);
    if ((rc = launched(__func__)) != DCO_OK)
        return rc;
    hipLaunchKernelGGL(k_sum_splits, gs, dim3(NTHR), 0, st, (const float *)a.part + E, (size_t)a.nsplit * 2 * E, (size_t)2 * E,
                       a.nsplit, E, s, dkey);
    return launched(__func__);
}
