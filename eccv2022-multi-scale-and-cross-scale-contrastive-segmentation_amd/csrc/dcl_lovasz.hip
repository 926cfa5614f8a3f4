// dcl_lovasz.hip -- Lovasz-Softmax loss for gfx950 (include/dcl_lovasz.h): keys, segmented LSD radix sort, scan + term,
// coefficients, backward.  Every kernel works on TILES of DLV_TILE consecutive elements of ONE segment (a tile never
// crosses a segment boundary: a short segment is a short tile), so a segment may span thousands of workgroups or be one
// pixel long with the same code.  Integer counts everywhere the order of a sum could matter; the float sums are fp64
// partials added in a fixed order.
#include <hip/hip_runtime.h>
#include <math.h>

#include "dcl_lovasz_plan.h"

#define LV_THREADS 256
#define LV_WAVES 4
#define LV_ITEMS (DLV_TILE / LV_THREADS)          // 16 elements per thread
#define LV_WAVE_SPAN (DLV_TILE / LV_WAVES)        // 1024 consecutive elements per wave
#define LV_KEY_ONE 0x3F800000u                    // bits of 1.0f: key = LV_KEY_ONE - bits(e), ascending key = descending e
#define LV_FG 0x80000000u                         // payload = position in the segment | LV_FG where the pixel is foreground
#define LV_PASSES 4

static_assert(LV_THREADS == DLV_RADIX, "one thread per digit");

#define DLV_LAUNCH_CHECK()                                                            \
    do {                                                                              \
        hipError_t e_ = hipGetLastError();                                            \
        if (e_ != hipSuccess) {                                                       \
            dlv_set_error("%s: launch failed: %s", __func__, hipGetErrorString(e_));  \
            return (int)e_;                                                           \
        }                                                                             \
    } while (0)

__device__ inline long long lv_label(const void *p, int bytes, size_t i)
{
    if (bytes == 8)
        return ((const long long *)p)[i];
    if (bytes == 4)
        return ((const int *)p)[i];
    return ((const unsigned char *)p)[i];
}

// inclusive scan over the 256 threads of a workgroup; *total = the sum.  wsum: LDS, LV_WAVES words.
__device__ inline uint32_t lv_block_scan(uint32_t v, uint32_t *wsum, uint32_t *total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        uint32_t u = __shfl_up(v, o, 64);
        if (lane >= o)
            v += u;
    }
    if (lane == 63)
        wsum[w] = v;
    __syncthreads();
    uint32_t add = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < LV_WAVES; ++i) {
        uint32_t s = wsum[i];
        add += i < w ? s : 0u;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return v + add;
}

// sum of one double per thread in a fixed order (butterfly inside the wave, then wave 0..3); valid in thread 0
__device__ inline double lv_block_sum(double v, double *wsum)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0)
        wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < LV_WAVES; ++i)
            s += wsum[i];
    __syncthreads();
    return s;
}

// ---- 1. keys --------------------------------------------------------------------------------------------------------
// One thread per pixel: softmax over C (exp in fp32, the denominator in fp64), then for every class the key
// (LV_KEY_ONE - bits of e) and the payload at the pixel's place in the class's segment.  Foreground totals: a histogram
// of the workgroup's labels in LDS, then one integer atomic per class and workgroup.
__global__ __launch_bounds__(LV_THREADS) void k_dlv_keys(const float *__restrict__ logits, const void *__restrict__ labels,
                                                         int label_bytes, int N, int C, int HW, int bpi, int per_image,
                                                         int has_ignore, int ignore, uint32_t *__restrict__ key,
                                                         uint32_t *__restrict__ pay, uint32_t *__restrict__ G)
{
    __shared__ uint32_t bins[DLV_RADIX];
    const int t = threadIdx.x;
    const int n = blockIdx.x / bpi, x = (blockIdx.x % bpi) * LV_THREADS + t;
    bins[t] = 0;
    __syncthreads();
    if (x < HW) {
        const float *lp = logits + (size_t)n * C * HW + x;
        float m = -INFINITY;
        for (int k = 0; k < C; ++k)
            m = fmaxf(m, lp[(size_t)k * HW]);
        double s = 0.0;
        for (int k = 0; k < C; ++k)
            s += (double)expf(lp[(size_t)k * HW] - m);
        const double inv = 1.0 / s;
        const long long lab = lv_label(labels, label_bytes, (size_t)n * HW + x);
        const bool valid = !(has_ignore && lab == (long long)ignore);
        const uint32_t pos = per_image ? (uint32_t)x : (uint32_t)n * (uint32_t)HW + (uint32_t)x;
        for (int k = 0; k < C; ++k) {
            float p = (float)((double)expf(lp[(size_t)k * HW] - m) * inv);
            bool fg = valid && lab == (long long)k;
            float e = valid ? fabsf((fg ? 1.0f : 0.0f) - p) : 0.0f;
            size_t o = per_image ? ((size_t)n * C + k) * HW + x : ((size_t)k * N + n) * HW + x;
            key[o] = LV_KEY_ONE - __float_as_uint(e);
            pay[o] = pos | (fg ? LV_FG : 0u);
        }
        if (valid && lab >= 0 && lab < (long long)C)
            atomicAdd(&bins[(int)lab], 1u);
    }
    __syncthreads();
    if (t < C && bins[t])
        atomicAdd(&G[per_image ? n * C + t : t], bins[t]);
}

// ---- weights of the terms: 1 / (terms of the group * groups) for a class that gives a term, 0 otherwise ----------------
__global__ __launch_bounds__(LV_THREADS) void k_dlv_plan(const uint32_t *__restrict__ G, const uint8_t *__restrict__ consider,
                                                         int C, int groups, int present_only, double *__restrict__ scale)
{
    const int k = threadIdx.x;
    for (int g = 0; g < groups; ++g) {
        int inc = 0;
        if (k < C)
            inc = (consider == nullptr || consider[k] != 0) && (!present_only || G[g * C + k] > 0);
        int terms = __syncthreads_count(inc);
        if (k < C)
            scale[g * C + k] = inc ? 1.0 / ((double)terms * (double)groups) : 0.0;
    }
}

// ---- 2. radix sort: digit histogram of every tile, hist[segment][digit][tile] ------------------------------------------
__global__ __launch_bounds__(LV_THREADS) void k_dlv_hist(const uint32_t *__restrict__ key, uint32_t *__restrict__ hist,
                                                         long long L, int tps, int shift)
{
    __shared__ uint32_t bins[DLV_RADIX];
    const int t = threadIdx.x;
    const int tile = blockIdx.x % tps;
    const long long seg = blockIdx.x / tps;
    const long long start = (long long)tile * DLV_TILE;
    const int n = (int)min((long long)DLV_TILE, L - start);
    const uint32_t *kp = key + seg * L + start;
    bins[t] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < LV_ITEMS; ++r) {
        int j = r * LV_THREADS + t;
        if (j < n)
            atomicAdd(&bins[(kp[j] >> shift) & (DLV_RADIX - 1)], 1u);
    }
    __syncthreads();
    hist[((size_t)seg * DLV_RADIX + t) * tps + tile] = bins[t];
}

// exclusive scan of every row of data[rows][len] in place; totals[row] = the row's sum (totals may be null)
__global__ __launch_bounds__(LV_THREADS) void k_dlv_rowscan(uint32_t *__restrict__ data, int len, uint32_t *__restrict__ totals)
{
    __shared__ uint32_t wsum[LV_WAVES];
    uint32_t *row = data + (size_t)blockIdx.x * len;
    uint32_t carry = 0;
    for (int c0 = 0; c0 < len; c0 += LV_THREADS) {
        const int i = c0 + threadIdx.x;
        uint32_t v = i < len ? row[i] : 0u, total;
        uint32_t incl = lv_block_scan(v, wsum, &total);
        if (i < len)
            row[i] = carry + incl - v;
        carry += total;
    }
    if (totals != nullptr && threadIdx.x == 0)
        totals[blockIdx.x] = carry;
}

// One pass of the sort for one tile.  Element order inside the tile: wave w holds elements [1024 w, 1024 (w + 1)), item r
// of lane l is element 1024 w + 64 r + l, so (wave, item, lane) is the tile's order and the rank below is stable:
//   rank in the tile = (elements of smaller digits) + (same digit in earlier waves) + (same digit earlier in this wave).
// The last comes from wave ballots: the lanes that hold the same digit find each other bit by bit, the first of them
// advances the wave's counter.  The tile is then laid out in rank order in LDS so that consecutive lanes write
// consecutive addresses of one digit's run.
__global__ __launch_bounds__(LV_THREADS) void k_dlv_scatter(const uint32_t *__restrict__ kin, const uint32_t *__restrict__ pin,
                                                            uint32_t *__restrict__ kout, uint32_t *__restrict__ pout,
                                                            const uint32_t *__restrict__ hist, const uint32_t *__restrict__ tot,
                                                            long long L, int tps, int shift)
{
    __shared__ uint32_t sk[DLV_TILE], sp[DLV_TILE];
    __shared__ uint32_t cnt[LV_WAVES * DLV_RADIX];
    __shared__ uint32_t tile_ex[DLV_RADIX];
    __shared__ long long rel[DLV_RADIX];
    __shared__ uint32_t wsum[LV_WAVES];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int tile = blockIdx.x % tps;
    const long long seg = blockIdx.x / tps;
    const long long start = (long long)tile * DLV_TILE;
    const int n = (int)min((long long)DLV_TILE, L - start);
    const size_t segbase = (size_t)seg * L, base = segbase + start;

    uint32_t key[LV_ITEMS], pay[LV_ITEMS], loc[LV_ITEMS];
#pragma unroll
    for (int r = 0; r < LV_ITEMS; ++r) {
        int j = w * LV_WAVE_SPAN + r * 64 + lane;
        key[r] = j < n ? kin[base + j] : 0u;
        pay[r] = j < n ? pin[base + j] : 0u;
    }
#pragma unroll
    for (int i = 0; i < LV_WAVES; ++i)
        cnt[i * DLV_RADIX + t] = 0;
    __syncthreads();

    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < LV_ITEMS; ++r) {
        const bool valid = w * LV_WAVE_SPAN + r * 64 + lane < n;
        const uint32_t d = (key[r] >> shift) & (DLV_RADIX - 1);
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            unsigned long long bb = __ballot(valid && bit);
            same &= bit ? bb : ~bb;
        }
        const uint32_t pre = cnt[w * DLV_RADIX + d];
        const uint32_t rank = __popcll(same & below);
        __builtin_amdgcn_wave_barrier();
        if (valid && rank == 0)
            cnt[w * DLV_RADIX + d] = pre + __popcll(same);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        loc[r] = pre + rank;
    }
    __syncthreads();

    {   // thread t = digit t
        uint32_t c0 = cnt[t], c1 = cnt[DLV_RADIX + t], c2 = cnt[2 * DLV_RADIX + t], c3 = cnt[3 * DLV_RADIX + t];
        uint32_t mine = c0 + c1 + c2 + c3, total;
        cnt[t] = 0;
        cnt[DLV_RADIX + t] = c0;
        cnt[2 * DLV_RADIX + t] = c0 + c1;
        cnt[3 * DLV_RADIX + t] = c0 + c1 + c2;
        uint32_t ex = lv_block_scan(mine, wsum, &total) - mine;
        tile_ex[t] = ex;
        uint32_t segtot = tot[(size_t)seg * DLV_RADIX + t];
        uint32_t digit_base = lv_block_scan(segtot, wsum, &total) - segtot;
        rel[t] = (long long)digit_base + (long long)hist[((size_t)seg * DLV_RADIX + t) * tps + tile] - (long long)ex;
    }
    __syncthreads();

#pragma unroll
    for (int r = 0; r < LV_ITEMS; ++r) {
        if (w * LV_WAVE_SPAN + r * 64 + lane < n) {
            const uint32_t d = (key[r] >> shift) & (DLV_RADIX - 1);
            const uint32_t p = tile_ex[d] + cnt[w * DLV_RADIX + d] + loc[r];
            if (p < (uint32_t)DLV_TILE) {
                sk[p] = key[r];
                sp[p] = pay[r];
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < LV_ITEMS; ++r) {
        const int p = r * LV_THREADS + t;
        if (p < n) {
            const uint32_t k = sk[p];
            const long long o = rel[(k >> shift) & (DLV_RADIX - 1)] + p;
            if (o >= 0 && o < L) {      // always true for histograms of these keys; keeps a store inside the segment regardless
                kout[segbase + o] = k;
                pout[segbase + o] = sp[p];
            }
        }
    }
}

// ---- 3. scan + term ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LV_THREADS) void k_dlv_fgcount(const uint32_t *__restrict__ pay, uint32_t *__restrict__ fgt,
                                                            long long L, int tps)
{
    const int t = threadIdx.x;
    const int tile = blockIdx.x % tps;
    const long long seg = blockIdx.x / tps;
    const long long start = (long long)tile * DLV_TILE;
    const int n = (int)min((long long)DLV_TILE, L - start);
    const uint32_t *pp = pay + seg * L + start;
    int c = 0;
#pragma unroll
    for (int r = 0; r < LV_ITEMS; ++r) {
        int j = r * LV_THREADS + t;
        c += (j < n && (pp[j] & LV_FG)) ? 1 : 0;
    }
    // counts of the 256 threads: an integer sum, any order gives the same
    __shared__ uint32_t total;
    if (t == 0)
        total = 0;
    __syncthreads();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        c += __shfl_xor(c, o, 64);
    if ((t & 63) == 0)
        atomicAdd(&total, (uint32_t)c);
    __syncthreads();
    if (t == 0)
        fgt[(size_t)seg * tps + tile] = total;
}

// For sorted position i of a segment with G foreground pixels and cum = foreground among positions 0..i:
//   I = G - cum, U = G + (i + 1 - cum), J_i = 1 - I / U, step g_i = J_i - J_{i-1} without the subtraction:
//   foreground: 1 / U_i      background: I / (U_{i-1} U_i) with U_{i-1} = U_i - 1      i = 0: J_0 = (U - I) / U = 1 / U_0.
// All integers are exact in fp64 (U^2 < 2^64 is not needed: the quotient is taken as (I / U_{i-1}) / U_i).
__global__ __launch_bounds__(LV_THREADS) void k_dlv_apply(const uint32_t *__restrict__ key, const uint32_t *__restrict__ pay,
                                                          const uint32_t *__restrict__ fgt, const uint32_t *__restrict__ G,
                                                          const double *__restrict__ scale, long long L, int tps, int per_image,
                                                          int C, int HW, float *__restrict__ coef, double *__restrict__ part)
{
    __shared__ uint32_t wcount[LV_WAVES];
    __shared__ double wsum[LV_WAVES];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int tile = blockIdx.x % tps;
    const long long seg = blockIdx.x / tps;
    const long long start = (long long)tile * DLV_TILE;
    const int n = (int)min((long long)DLV_TILE, L - start);
    const size_t base = (size_t)seg * L + start;

    uint32_t kk[LV_ITEMS], pp[LV_ITEMS];
    uint32_t mine = 0;
#pragma unroll
    for (int r = 0; r < LV_ITEMS; ++r) {
        int j = w * LV_WAVE_SPAN + r * 64 + lane;
        kk[r] = j < n ? key[base + j] : LV_KEY_ONE;
        pp[r] = j < n ? pay[base + j] : 0u;
        mine += __popcll(__ballot((pp[r] & LV_FG) != 0));
    }
    if (lane == 0)
        wcount[w] = mine;
    __syncthreads();
    uint32_t cum0 = fgt[(size_t)seg * tps + tile];        // foreground in the segment's earlier tiles
    for (int i = 0; i < w; ++i)
        cum0 += wcount[i];

    const double Gd = (double)G[seg];
    const double sc = scale[seg];
    const unsigned long long upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
    double term = 0.0;
#pragma unroll
    for (int r = 0; r < LV_ITEMS; ++r) {
        const int j = w * LV_WAVE_SPAN + r * 64 + lane;
        const bool fg = (pp[r] & LV_FG) != 0;
        const unsigned long long b = __ballot(fg);
        const uint32_t cum = cum0 + __popcll(b & upto);
        cum0 += __popcll(b);
        if (j < n) {
            const long long i = start + j;
            const double I = Gd - (double)cum;
            const double U = Gd + (double)(i + 1 - (long long)cum);
            const double g = (fg || i == 0) ? 1.0 / U : (I / (U - 1.0)) / U;
            const float e = __uint_as_float(LV_KEY_ONE - kk[r]);
            term += (double)e * g;
            const float c = e != 0.0f ? (float)((fg ? -g : g) * sc) : 0.0f;
            const long long q = pp[r] & ~LV_FG;
            if (q < L) {
                size_t o = per_image ? (size_t)seg * L + q : ((size_t)(q / HW) * C + seg) * HW + (size_t)(q % HW);
                coef[o] = c;
            }
        }
    }
    double s = lv_block_sum(term, wsum);
    if (t == 0)
        part[(size_t)seg * tps + tile] = s;
}

__global__ __launch_bounds__(LV_THREADS) void k_dlv_segsum(const double *__restrict__ part, const double *__restrict__ scale,
                                                           int tps, double *__restrict__ segterm)
{
    __shared__ double wsum[LV_WAVES];
    const double *row = part + (size_t)blockIdx.x * tps;
    double v = 0.0;
    for (int i = threadIdx.x; i < tps; i += LV_THREADS)
        v += row[i];
    double s = lv_block_sum(v, wsum);
    if (threadIdx.x == 0)
        segterm[blockIdx.x] = s * scale[blockIdx.x];
}

__global__ __launch_bounds__(LV_THREADS) void k_dlv_final(const double *__restrict__ segterm, long long S, float *__restrict__ loss)
{
    __shared__ double wsum[LV_WAVES];
    double v = 0.0;
    for (long long i = threadIdx.x; i < S; i += LV_THREADS)
        v += segterm[i];
    double s = lv_block_sum(v, wsum);
    if (threadIdx.x == 0)
        loss[0] = (float)s;
}

// ---- 4. backward -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LV_THREADS) void k_dlv_bwd(const float *__restrict__ logits, const float *__restrict__ coef,
                                                        const float *__restrict__ upstream, int C, int HW, int bpi,
                                                        float *__restrict__ dlogits)
{
    const int n = blockIdx.x / bpi, x = (blockIdx.x % bpi) * LV_THREADS + threadIdx.x;
    if (x >= HW)
        return;
    const size_t off = (size_t)n * C * HW + x;
    const float *lp = logits + off, *cp = coef + off;
    float *dp = dlogits + off;
    float m = -INFINITY;
    for (int k = 0; k < C; ++k)
        m = fmaxf(m, lp[(size_t)k * HW]);
    double s = 0.0;
    for (int k = 0; k < C; ++k)
        s += (double)expf(lp[(size_t)k * HW] - m);
    const double inv = 1.0 / s;
    double dot = 0.0;
    for (int k = 0; k < C; ++k)
        dot += (double)cp[(size_t)k * HW] * ((double)expf(lp[(size_t)k * HW] - m) * inv);
    const double up = (double)upstream[0];
    for (int k = 0; k < C; ++k) {
        double p = (double)expf(lp[(size_t)k * HW] - m) * inv;
        dp[(size_t)k * HW] = (float)(up * p * ((double)cp[(size_t)k * HW] - dot));
    }
}

// ---- entries -----------------------------------------------------------------------------------------------------------
extern "C" int dlv_lovasz_fwd(const float *logits, const void *labels, int label_bytes, int N, int C, int HW, int per_image,
                              int has_ignore, int ignore, int present_only, const uint8_t *consider, void *workspace,
                              int64_t workspace_bytes, float *coef, float *loss, void *stream)
{
    DlvLayout lay;
    DLV_CHECK_ARG(dlv_layout(N, C, HW, per_image, &lay), "need 1 <= C <= 256, N, HW >= 1, N*C*HW < 2^31");
    DLV_CHECK_ARG(label_bytes == 8 || label_bytes == 4 || label_bytes == 1, "labels are int64, int32 or uint8");
    DLV_CHECK_ARG(logits && labels && workspace && coef && loss, "null pointer");
    DLV_CHECK_ARG(workspace_bytes >= lay.bytes, "workspace smaller than dlv_workspace_bytes");
    DLV_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
    DLV_CHECK_ARG(lay.S * lay.tps * DLV_RADIX < (1ll << 31), "too many tiles");
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    uint32_t *key[2] = {(uint32_t *)(ws + lay.key[0]), (uint32_t *)(ws + lay.key[1])};
    uint32_t *pay[2] = {(uint32_t *)(ws + lay.pay[0]), (uint32_t *)(ws + lay.pay[1])};
    uint32_t *hist = (uint32_t *)(ws + lay.hist), *tot = (uint32_t *)(ws + lay.tot), *fgt = (uint32_t *)(ws + lay.fgt);
    uint32_t *G = (uint32_t *)(ws + lay.G);
    double *part = (double *)(ws + lay.part), *scale = (double *)(ws + lay.scale), *segterm = (double *)(ws + lay.segterm);
    const int tps = (int)lay.tps, bpi = (HW + LV_THREADS - 1) / LV_THREADS;
    const unsigned tiles = (unsigned)(lay.S * lay.tps);

    hipError_t e = hipMemsetAsync(G, 0, sizeof(uint32_t) * lay.S, s);
    if (e != hipSuccess) {
        dlv_set_error("%s: memset failed: %s", __func__, hipGetErrorString(e));
        return (int)e;
    }
    k_dlv_keys<<<(unsigned)N * bpi, LV_THREADS, 0, s>>>(logits, labels, label_bytes, N, C, HW, bpi, per_image, has_ignore,
                                                        ignore, key[0], pay[0], G);
    k_dlv_plan<<<1, LV_THREADS, 0, s>>>(G, consider, C, per_image ? N : 1, present_only, scale);
    for (int p = 0; p < LV_PASSES; ++p) {
        const int a = p & 1, b = a ^ 1;
        k_dlv_hist<<<tiles, LV_THREADS, 0, s>>>(key[a], hist, lay.L, tps, 8 * p);
        k_dlv_rowscan<<<(unsigned)(lay.S * DLV_RADIX), LV_THREADS, 0, s>>>(hist, tps, tot);
        k_dlv_scatter<<<tiles, LV_THREADS, 0, s>>>(key[a], pay[a], key[b], pay[b], hist, tot, lay.L, tps, 8 * p);
    }
    static_assert(LV_PASSES % 2 == 0, "the sorted order ends in buffer 0");
    k_dlv_fgcount<<<tiles, LV_THREADS, 0, s>>>(pay[0], fgt, lay.L, tps);
    k_dlv_rowscan<<<(unsigned)lay.S, LV_THREADS, 0, s>>>(fgt, tps, nullptr);
    k_dlv_apply<<<tiles, LV_THREADS, 0, s>>>(key[0], pay[0], fgt, G, scale, lay.L, tps, per_image, C, HW, coef, part);
    k_dlv_segsum<<<(unsigned)lay.S, LV_THREADS, 0, s>>>(part, scale, tps, segterm);
    k_dlv_final<<<1, LV_THREADS, 0, s>>>(segterm, lay.S, loss);
    DLV_LAUNCH_CHECK();
    return DLV_OK;
}

extern "C" int dlv_lovasz_bwd(const float *logits, const float *coef, const float *upstream, int N, int C, int HW,
                              float *dlogits, void *stream)
{
    DlvLayout lay;
    DLV_CHECK_ARG(dlv_layout(N, C, HW, 0, &lay), "need 1 <= C <= 256, N, HW >= 1, N*C*HW < 2^31");
    DLV_CHECK_ARG(logits && coef && upstream && dlogits, "null pointer");
    const int bpi = (HW + LV_THREADS - 1) / LV_THREADS;
    k_dlv_bwd<<<(unsigned)N * bpi, LV_THREADS, 0, (hipStream_t)stream>>>(logits, coef, upstream, C, HW, bpi, dlogits);
    DLV_LAUNCH_CHECK();
    return DLV_OK;
}
