// dcl_ohem.hip -- online hard example mining for the pixel-wise cross-entropy (C ABI: include/dcl_ohem.h).
//
// The torch form of the public HRNet OhemCrossEntropy writes the full-resolution logits (478 MB for 12 x 19 x 512 x 1024), takes a
// softmax over them, sorts 6.3 million probabilities and indexes with boolean masks (a host synchronisation each).  Here:
//   k_doh_target_prob : one thread per output pixel: the four taps of the TARGET class only (dcl_bilinear.h), p = exp(z_t - lse),
//                   l = w_t (lse - z_t) with lse from dcl_upsample_ce_fwd; counts the valid pixels; histogram of the first digit
//   k_doh_pick        : one workgroup: scans a histogram, fixes the digit and the rank inside it (dcl_ohem_plan.h: the same function the
//                   host test runs against a sorted array); the last one writes v and thr = max(v, thresh)
//   k_doh_hist        : the histogram of the next digit over the keys that match the digits fixed so far (read from device memory)
//   k_doh_reduce      : one workgroup per row: kept = p < thr, the hard-target map for dcl_upsample_ce_bwd, {sum l, count} per row
//   k_doh_finish      : one workgroup: the rows summed in double, loss = sum / max(m, 1)
// Exact selection in three passes over 4 bytes per pixel instead of a sort; the host never learns n, k, v or m.
// Histograms are built per workgroup in LDS and flushed with integer atomics (the only atomics here).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcl_bilinear.h"
#include "dcl_ohem_plan.h"

namespace {

constexpr int NTHR = 256;
constexpr int PIX_PER_BLOCK = NTHR * 8;        // pixels a workgroup of k_doh_target_prob / k_doh_hist walks (8 coalesced trips)

struct Axis {
    float scale;
    int align;
};

struct ProbArgs {
    const float *z;             // [N, C, h, w]
    const long long *target;    // [N, H, W]
    const float *weight;        // [C] or null
    const float *lse;           // [N, H, W]
    float *p, *l;               // [N, H, W]
    uint32_t *ws;
    int N, C, h, w, H, W, ignore;
    Axis ay, ax;
};

__global__ __launch_bounds__(NTHR) void k_doh_clear(uint32_t *ws, int words)
{
    const int i = blockIdx.x * NTHR + threadIdx.x;
    if (i < words)
        ws[i] = 0u;
}

// flush an LDS histogram: the non-empty bins only (a pass of the select fills a few)
__device__ __forceinline__ void flush_hist(const uint32_t *sh, uint32_t *dst, int bins)
{
    for (int b = threadIdx.x; b < bins; b += NTHR) {
        const uint32_t c = sh[b];
        if (c)
            atomicAdd(dst + b, c);
    }
}

__global__ __launch_bounds__(NTHR) void k_doh_target_prob(ProbArgs a)
{
    __shared__ uint32_t sh[DOH_MAX_BINS];
    __shared__ uint32_t cnt[NTHR / 64];
    for (int b = threadIdx.x; b < DOH_MAX_BINS; b += NTHR)
        sh[b] = 0u;
    __syncthreads();
    const size_t total = (size_t)a.N * a.H * a.W;
    const size_t plane = (size_t)a.h * a.w;
    const size_t base = (size_t)blockIdx.x * PIX_PER_BLOCK;
    uint32_t valid_here = 0;
    for (int trip = 0; trip < PIX_PER_BLOCK / NTHR; ++trip) {
        const size_t i = base + (size_t)trip * NTHR + threadIdx.x;
        if (i >= total)
            break;
        const int ox = (int)(i % a.W);
        const size_t row = i / a.W;
        const int oy = (int)(row % a.H), n = (int)(row / a.H);
        const long long t = a.target[i];
        uint32_t bits = DOH_INVALID_BITS;
        float l = 0.f;
        if (t >= 0 && t < a.C && t != a.ignore) {
            int y0, y1, x0, x1;
            float ly0, ly1, lx0, lx1;
            dcl_bilinear_src_index(a.ay.scale, a.ay.align, oy, a.h, &y0, &y1, &ly0, &ly1);
            dcl_bilinear_src_index(a.ax.scale, a.ax.align, ox, a.w, &x0, &x1, &lx0, &lx1);
            const float *zc = a.z + ((size_t)n * a.C + (size_t)t) * plane;
            const float *r0 = zc + (size_t)y0 * a.w, *r1 = zc + (size_t)y1 * a.w;
            const float zt = ly0 * (lx0 * r0[x0] + lx1 * r0[x1]) + ly1 * (lx0 * r1[x0] + lx1 * r1[x1]);
            const float lse = a.lse[i];
            const float wt = a.weight ? a.weight[t] : 1.f;
            l = wt * (lse - zt);
            bits = doh_canonical_bits(__float_as_uint(expf(zt - lse)));
            if (bits >> 31)                      // a negative p cannot occur; were it to, it is the smallest key
                bits = 0u;
            atomicAdd(&sh[doh_digit(bits, 0)], 1u);
            ++valid_here;
        }
        a.p[i] = __uint_as_float(bits);
        a.l[i] = l;
    }
    // the count of valid pixels: lanes -> wave -> workgroup -> one atomic
    for (int o = 32; o > 0; o >>= 1)
        valid_here += __shfl_xor(valid_here, o, 64);
    if ((threadIdx.x & 63) == 0)
        cnt[threadIdx.x >> 6] = valid_here;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t c = (cnt[0] + cnt[1]) + (cnt[2] + cnt[3]);
        if (c)
            atomicAdd(a.ws + DOH_WS_STATE + DOH_ST_N, c);
    }
    flush_hist(sh, a.ws + DOH_WS_HIST0, doh_bins(0));
}

// histogram of digit `pass` (1 or 2) over the keys whose higher digits are the state's prefix
__global__ __launch_bounds__(NTHR) void k_doh_hist(const uint32_t *__restrict__ keys, size_t total, uint32_t *ws, int pass)
{
    __shared__ uint32_t sh[DOH_MAX_BINS];
    const int bins = doh_bins(pass);
    for (int b = threadIdx.x; b < bins; b += NTHR)
        sh[b] = 0u;
    __syncthreads();
    const uint32_t prefix = ws[DOH_WS_STATE + DOH_ST_PREFIX];
    if (ws[DOH_WS_STATE + DOH_ST_EMPTY])             // uniform: no valid pixel, nothing to count
        return;
    const size_t base = (size_t)blockIdx.x * PIX_PER_BLOCK;
    for (int trip = 0; trip < PIX_PER_BLOCK / NTHR; ++trip) {
        const size_t i = base + (size_t)trip * NTHR + threadIdx.x;
        if (i >= total)
            break;
        const uint32_t key = keys[i];
        if ((key >> 31) == 0 && doh_prefix_match(key, prefix, pass))
            atomicAdd(&sh[doh_digit(key, pass)], 1u);
    }
    __syncthreads();
    flush_hist(sh, ws + doh_ws_hist(pass), bins);
}

// one workgroup: fix the digit of `pass`; pass 0 forms k from the counted n, the last pass writes v and thr
__global__ __launch_bounds__(NTHR) void k_doh_pick(uint32_t *ws, int pass, int min_kept, float thresh)
{
    __shared__ uint32_t sh[DOH_MAX_BINS];
    __shared__ uint32_t sums[DOH_CHUNKS];
    const int bins = doh_bins(pass);
    const uint32_t *hist = ws + doh_ws_hist(pass);
    uint32_t *st = ws + DOH_WS_STATE;
    for (int b = threadIdx.x; b < bins; b += NTHR)
        sh[b] = hist[b];
    __syncthreads();
    sums[threadIdx.x] = doh_chunk_sum(sh, bins / DOH_CHUNKS, threadIdx.x);
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    uint32_t prefix = 0u, rank = 0u, empty = 0u;
    if (pass == 0) {
        const uint32_t n = st[DOH_ST_N];
        empty = n == 0u ? 1u : 0u;
        rank = empty ? 0u : doh_rank(min_kept, n);
        st[DOH_ST_K] = rank;
        st[DOH_ST_EMPTY] = empty;
    } else {
        prefix = st[DOH_ST_PREFIX];
        rank = st[DOH_ST_RANK];
        empty = st[DOH_ST_EMPTY];
    }
    uint32_t rem = 0u;
    const int b = empty ? -1 : doh_pick_two_level(sh, sums, bins, rank, &rem);
    // b < 0 with valid pixels cannot occur (the rank is below the count of the bin it came from); the prefix then stays as it is
    if (b >= 0)
        prefix = doh_with_digit(prefix, pass, (uint32_t)b);
    st[DOH_ST_PREFIX] = prefix;
    st[DOH_ST_RANK] = rem;
    if (pass == DOH_PASSES - 1) {
        const float v = __uint_as_float(prefix);
        st[DOH_ST_V] = prefix;
        st[DOH_ST_THR] = __float_as_uint(fmaxf(v, thresh));         // a NaN v (non-finite logits) gives thresh
    }
}

__global__ __launch_bounds__(NTHR) void k_doh_reduce(const float *__restrict__ p, const float *__restrict__ l,
                                                 const long long *__restrict__ target, int W, long long ignore, uint32_t *ws,
                                                 long long *__restrict__ hard, unsigned char *__restrict__ kept8)
{
    __shared__ float ssum[NTHR];
    __shared__ uint32_t scnt[NTHR];
    const size_t row = blockIdx.x;
    const float thr = __uint_as_float(ws[DOH_WS_STATE + DOH_ST_THR]);
    float s = 0.f;
    uint32_t c = 0u;
    for (int x = threadIdx.x; x < W; x += NTHR) {
        const size_t i = row * W + x;
        const bool kept = p[i] < thr;                 // an invalid pixel's p is a NaN pattern: false
        hard[i] = kept ? target[i] : ignore;
        if (kept8)
            kept8[i] = kept ? 1 : 0;
        s += kept ? l[i] : 0.f;
        c += kept ? 1u : 0u;
    }
    ssum[threadIdx.x] = s;
    scnt[threadIdx.x] = c;
    __syncthreads();
    for (int o = NTHR / 2; o > 0; o >>= 1) {          // a fixed tree
        if (threadIdx.x < o) {
            ssum[threadIdx.x] += ssum[threadIdx.x + o];
            scnt[threadIdx.x] += scnt[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        ws[DOH_WS_PART + 2 * row] = __float_as_uint(ssum[0]);
        ws[DOH_WS_PART + 2 * row + 1] = scnt[0];
    }
}

__global__ __launch_bounds__(NTHR) void k_doh_finish(const uint32_t *__restrict__ ws, int rows, uint32_t *__restrict__ res)
{
    __shared__ double ssum[NTHR];
    __shared__ uint32_t scnt[NTHR];
    double s = 0.0;
    uint32_t c = 0u;
    for (int r = threadIdx.x; r < rows; r += NTHR) {
        s += (double)__uint_as_float(ws[DOH_WS_PART + 2 * (size_t)r]);
        c += ws[DOH_WS_PART + 2 * (size_t)r + 1];
    }
    ssum[threadIdx.x] = s;
    scnt[threadIdx.x] = c;
    __syncthreads();
    for (int o = NTHR / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            ssum[threadIdx.x] += ssum[threadIdx.x + o];
            scnt[threadIdx.x] += scnt[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint32_t *st = ws + DOH_WS_STATE;
        const uint32_t m = scnt[0];
        const double denom = m > 0u ? (double)m : 1.0;
        res[DOH_RES_LOSS] = __float_as_uint((float)(ssum[0] / denom));
        res[DOH_RES_DENOM] = __float_as_uint((float)denom);
        res[DOH_RES_V] = st[DOH_ST_V];
        res[DOH_RES_THR] = st[DOH_ST_THR];
        res[DOH_RES_N] = st[DOH_ST_N];
        res[DOH_RES_M] = m;
        res[DOH_RES_K] = st[DOH_ST_K];
        res[DOH_RES_EMPTY] = st[DOH_ST_EMPTY];
    }
}

Axis make_axis(int in_size, int out_size, int align)
{
    Axis a;
    a.align = align;
    a.scale = dcl_bilinear_scale(in_size, out_size, align);
    return a;
}

int launch_failed(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        return 0;
    doh_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return (int)e;
}

unsigned pixel_blocks(int64_t total) { return (unsigned)((total + PIX_PER_BLOCK - 1) / PIX_PER_BLOCK); }

}  // namespace

extern "C" int doh_target_prob(const float *z, int N, int C, int h, int w, int H, int W, int align_corners, const int64_t *target,
                               const float *weight, int ignore_index, const float *lse, float *p, float *l, void *workspace,
                               void *stream)
{
    if (!doh_shape_ok(N, C, h, w, H, W)) {
        doh_set_error("doh_target_prob: shape not taken (doh_supported)");
        return DOH_EINVAL;
    }
    if (!z || !target || !lse || !p || !l || !workspace) {
        doh_set_error("doh_target_prob: a tensor is null");
        return DOH_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    uint32_t *ws = (uint32_t *)workspace;
    hipLaunchKernelGGL(k_doh_clear, dim3((DOH_WS_CLEAR + NTHR - 1) / NTHR), dim3(NTHR), 0, st, ws, DOH_WS_CLEAR);
    if (int rc = launch_failed("doh_target_prob (clear)"))
        return rc;
    ProbArgs a = {};
    a.z = z; a.target = (const long long *)target; a.weight = weight; a.lse = lse; a.p = p; a.l = l; a.ws = ws;
    a.N = N; a.C = C; a.h = h; a.w = w; a.H = H; a.W = W; a.ignore = ignore_index;
    a.ay = make_axis(h, H, align_corners ? 1 : 0);
    a.ax = make_axis(w, W, align_corners ? 1 : 0);
    hipLaunchKernelGGL(k_doh_target_prob, dim3(pixel_blocks((int64_t)N * H * W)), dim3(NTHR), 0, st, a);
    return launch_failed("doh_target_prob");
}

extern "C" int doh_select(const float *p, int64_t total, int min_kept, float thresh, void *workspace, void *stream)
{
    if (!p || !workspace || total < 1 || total >= (1ll << 31)) {
        doh_set_error("doh_select: null pointer, or a pixel count outside [1, 2^31)");
        return DOH_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    uint32_t *ws = (uint32_t *)workspace;
    for (int pass = 0; pass < DOH_PASSES; ++pass) {
        if (pass > 0) {
            hipLaunchKernelGGL(k_doh_hist, dim3(pixel_blocks(total)), dim3(NTHR), 0, st, (const uint32_t *)p, (size_t)total, ws, pass);
            if (int rc = launch_failed("doh_select (histogram)"))
                return rc;
        }
        hipLaunchKernelGGL(k_doh_pick, dim3(1), dim3(NTHR), 0, st, ws, pass, min_kept, thresh);
        if (int rc = launch_failed("doh_select (pick)"))
            return rc;
    }
    return DOH_OK;
}

extern "C" int doh_reduce(const float *p, const float *l, const int64_t *target, int N, int H, int W, int ignore_index,
                          void *workspace, int64_t *hard, uint8_t *kept8, void *res, void *stream)
{
    if (N < 1 || H < 1 || W < 1 || (int64_t)N * H >= (1ll << 31) || (int64_t)N * H * W >= (1ll << 31)) {
        doh_set_error("doh_reduce: shape not taken");
        return DOH_EINVAL;
    }
    if (!p || !l || !target || !workspace || !hard || !res) {
        doh_set_error("doh_reduce: a tensor is null");
        return DOH_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    uint32_t *ws = (uint32_t *)workspace;
    hipLaunchKernelGGL(k_doh_reduce, dim3((unsigned)(N * H)), dim3(NTHR), 0, st, p, l, (const long long *)target, W,
                       (long long)ignore_index, ws, (long long *)hard, kept8);
    if (int rc = launch_failed("doh_reduce"))
        return rc;
    hipLaunchKernelGGL(k_doh_finish, dim3(1), dim3(NTHR), 0, st, (const uint32_t *)ws, N * H, (uint32_t *)res);
    return launch_failed("doh_reduce (finish)");
}
