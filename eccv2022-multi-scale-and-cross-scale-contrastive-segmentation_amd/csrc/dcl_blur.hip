// dcl_blur.hip -- the steps of the input augmentation that follow the crop (include/dcl_blur.h), on ONE image's float32 planes and its
// int64 label map, every launch on the caller's stream with no host readback.
//
//   k_blur_rows     PIL's three box passes along x: a workgroup stages DBL_ROW_TILE_H rows x (DBL_ROW_TILE_W columns + halo) in LDS
//                   (whole rows when w <= DBL_ROW_TILE_W) and ping-pongs the three passes between two LDS buffers.
//   k_blur_cols     the three passes along y: a workgroup owns a strip DBL_COL_TILE_W = 64 columns wide (every wave reads 64
//                   consecutive addresses) and a tile of DBL_COL_TILE_H rows + halo, LDS [row][64]: 57344 bytes at l = 7.
//                   The halo is 3 (l + 1) and the index is clamped to the image in every pass (dcl_blur_plan.h): a tile's result
//                   does not depend on where the tile lies.
//   k_pad_rows      one thread per output element of the planes and of the label map: the reflected source row.
//   k_gray_mean     m of the contrast operation, as k_aug_gray_mean of dcl_aug.hip: double sums per thread (grid-stride, fixed
//                   order), per workgroup (a fixed tree) and by the workgroup that draws the last ticket.  No float atomics.
//   k_colour        the colour chain of dcl_colour.h on a pixel of the planes, in place.
//   k_from_unit, k_normalise   the two ends of the chain.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcl_blur_plan.h"
#include "dcl_colour.h"

namespace {

constexpr int NTHR = 256;
constexpr int MAX_L = DBL_MAX_RADIUS - 1;                              // l of the largest radius
constexpr int ROW_EXT = DBL_ROW_TILE_W + 6 * (MAX_L + 1);              // 304
constexpr int COL_EXT = DBL_COL_TILE_H + 6 * (MAX_L + 1);              // 112
static_assert(2 * COL_EXT * DBL_COL_TILE_W * sizeof(float) < 64 * 1024, "a workgroup stays under 64 KB of LDS");
static_assert(NTHR % DBL_COL_TILE_W == 0, "whole strips of threads");

// one box pass at global index g of an axis of length n: the taps of line a (stride `st` between neighbours)
__device__ __forceinline__ float box_at(const float *a, int st, int g, int n, int base, int l, float ww, float fw)
{
    float acc = 0.f;
    for (int d = -l; d <= l; ++d)
        acc += a[dbl_tap(g, d, n, base) * st];
    const float e = a[dbl_tap(g, -l - 1, n, base) * st] + a[dbl_tap(g, l + 1, n, base) * st];
    return fmaf(ww, acc, fw * e);
}

__global__ __launch_bounds__(NTHR) void k_blur_rows(const float *__restrict__ src, float *__restrict__ dst, int rows, int w, int nseg,
                                                    int l, float ww, float fw)
{
    __shared__ float buf[2][DBL_ROW_TILE_H * ROW_EXT];
    constexpr int TH = DBL_ROW_TILE_H, TW = DBL_ROW_TILE_W;
    const int seg = blockIdx.x % nseg, rb = blockIdx.x / nseg;
    const int t0 = seg * TW, halo = dbl_halo(l), ext = dbl_ext(TW, l), base = t0 - halo;
    for (int i = threadIdx.x; i < TH * ext; i += NTHR) {
        const int r = i / ext, j = i - r * ext;
        const int row = rb * TH + r, g = base + j;
        buf[0][i] = (row < rows && g >= 0 && g < w) ? src[(int64_t)row * w + g] : 0.f;
    }
    __syncthreads();
    for (int p = 1; p <= 3; ++p) {
        const float *a = buf[(p - 1) & 1];
        float *b = buf[p & 1];
        const int lo = dbl_pass_lo(p, l), span = dbl_pass_hi(p, TW, l) - lo;
        for (int i = threadIdx.x; i < TH * span; i += NTHR) {
            const int r = i / span, j = lo + i - r * span;
            const int g = base + j;
            if (g >= 0 && g < w)
                b[r * ext + j] = box_at(a + r * ext, 1, g, w, base, l, ww, fw);
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < TH * TW; i += NTHR) {
        const int r = i / TW, x = i - r * TW;
        const int row = rb * TH + r, g = t0 + x;
        if (row < rows && g < w)
            dst[(int64_t)row * w + g] = buf[1][r * ext + halo + x];
    }
}

__global__ __launch_bounds__(NTHR) void k_blur_cols(const float *__restrict__ src, float *__restrict__ dst, int h, int w, int nstrip,
                                                    int ntile, int l, float ww, float fw)
{
    __shared__ float buf[2][COL_EXT * DBL_COL_TILE_W];
    constexpr int TH = DBL_COL_TILE_H, TW = DBL_COL_TILE_W, NG = NTHR / TW;
    const int strip = blockIdx.x % nstrip, rest = blockIdx.x / nstrip;
    const int tile = rest % ntile, plane = rest / ntile;
    const int col = threadIdx.x % TW, rg = threadIdx.x / TW;
    const int x = strip * TW + col;
    const int t0 = tile * TH, halo = dbl_halo(l), ext = dbl_ext(TH, l), base = t0 - halo;
    const int64_t off = (int64_t)plane * h * w + x;
    for (int j = rg; j < ext; j += NG) {
        const int g = base + j;
        buf[0][j * TW + col] = (x < w && g >= 0 && g < h) ? src[off + (int64_t)g * w] : 0.f;
    }
    __syncthreads();
    for (int p = 1; p <= 3; ++p) {
        const float *a = buf[(p - 1) & 1];
        float *b = buf[p & 1];
        const int hi = dbl_pass_hi(p, TH, l);
        for (int j = dbl_pass_lo(p, l) + rg; j < hi; j += NG) {
            const int g = base + j;
            if (g >= 0 && g < h)
                b[j * TW + col] = box_at(a + col, TW, g, h, base, l, ww, fw);
        }
        __syncthreads();
    }
    for (int j = rg; j < TH; j += NG) {
        const int g = t0 + j;
        if (x < w && g < h)
            dst[off + (int64_t)g * w] = buf[1][(halo + j) * TW + col];
    }
}

// planes 0 .. C - 1: the image's; plane C: the label map
__global__ __launch_bounds__(NTHR) void k_pad_rows(const float *__restrict__ src, float *__restrict__ dst,
                                                   const int64_t *__restrict__ lbl_src, int64_t *__restrict__ lbl_dst, int C, int h, int w,
                                                   int top, int ho)
{
    const int64_t n = (int64_t)ho * w;
    const int64_t i = (int64_t)blockIdx.x * NTHR + threadIdx.x;
    if (i >= (int64_t)(C + 1) * n)
        return;
    const int plane = (int)(i / n);
    const int64_t q = i - (int64_t)plane * n;
    const int y = (int)(q / w), x = (int)(q - (int64_t)y * w);
    const int64_t s = (int64_t)dbl_reflect_row(y, top, h) * w + x;
    if (plane < C)
        dst[i] = src[(int64_t)plane * h * w + s];
    else
        lbl_dst[q] = lbl_src[s];
}

__device__ __forceinline__ int contrast_pos(const dbl_colour_plan &pl)
{
    for (int i = 0; i < pl.ncolor; ++i)
        if (pl.perm[i] == 1)
            return i;
    return -1;
}

__global__ __launch_bounds__(NTHR) void k_gray_mean(const float *__restrict__ planes, const dbl_colour_plan pl, int32_t *__restrict__ ws,
                                                    int cpos)
{
    __shared__ double sh[NTHR];
    const int n = pl.h * pl.w;
    double sum = 0.0;
    for (int i = blockIdx.x * NTHR + threadIdx.x; i < n; i += gridDim.x * NTHR) {
        const Rgb v = {planes[i], planes[(int64_t)n + i], planes[2 * (int64_t)n + i]};
        sum += (double)luma(colour_ops(v, pl, 0, cpos, 0.f));
    }
    sh[threadIdx.x] = sum;
    __syncthreads();
    for (int s = NTHR / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    double *part = reinterpret_cast<double *>(ws + DBL_WS_PART);
    unsigned *ticket = reinterpret_cast<unsigned *>(ws + DBL_WS_TICKET);
    if (threadIdx.x == 0) {
        // publish, then draw a ticket: the release orders the partial sum before the ticket for whoever draws the last one
        __hip_atomic_store(part + blockIdx.x, sh[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (t == gridDim.x - 1u) {
            double total = 0.0;
            for (unsigned b = 0; b < gridDim.x; ++b)
                total += __hip_atomic_load(part + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ws[DBL_WS_MEAN] = __float_as_int((float)(total / (double)n));
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);        // for the next call
        }
    }
}

__global__ __launch_bounds__(NTHR) void k_colour(float *__restrict__ planes, const dbl_colour_plan pl, const int32_t *__restrict__ ws,
                                                 int cpos)
{
    const int n = pl.h * pl.w;
    const int i = blockIdx.x * NTHR + threadIdx.x;
    if (i >= n)
        return;
    const float m = cpos >= 0 ? __int_as_float(ws[DBL_WS_MEAN]) : 0.f;
    Rgb v = {planes[i], planes[(int64_t)n + i], planes[2 * (int64_t)n + i]};
    v = colour_ops(v, pl, 0, pl.ncolor, m);
    planes[i] = v.r;
    planes[(int64_t)n + i] = v.g;
    planes[2 * (int64_t)n + i] = v.b;
}

__global__ __launch_bounds__(NTHR) void k_from_unit(const float *src, float *dst, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * NTHR + threadIdx.x;
    if (i < n)
        dst[i] = src[i] * 255.f;
}

__global__ __launch_bounds__(NTHR) void k_normalise(const float *__restrict__ planes, float *__restrict__ out, int normalise, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * NTHR + threadIdx.x;
    if (i >= n)
        return;
    Rgb v = {planes[i] / 255.f, planes[n + i] / 255.f, planes[2 * n + i] / 255.f};
    if (normalise)
        v = {(v.r - 0.485f) / 0.229f, (v.g - 0.456f) / 0.224f, (v.b - 0.406f) / 0.225f};
    out[i] = v.r;
    out[n + i] = v.g;
    out[2 * n + i] = v.b;
}

#define DBL_CHECK_ARG(cond, what)                        \
    do {                                                 \
        if (!(cond)) {                                   \
            dbl_set_error("%s: %s", what, #cond);        \
            return DBL_EINVAL;                           \
        }                                                \
    } while (0)

int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        dbl_set_error("%s: %s", what, hipGetErrorString(e));
        return DBL_EINVAL;
    }
    return DBL_OK;
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + NTHR - 1) / NTHR); }

bool colour_plan_ok(const dbl_colour_plan *p)
{
    if (!p || p->h < 1 || p->w < 1 || 3 * (int64_t)p->h * p->w >= (1ll << 31) || p->ncolor < 0 || p->ncolor > 4)
        return false;
    int seen = 0;
    for (int i = 0; i < p->ncolor; ++i) {
        if (p->perm[i] < 0 || p->perm[i] > 3 || (seen >> p->perm[i] & 1))
            return false;
        seen |= 1 << p->perm[i];
    }
    return isfinite(p->b) && isfinite(p->c) && isfinite(p->s) && isfinite(p->delta);
}

}  // namespace

extern "C" int dbl_blur(const float *src, float *dst, float *scratch, int C, int h, int w, int radius, void *stream)
{
    DBL_CHECK_ARG(src && dst && scratch && src != dst && src != scratch && dst != scratch && dbl_blur_ok(C, h, w, radius), "dbl_blur");
    const DblBox box = dbl_box_of(radius);
    DBL_CHECK_ARG(box.l >= 0 && box.l <= MAX_L, "dbl_blur");
    const int rows = C * h;                                            // < 2^31 (dbl_blur_ok)
    const int nseg = (w + DBL_ROW_TILE_W - 1) / DBL_ROW_TILE_W;
    const int64_t nrb = (rows + DBL_ROW_TILE_H - 1) / DBL_ROW_TILE_H;
    const int nstrip = (w + DBL_COL_TILE_W - 1) / DBL_COL_TILE_W, ntile = (h + DBL_COL_TILE_H - 1) / DBL_COL_TILE_H;
    DBL_CHECK_ARG(nseg * nrb < (1ll << 31) && (int64_t)nstrip * ntile * C < (1ll << 31), "dbl_blur (grid)");
    hipLaunchKernelGGL(k_blur_rows, dim3((unsigned)(nseg * nrb)), dim3(NTHR), 0, (hipStream_t)stream, src, scratch, rows, w, nseg,
                       box.l, box.ww, box.fw);
    if (launched("dbl_blur (rows)") != DBL_OK)
        return DBL_EINVAL;
    hipLaunchKernelGGL(k_blur_cols, dim3((unsigned)((int64_t)nstrip * ntile * C)), dim3(NTHR), 0, (hipStream_t)stream, scratch, dst, h,
                       w, nstrip, ntile, box.l, box.ww, box.fw);
    return launched("dbl_blur (columns)");
}

extern "C" int dbl_pad_rows(const float *src, float *dst, const int64_t *lbl_src, int64_t *lbl_dst, int C, int h, int w, int top,
                            int bottom, void *stream)
{
    DBL_CHECK_ARG(src && dst && lbl_src && lbl_dst && src != dst && lbl_src != lbl_dst && dbl_pad_ok(C, h, w, top, bottom),
                  "dbl_pad_rows");
    const int ho = h + top + bottom;
    hipLaunchKernelGGL(k_pad_rows, dim3(blocks_of((int64_t)(C + 1) * ho * w)), dim3(NTHR), 0, (hipStream_t)stream, src, dst, lbl_src,
                       lbl_dst, C, h, w, top, ho);
    return launched("dbl_pad_rows");
}

extern "C" int dbl_gray_mean(const float *planes, const dbl_colour_plan *plan, int32_t *ws, void *stream)
{
    DBL_CHECK_ARG(planes && ws && ((uintptr_t)ws & 7) == 0 && colour_plan_ok(plan), "dbl_gray_mean");
    int cpos = -1;
    for (int i = 0; i < plan->ncolor; ++i)
        if (plan->perm[i] == 1)
            cpos = i;
    DBL_CHECK_ARG(cpos >= 0, "dbl_gray_mean (the chain holds no contrast)");
    const int64_t n = (int64_t)plan->h * plan->w;
    unsigned blocks = blocks_of(n);
    if (blocks > DBL_MAX_BLOCKS)
        blocks = DBL_MAX_BLOCKS;
    hipLaunchKernelGGL(k_gray_mean, dim3(blocks), dim3(NTHR), 0, (hipStream_t)stream, planes, *plan, ws, cpos);
    return launched("dbl_gray_mean");
}

extern "C" int dbl_colour(float *planes, const dbl_colour_plan *plan, const int32_t *ws, void *stream)
{
    DBL_CHECK_ARG(planes && ws && colour_plan_ok(plan), "dbl_colour");
    int cpos = -1;
    for (int i = 0; i < plan->ncolor; ++i)
        if (plan->perm[i] == 1)
            cpos = i;
    hipLaunchKernelGGL(k_colour, dim3(blocks_of((int64_t)plan->h * plan->w)), dim3(NTHR), 0, (hipStream_t)stream, planes, *plan, ws,
                       cpos);
    return launched("dbl_colour");
}

extern "C" int dbl_from_unit(const float *src, float *dst, int64_t n, void *stream)
{
    DBL_CHECK_ARG(src && dst && n >= 1 && n < (1ll << 31), "dbl_from_unit");
    hipLaunchKernelGGL(k_from_unit, dim3(blocks_of(n)), dim3(NTHR), 0, (hipStream_t)stream, src, dst, n);
    return launched("dbl_from_unit");
}

extern "C" int dbl_normalise(const float *planes, float *out, int normalise, int64_t n, void *stream)
{
    DBL_CHECK_ARG(planes && out && planes != out && n >= 1 && 3 * n < (1ll << 31), "dbl_normalise");
    hipLaunchKernelGGL(k_normalise, dim3(blocks_of(n)), dim3(NTHR), 0, (hipStream_t)stream, planes, out, normalise, n);
    return launched("dbl_normalise");
}
