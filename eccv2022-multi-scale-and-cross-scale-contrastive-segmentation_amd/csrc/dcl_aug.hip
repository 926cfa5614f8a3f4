// dcl_aug.hip -- the input augmentation of ONE image (include/dcl_aug.h): three launches on the caller's stream that take the decoded
// uint8 pixels to the image's float32 [3, h, w] / int64 [h, w] slice of the batch, with no host readback in between.
//
//   k_aug_crop_select  one workgroup per candidate crop: the candidate window's labels (through flip, nearest index, pad and lookup
//                      table: dcl_aug_plan.h) into 256 LDS bins with integer atomics, then the verdict and the two counts to ws.
//   k_aug_gray_mean    m of the contrast operation: L of every pixel of the chosen crop after the operations that precede contrast,
//                      summed in double per thread (grid-stride, fixed order), per workgroup (a fixed tree) and by the workgroup
//                      that draws the last ticket over the partial sums in index order.  No float atomics: bitwise reproducible.
//   k_aug_apply        one thread per output pixel: the chosen corner and m from ws, the triangle filter's taps on the uint8 source,
//                      the colour chain, normalisation; the padded region never touches the source.
//
// The plan travels by value in the kernel arguments.  The x taps' weights are formed again for every row tap instead of being kept
// in a per-thread array (a runtime-indexed array would live in scratch).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcl_aug_plan.h"
#include "dcl_colour.h"

namespace {

constexpr int NTHR = 256;
constexpr int NSEL = 1024;          // threads of a candidate's workgroup

// the resized image at (ry, rx): sum over row taps of wy * (sum over column taps of wx * src)
__device__ __forceinline__ Rgb resized_pixel(const uint8_t *__restrict__ img, const dau_plan &pl, const DauAxis ay, const DauAxis ax,
                                             int ry, int rx)
{
    int y0, y1, x0, x1;
    double cy, cx;
    const double sy = dau_tap_range(ay, ry, &y0, &y1, &cy);
    const double sx = dau_tap_range(ax, rx, &x0, &x1, &cx);
    Rgb acc = {0.f, 0.f, 0.f};
    for (int ky = y0; ky < y1; ++ky) {
        const float wy = dau_tap_weight(ay, cy, sy, ky);
        const uint8_t *row = img + (int64_t)ky * pl.W * 3;
        Rgb line = {0.f, 0.f, 0.f};
        for (int kx = x0; kx < x1; ++kx) {
            const float wx = dau_tap_weight(ax, cx, sx, kx);
            const uint8_t *px = row + 3 * dau_src_col(kx, pl.W, pl.flip);
            line.r = fmaf(wx, (float)px[0], line.r);
            line.g = fmaf(wx, (float)px[1], line.g);
            line.b = fmaf(wx, (float)px[2], line.b);
        }
        acc.r = fmaf(wy, line.r, acc.r);
        acc.g = fmaf(wy, line.g, acc.g);
        acc.b = fmaf(wy, line.b, acc.b);
    }
    return acc;
}

__global__ __launch_bounds__(NSEL) void k_aug_crop_select(const uint8_t *__restrict__ lbl, const uint8_t *__restrict__ lut,
                                                          const dau_plan pl, int32_t *__restrict__ ws)
{
    __shared__ int hist[256];
    const int p = blockIdx.x;
    for (int i = threadIdx.x; i < 256; i += NSEL)
        hist[i] = 0;
    __syncthreads();
    const int n = pl.h * pl.w;                       // < 2^31 / 3 (dau_plan_ok)
    for (int i = threadIdx.x; i < n; i += NSEL) {
        const int y = i / pl.w, x = i - y * pl.w;
        int ry, rx;
        const int v = dau_crop_to_resized(pl, p, y, x, &ry, &rx) ? dau_label_at(lbl, lut, pl, ry, rx) : pl.ignore;
        atomicAdd(&hist[v], 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int classes = 0, mx = 0, sum = 0;
        for (int b = 0; b < 256; ++b) {
            const int c = b == pl.ignore ? 0 : hist[b];
            classes += c > 0;
            mx = max(mx, c);
            sum += c;
        }
        ws[3 * p + 0] = dau_verdict(classes, mx, sum, pl.max_ratio);
        ws[3 * p + 1] = mx;
        ws[3 * p + 2] = sum;
    }
}

__global__ __launch_bounds__(NTHR) void k_aug_gray_mean(const uint8_t *__restrict__ img, const dau_plan pl, int32_t *__restrict__ ws,
                                                        int cpos)
{
    __shared__ double sh[NTHR];
    const int p = dau_chosen(ws, pl.P);
    const DauAxis ay = dau_axis(pl.H, pl.rh), ax = dau_axis(pl.W, pl.rw);
    const int n = pl.h * pl.w;
    double sum = 0.0;
    for (int i = blockIdx.x * NTHR + threadIdx.x; i < n; i += gridDim.x * NTHR) {
        const int y = i / pl.w, x = i - y * pl.w;
        int ry, rx;
        Rgb v = {0.f, 0.f, 0.f};
        if (dau_crop_to_resized(pl, p, y, x, &ry, &rx))
            v = resized_pixel(img, pl, ay, ax, ry, rx);
        sum += (double)luma(colour_ops(v, pl, 0, cpos, 0.f));
    }
    sh[threadIdx.x] = sum;
    __syncthreads();
    for (int s = NTHR / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    double *part = reinterpret_cast<double *>(ws + DAU_WS_PART);
    unsigned *ticket = reinterpret_cast<unsigned *>(ws + DAU_WS_TICKET);
    if (threadIdx.x == 0) {
        // publish, then draw a ticket: the release orders the partial sum before the ticket for whoever draws the last one
        __hip_atomic_store(part + blockIdx.x, sh[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (t == gridDim.x - 1u) {
            double total = 0.0;
            for (unsigned b = 0; b < gridDim.x; ++b)
                total += __hip_atomic_load(part + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ws[DAU_WS_MEAN] = __float_as_int((float)(total / (double)n));
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);        // for the next call
        }
    }
}

__global__ __launch_bounds__(NTHR) void k_aug_apply(const uint8_t *__restrict__ img, const uint8_t *__restrict__ lbl,
                                                    const uint8_t *__restrict__ lut, const dau_plan pl, const int32_t *__restrict__ ws,
                                                    float *__restrict__ out_img, int64_t *__restrict__ out_lbl, int cpos)
{
    const int n = pl.h * pl.w;
    const int i = blockIdx.x * NTHR + threadIdx.x;
    if (i >= n)
        return;
    const int p = dau_chosen(ws, pl.P);
    const float m = cpos >= 0 ? __int_as_float(ws[DAU_WS_MEAN]) : 0.f;
    const int y = i / pl.w, x = i - y * pl.w;
    int ry, rx;
    Rgb v = {0.f, 0.f, 0.f};
    int label = pl.ignore;
    if (dau_crop_to_resized(pl, p, y, x, &ry, &rx)) {
        v = resized_pixel(img, pl, dau_axis(pl.H, pl.rh), dau_axis(pl.W, pl.rw), ry, rx);
        label = dau_label_at(lbl, lut, pl, ry, rx);
    }
    v = colour_ops(v, pl, 0, pl.ncolor, m);
    v = {v.r / 255.f, v.g / 255.f, v.b / 255.f};
    if (pl.normalise)
        v = {(v.r - 0.485f) / 0.229f, (v.g - 0.456f) / 0.224f, (v.b - 0.406f) / 0.225f};
    out_img[i] = v.r;
    out_img[(int64_t)n + i] = v.g;
    out_img[2 * (int64_t)n + i] = v.b;
    out_lbl[i] = label;
}

#define DAU_CHECK_ARG(cond, what)                        \
    do {                                                 \
        if (!(cond)) {                                   \
            dau_set_error("%s: %s", what, #cond);        \
            return DAU_EINVAL;                           \
        }                                                \
    } while (0)

int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        dau_set_error("%s: %s", what, hipGetErrorString(e));
        return DAU_EINVAL;
    }
    return DAU_OK;
}

}  // namespace

extern "C" int dau_crop_select(const uint8_t *lbl, const uint8_t *lut, const dau_plan *plan, int32_t *ws, void *stream)
{
    DAU_CHECK_ARG(lbl && lut && ws && dau_plan_ok(plan), "dau_crop_select");
    hipLaunchKernelGGL(k_aug_crop_select, dim3(plan->P), dim3(NSEL), 0, (hipStream_t)stream, lbl, lut, *plan, ws);
    return launched("dau_crop_select");
}

extern "C" int dau_gray_mean(const uint8_t *img, const dau_plan *plan, int32_t *ws, void *stream)
{
    DAU_CHECK_ARG(img && ws && ((uintptr_t)ws & 7) == 0 && dau_plan_ok(plan), "dau_gray_mean");
    const int cpos = dau_contrast_pos(*plan);
    DAU_CHECK_ARG(cpos >= 0, "dau_gray_mean (the chain holds no contrast)");
    const int64_t n = (int64_t)plan->h * plan->w;
    int blocks = (int)((n + NTHR - 1) / NTHR);
    if (blocks > DAU_MAX_BLOCKS)
        blocks = DAU_MAX_BLOCKS;
    hipLaunchKernelGGL(k_aug_gray_mean, dim3(blocks), dim3(NTHR), 0, (hipStream_t)stream, img, *plan, ws, cpos);
    return launched("dau_gray_mean");
}

extern "C" int dau_apply(const uint8_t *img, const uint8_t *lbl, const uint8_t *lut, const dau_plan *plan, const int32_t *ws,
                         float *out_img, int64_t *out_lbl, void *stream)
{
    DAU_CHECK_ARG(img && lbl && lut && ws && out_img && out_lbl && dau_plan_ok(plan), "dau_apply");
    const int64_t n = (int64_t)plan->h * plan->w;
    hipLaunchKernelGGL(k_aug_apply, dim3((unsigned)((n + NTHR - 1) / NTHR)), dim3(NTHR), 0, (hipStream_t)stream, img, lbl, lut, *plan,
                       ws, out_img, out_lbl, dau_contrast_pos(*plan));
    return launched("dau_apply");
}
