// dcl_slide.hip -- sliding-window test-time augmentation with equal-size windows (include/dcl_slide.h): the reference
// (models/TTA_wrapper_PC.py, models/TTAWrapperSlide.py) writes, per scale, the resized image, its padded copy, a slice and a mirrored
// slice per window, and per window a read-modify-write of the canvas and of a count map.  Here the crop batch is ONE gather from the
// original image (k_slide_crops) and the averaged canvas ONE gather from the batch's logits (k_slide_gather).
//
// Both kernels follow dcl_tta.hip: a thread owns DSW_RUN = 4 consecutive output pixels of one row, forms tap indices and weights
// once and reuses them (over the input channels and both orientations in k_slide_crops, over a chunk of classes in k_slide_gather);
// a run is stored as one float4 where base and row length allow, element by element otherwise.  No LDS, no atomics, one thread per
// output element, offsets in 64 bits.  The window tables arrive by value in the kernel arguments and are indexed with wave-uniform
// indices only (the window of a workgroup in k_slide_crops, the loop counters in k_slide_gather), so they stay scalar loads.
//
// Arithmetic order is the reference's: ly0 * (lx0 a + lx1 b) + ly1 * (lx0 c + lx1 d) as ATen, 0.5 * (plain + mirrored), expf, the
// sum over the covering windows r ascending then q ascending starting from the first term, one division by the count.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcl_slide_plan.h"

namespace {

constexpr int NTHR = 256;
constexpr int RUN = DSW_RUN;
constexpr int CSUB = 8;       // classes a thread of k_slide_gather sums in registers per pass over the covering windows

struct Axis {
    float scale;
    int align;
    int in;        // size of the axis that is read
};

struct Tap {
    int i0, i1;
    float l0, l1;
};

struct Table {
    int row_lo[DSW_MAX_WIN];
    int col_lo[DSW_MAX_WIN];
};

struct Pad {
    float v[DSW_MAX_CIN];
};

Axis make_axis(int in_size, int out_size, int align)
{
    Axis a;
    a.align = align ? 1 : 0;
    a.in = in_size;
    a.scale = dcl_bilinear_scale(in_size, out_size, a.align);
    return a;
}

__device__ __forceinline__ Tap tap(const Axis a, int dst)
{
    Tap t;
    dcl_bilinear_src_index(a.scale, a.align, dst, a.in, &t.i0, &t.i1, &t.l0, &t.l1);
    return t;
}

// bilinear value of plane p at row taps r (i0 / i1 already multiplied by the row length) and column taps c
__device__ __forceinline__ float bilerp(const float *__restrict__ p, const Tap r, const Tap c)
{
    return r.l0 * (c.l0 * p[r.i0 + c.i0] + c.l1 * p[r.i0 + c.i1]) + r.l1 * (c.l0 * p[r.i1 + c.i0] + c.l1 * p[r.i1 + c.i1]);
}

// p[0 .. n) = v[0 .. n): one 16-byte store for a whole run at an aligned address, else element by element
__device__ __forceinline__ void store_run(float *__restrict__ p, const float (&v)[RUN], int n, bool vec)
{
    if (vec && n == RUN) {
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < RUN; ++k)
            if (k < n)
                p[k] = v[k];
    }
}

// out[n, c, y, x0 .. x0 + RUN) of window n = blockIdx.y, all channels, and its mirror in block Nw + n.  ay / ax: H -> nh, W -> nw.
__global__ __launch_bounds__(NTHR) void k_slide_crops(const float *__restrict__ x, int Cin, int H, int W, Axis ay, Axis ax, int nh, int nw,
                                                      Table tab, int Q, int wh, int ww, Pad pad, int mirror, float *__restrict__ out,
                                                      int Nw, int runs, int vec)
{
    const int item = blockIdx.x * NTHR + threadIdx.x;
    if (item >= wh * runs)
        return;
    const int y = item / runs, x0 = (item - y * runs) * RUN;
    const int n = blockIdx.y;                       // the workgroup's window: uniform, the table reads are scalar
    const int Y = tab.row_lo[n / Q] + y, X0 = tab.col_lo[n % Q] + x0;
    const int cnt = min(RUN, ww - x0);
    const bool row_in = Y < nh;
    Tap ty = tap(ay, row_in ? Y : 0);
    ty.i0 *= W, ty.i1 *= W;
    Tap tx[RUN];
    bool in[RUN];
#pragma unroll
    for (int k = 0; k < RUN; ++k) {
        in[k] = row_in && k < cnt && X0 + k < nw;
        tx[k] = tap(ax, in[k] ? X0 + k : 0);
    }
    const int64_t plane = (int64_t)H * W, oplane = (int64_t)wh * ww;
    for (int c = 0; c < Cin; ++c) {
        const float *__restrict__ xc = x + (int64_t)c * plane;
        const float pv = pad.v[c];
        float v[RUN];
#pragma unroll
        for (int k = 0; k < RUN; ++k)
            v[k] = in[k] ? bilerp(xc, ty, tx[k]) : pv;
        float *__restrict__ row = out + ((int64_t)n * Cin + c) * oplane + (int64_t)y * ww;
        store_run(row + x0, v, cnt, vec != 0);
        if (mirror) {
            // column x of the plain window is column ww - 1 - x of the mirrored one: a whole run lands on ww - x0 - RUN, reversed
            float *__restrict__ mrow = row + (int64_t)Nw * Cin * oplane;
            if (vec && cnt == RUN) {
                *reinterpret_cast<float4 *>(mrow + (ww - x0 - RUN)) = make_float4(v[3], v[2], v[1], v[0]);
            } else {
#pragma unroll
                for (int k = 0; k < RUN; ++k)
                    if (k < cnt)
                        mrow[ww - 1 - x0 - k] = v[k];
            }
        }
    }
}

// canvas[c, y, x0 .. x0 + RUN) of the thread's class chunk.  ay / ax: h -> wh, w -> ww.
template <bool FLIP>
__global__ __launch_bounds__(NTHR) void k_slide_gather(const float *__restrict__ z, const float *__restrict__ zf, int C, int h, int w,
                                                       Axis ay, Axis ax, int wh, int ww, Table tab, int R, int Q,
                                                       float *__restrict__ canvas, int Hc, int Wc, int runs, int cchunk, int vec)
{
    const int64_t item = (int64_t)blockIdx.x * NTHR + threadIdx.x;
    if (item >= (int64_t)Hc * runs)
        return;
    const int y = (int)(item / runs), x0 = (int)(item - (int64_t)y * runs) * RUN;
    const int n = min(RUN, Wc - x0);
    const int c0 = blockIdx.y * cchunk, c1 = min(C, c0 + cchunk);
    const int64_t plane = (int64_t)h * w;
    for (int cs = c0; cs < c1; cs += CSUB) {
        float acc[CSUB][RUN] = {};                  // 0 + e is e: the sum starts from its first term
        int cover[RUN] = {};
        for (int r = 0; r < R; ++r) {
            const int dy = y - tab.row_lo[r];
            if (dy < 0 || dy >= wh)
                continue;
            Tap ty = tap(ay, dy);
            ty.i0 *= w, ty.i1 *= w;
            for (int q = 0; q < Q; ++q) {
                const int dx0 = x0 - tab.col_lo[q];
                if (dx0 + RUN <= 0 || dx0 >= ww)
                    continue;
                Tap tx[RUN], tf[RUN];
                bool on[RUN];
#pragma unroll
                for (int k = 0; k < RUN; ++k) {
                    const int dx = dx0 + k;
                    on[k] = k < n && dx >= 0 && dx < ww;
                    const int d = on[k] ? dx : 0;
                    tx[k] = tap(ax, d);
                    if (FLIP)
                        tf[k] = tap(ax, ww - 1 - d);    // column d of the un-mirrored map is column ww - 1 - d of up(zf)
                }
                const int64_t base = (int64_t)(r * Q + q) * C * plane;
#pragma unroll
                for (int j = 0; j < CSUB; ++j) {
                    const int c = cs + j;
                    if (c >= c1)                    // (uniform over the workgroup: the last pass of a chunk may be short)
                        break;
                    const float *__restrict__ zc = z + base + (int64_t)c * plane;
#pragma unroll
                    for (int k = 0; k < RUN; ++k) {
                        if (!on[k])
                            continue;
                        float m = bilerp(zc, ty, tx[k]);
                        if (FLIP)
                            m = (m + bilerp(zf + base + (int64_t)c * plane, ty, tf[k])) * 0.5f;
                        acc[j][k] += expf(m);
                    }
                }
#pragma unroll
                for (int k = 0; k < RUN; ++k)
                    cover[k] += on[k] ? 1 : 0;
            }
        }
#pragma unroll
        for (int j = 0; j < CSUB; ++j) {
            if (cs + j >= c1)
                break;
            float v[RUN];
#pragma unroll
            for (int k = 0; k < RUN; ++k)
                v[k] = k < n ? acc[j][k] / (float)cover[k] : 0.f;     // the host check: cover >= 1 over every canvas pixel
            store_run(canvas + ((int64_t)(cs + j) * Hc + y) * Wc + x0, v, n, vec != 0);
        }
    }
}

int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        dsw_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return DSW_OK;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

bool fill_table(Table *t, const int *row_lo, int R, const int *col_lo, int Q)
{
    for (int i = 0; i < DSW_MAX_WIN; ++i) {
        t->row_lo[i] = i < R ? row_lo[i] : 0;
        t->col_lo[i] = i < Q ? col_lo[i] : 0;
        if (t->row_lo[i] < 0 || t->col_lo[i] < 0)
            return false;
    }
    return true;
}

}  // namespace

extern "C" int dsw_crops(const float *x, int Cin, int H, int W, int nh, int nw, const int *row_lo, int R, const int *col_lo, int Q,
                         int wh, int ww, const float *pad, int mirror, float *out, void *stream)
{
    if (R > DSW_MAX_WIN || Q > DSW_MAX_WIN) {
        dsw_set_error("dsw_crops: %d x %d windows, at most DSW_MAX_WIN = %d per axis", R, Q, DSW_MAX_WIN);
        return DSW_EINVAL;
    }
    if (!dsw_crops_ok(Cin, H, W, nh, nw, R, Q, wh, ww)) {
        dsw_set_error("dsw_crops: shape not taken (dsw_supported)");
        return DSW_EINVAL;
    }
    if (!x || !out || !row_lo || !col_lo || !pad) {
        dsw_set_error("dsw_crops: a pointer is null");
        return DSW_EINVAL;
    }
    Table tab;
    if (!fill_table(&tab, row_lo, R, col_lo, Q)) {
        dsw_set_error("dsw_crops: a window starts below 0");
        return DSW_EINVAL;
    }
    for (int r = 0; r < R; ++r)
        if ((int64_t)row_lo[r] + wh >= (1ll << 31)) {
            dsw_set_error("dsw_crops: window row %d + %d overflows", row_lo[r], wh);
            return DSW_EINVAL;
        }
    for (int q = 0; q < Q; ++q)
        if ((int64_t)col_lo[q] + ww + DSW_RUN >= (1ll << 31)) {
            dsw_set_error("dsw_crops: window column %d + %d overflows", col_lo[q], ww);
            return DSW_EINVAL;
        }
    Pad pv;
    for (int c = 0; c < DSW_MAX_CIN; ++c)
        pv.v[c] = c < Cin ? pad[c] : 0.f;
    const int runs = (ww + RUN - 1) / RUN;
    const int64_t bx = ((int64_t)wh * runs + NTHR - 1) / NTHR;          // wh * ww < 2^31: fits
    const dim3 grid((unsigned)bx, (unsigned)(R * Q));
    const int vec = aligned16(out) && (ww % RUN) == 0;
    hipLaunchKernelGGL(k_slide_crops, grid, dim3(NTHR), 0, (hipStream_t)stream, x, Cin, H, W, make_axis(H, nh, 0), make_axis(W, nw, 0), nh,
                       nw, tab, Q, wh, ww, pv, mirror ? 1 : 0, out, R * Q, runs, vec);
    return launched("dsw_crops");
}

extern "C" int dsw_gather(const float *z, const float *zf, int C, int h, int w, int wh, int ww, int align_inner, const int *row_lo, int R,
                          const int *col_lo, int Q, float *canvas, int Hc, int Wc, void *stream)
{
    if (R > DSW_MAX_WIN || Q > DSW_MAX_WIN) {
        dsw_set_error("dsw_gather: %d x %d windows, at most DSW_MAX_WIN = %d per axis", R, Q, DSW_MAX_WIN);
        return DSW_EINVAL;
    }
    if (!dsw_gather_ok(C, h, w, wh, ww, R, Q, Hc, Wc)) {
        dsw_set_error("dsw_gather: shape not taken (dsw_supported)");
        return DSW_EINVAL;
    }
    if (!z || !canvas || !row_lo || !col_lo) {
        dsw_set_error("dsw_gather: a pointer is null");
        return DSW_EINVAL;
    }
    const int rows = dsw_cover(Hc, wh, row_lo, R, nullptr), cols = dsw_cover(Wc, ww, col_lo, Q, nullptr);
    if (rows < 0 || cols < 0) {
        dsw_set_error("dsw_gather: a window starts outside the %d x %d canvas", Hc, Wc);
        return DSW_EINVAL;
    }
    if (rows < 1 || cols < 1) {
        dsw_set_error("dsw_gather: a pixel of the %d x %d canvas is under no %d x %d window (its count would be zero)", Hc, Wc, wh, ww);
        return DSW_EINVAL;
    }
    Table tab;
    fill_table(&tab, row_lo, R, col_lo, Q);
    const int runs = (Wc + RUN - 1) / RUN;
    const int64_t bx = ((int64_t)Hc * runs + NTHR - 1) / NTHR;
    // classes over grid y where the pixels alone give few workgroups, in whole register passes
    int64_t split = 1;
    if (bx < 2048) {
        split = (2048 + bx - 1) / bx;
        const int64_t most = C / CSUB > 1 ? C / CSUB : 1;
        split = split > most ? most : split;
    }
    int cchunk = (int)((C + split - 1) / split);
    cchunk = (cchunk + CSUB - 1) / CSUB * CSUB;
    const dim3 grid((unsigned)bx, (unsigned)((C + cchunk - 1) / cchunk));
    const int vec = aligned16(canvas) && (Wc % RUN) == 0;
    const Axis ay = make_axis(h, wh, align_inner), ax = make_axis(w, ww, align_inner);
    if (zf)
        hipLaunchKernelGGL(k_slide_gather<true>, grid, dim3(NTHR), 0, (hipStream_t)stream, z, zf, C, h, w, ay, ax, wh, ww, tab, R, Q,
                           canvas, Hc, Wc, runs, cchunk, vec);
    else
        hipLaunchKernelGGL(k_slide_gather<false>, grid, dim3(NTHR), 0, (hipStream_t)stream, z, zf, C, h, w, ay, ax, wh, ww, tab, R, Q,
                           canvas, Hc, Wc, runs, cchunk, vec);
    return launched("dsw_gather");
}
