// dcl_tta.hip -- the merge of test-time-augmentation views (include/dcl_tta.h): the reference (models/TTA_wrapper.py,
// models/TTA_wrapper_CTS.py) writes, per view, the logits at the scaled size, a mirrored copy, the copy resized to the input size and
// then the sum; all of that is a linear gather from the model's low-resolution logits, so here every view is ONE read-modify-write of
// the accumulator and reads of a map that stays in cache.
//
// All three kernels have one shape.  A thread owns DTT_RUN = 4 consecutive output pixels of one row: it forms their tap indices and
// weights once and then walks the classes of its class chunk, so the index arithmetic is amortised over C.  The accumulator run is
// read and written as one float4 where its base, the row length and the column offset allow (a scalar tail otherwise); the
// low-resolution taps are plain scalar loads (neighbouring lanes read neighbouring or identical addresses: L1 / L2 serve them).  No
// LDS, no atomics: one thread per accumulator element and launch, offsets in 64 bits.  Pixel items fill grid x; where they alone give
// fewer than ~2048 workgroups the classes are split over grid y (chunks of at least 8 classes).
//
// Arithmetic order is the reference's: the inner bilinear value of each of the four outer taps first (ly0 * (lx0 a + lx1 b) + ly1 *
// (lx0 c + lx1 d), as ATen), then the same expression over them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcl_tta_plan.h"

namespace {

constexpr int NTHR = 256;
constexpr int RUN = DTT_RUN;

struct Axis {
    float scale;
    int align;
    int in;        // size of the axis that is read
};

struct Tap {
    int i0, i1;
    float l0, l1;
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

// bilinear value of plane p (row length w) at row taps r (i0 / i1 already multiplied by w) and column taps c
__device__ __forceinline__ float bilerp(const float *__restrict__ p, const Tap r, const Tap c)
{
    return r.l0 * (c.l0 * p[r.i0 + c.i0] + c.l1 * p[r.i0 + c.i1]) + r.l1 * (c.l0 * p[r.i1 + c.i0] + c.l1 * p[r.i1 + c.i1]);
}

// p[0 .. n) += s * v[0 .. n): one 16-byte read-modify-write for a whole run at an aligned address, else element by element
__device__ __forceinline__ void add_run(float *__restrict__ p, const float (&v)[RUN], int n, bool vec, float s)
{
    if (vec && n == RUN) {
        float4 a = *reinterpret_cast<const float4 *>(p);
        a.x = fmaf(s, v[0], a.x);
        a.y = fmaf(s, v[1], a.y);
        a.z = fmaf(s, v[2], a.z);
        a.w = fmaf(s, v[3], a.w);
        *reinterpret_cast<float4 *>(p) = a;
    } else {
#pragma unroll
        for (int k = 0; k < RUN; ++k)
            if (k < n)
                p[k] = fmaf(s, v[k], p[k]);
    }
}

// the thread's item: output row and first column of its run; false past the end
__device__ __forceinline__ bool my_item(int rows, int runs, int &y, int &x0)
{
    const int64_t item = (int64_t)blockIdx.x * NTHR + threadIdx.x;
    if (item >= (int64_t)rows * runs)
        return false;
    y = (int)(item / runs);
    x0 = (int)(item - (int64_t)y * runs) * RUN;
    return true;
}

// acc[c, Y, X] += weight * outer(unflip(inner(z)))[c, Y, X].  iy / ix: h -> Hm, w -> Wm; oy / ox: Hm -> H, Wm -> W.
// IDENT: h == Hm and w == Wm, the inner level is the identity.
template <bool IDENT>
__global__ __launch_bounds__(NTHR) void k_tta_merge(const float *__restrict__ z, int C, int h, int w, Axis iy, Axis ix, int Wm, int flip,
                                                    Axis oy, Axis ox, float *__restrict__ acc, int H, int W, int runs, int cchunk,
                                                    float weight, int vec)
{
    int Y, X0;
    if (!my_item(H, runs, Y, X0))
        return;
    const int n = min(RUN, W - X0);
    const Tap ty = tap(oy, Y);                      // rows of the Hm x Wm map
    Tap ya = {}, yb = {};                           // their rows of z (times w)
    if (!IDENT) {
        ya = tap(iy, ty.i0);
        yb = tap(iy, ty.i1);
        ya.i0 *= w, ya.i1 *= w, yb.i0 *= w, yb.i1 *= w;
    }
    Tap tx[RUN], xa[RUN], xb[RUN];                  // columns of the map; of z for the left / right map column
#pragma unroll
    for (int k = 0; k < RUN; ++k) {
        tx[k] = tap(ox, min(X0 + k, W - 1));
        if (flip) {                                 // the map holds the mirrored view: column x of the un-mirrored one is Wm - 1 - x
            tx[k].i0 = Wm - 1 - tx[k].i0;
            tx[k].i1 = Wm - 1 - tx[k].i1;
        }
        if (!IDENT) {
            xa[k] = tap(ix, tx[k].i0);
            xb[k] = tap(ix, tx[k].i1);
        }
    }
    const int c0 = blockIdx.y * cchunk, c1 = min(C, c0 + cchunk);
    const int64_t plane = (int64_t)h * w;
    for (int c = c0; c < c1; ++c) {
        const float *__restrict__ zc = z + (int64_t)c * plane;
        float v[RUN];
#pragma unroll
        for (int k = 0; k < RUN; ++k) {
            float m00, m01, m10, m11;               // the four map values under the outer taps
            if (IDENT) {
                const float *r0 = zc + (int64_t)ty.i0 * w, *r1 = zc + (int64_t)ty.i1 * w;
                m00 = r0[tx[k].i0], m01 = r0[tx[k].i1], m10 = r1[tx[k].i0], m11 = r1[tx[k].i1];
            } else {
                m00 = bilerp(zc, ya, xa[k]), m01 = bilerp(zc, ya, xb[k]);
                m10 = bilerp(zc, yb, xa[k]), m11 = bilerp(zc, yb, xb[k]);
            }
            v[k] = ty.l0 * (tx[k].l0 * m00 + tx[k].l1 * m01) + ty.l1 * (tx[k].l0 * m10 + tx[k].l1 * m11);
        }
        add_run(acc + ((int64_t)c * H + Y) * W + X0, v, n, vec != 0, weight);
    }
}

// canvas[c, h0 + y, w0 + x] += exp(m[c, y, x]), m = up(z) or 0.5 * (up(z) + unflip(up(zf))).  ay / ax: h -> ch, w -> cw.
template <bool FLIP>
__global__ __launch_bounds__(NTHR) void k_tta_window(const float *__restrict__ z, const float *__restrict__ zf, int C, int h, int w,
                                                     Axis ay, Axis ax, int cw, float *__restrict__ canvas, int Hc, int Wc, int h0, int w0,
                                                     int wh, int ww, int runs, int cchunk, int vec)
{
    int y, x0;
    if (!my_item(wh, runs, y, x0))
        return;
    const int n = min(RUN, ww - x0);
    Tap ty = tap(ay, y);
    ty.i0 *= w, ty.i1 *= w;
    Tap tx[RUN], tf[RUN];
#pragma unroll
    for (int k = 0; k < RUN; ++k) {
        const int x = min(x0 + k, ww - 1);
        tx[k] = tap(ax, x);
        if (FLIP)
            tf[k] = tap(ax, cw - 1 - x);            // column x of the un-mirrored map is column cw - 1 - x of up(zf)
    }
    const int c0 = blockIdx.y * cchunk, c1 = min(C, c0 + cchunk);
    const int64_t plane = (int64_t)h * w;
    for (int c = c0; c < c1; ++c) {
        float v[RUN];
#pragma unroll
        for (int k = 0; k < RUN; ++k) {
            float m = bilerp(z + (int64_t)c * plane, ty, tx[k]);
            if (FLIP)
                m = (m + bilerp(zf + (int64_t)c * plane, ty, tf[k])) * 0.5f;
            v[k] = expf(m);
        }
        add_run(canvas + ((int64_t)c * Hc + h0 + y) * Wc + w0 + x0, v, n, vec != 0, 1.f);
    }
}

// acc[c, Y, X] += resize(canvas / count)[c, Y, X], count[y, x] = rowcnt[y] * colcnt[x].  ay / ax: Hc -> H, Wc -> W.
__global__ __launch_bounds__(NTHR) void k_tta_canvas(const float *__restrict__ canvas, const int32_t *__restrict__ rowcnt,
                                                     const int32_t *__restrict__ colcnt, int C, int Hc, int Wc, Axis ay, Axis ax,
                                                     float *__restrict__ acc, int H, int W, int runs, int cchunk, int vec)
{
    int Y, X0;
    if (!my_item(H, runs, Y, X0))
        return;
    const int n = min(RUN, W - X0);
    Tap ty = tap(ay, Y);
    const int r0 = rowcnt[ty.i0], r1 = rowcnt[ty.i1];
    ty.i0 *= Wc, ty.i1 *= Wc;
    Tap tx[RUN];
    float n00[RUN], n01[RUN], n10[RUN], n11[RUN];   // the counts under the four taps (small integers: exact as floats)
#pragma unroll
    for (int k = 0; k < RUN; ++k) {
        tx[k] = tap(ax, min(X0 + k, W - 1));
        const int q0 = colcnt[tx[k].i0], q1 = colcnt[tx[k].i1];
        n00[k] = (float)(r0 * q0), n01[k] = (float)(r0 * q1), n10[k] = (float)(r1 * q0), n11[k] = (float)(r1 * q1);
    }
    const int c0 = blockIdx.y * cchunk, c1 = min(C, c0 + cchunk);
    const int64_t plane = (int64_t)Hc * Wc;
    for (int c = c0; c < c1; ++c) {
        const float *__restrict__ p = canvas + (int64_t)c * plane;
        float v[RUN];
#pragma unroll
        for (int k = 0; k < RUN; ++k) {
            const Tap t = tx[k];
            v[k] = ty.l0 * (t.l0 * (p[ty.i0 + t.i0] / n00[k]) + t.l1 * (p[ty.i0 + t.i1] / n01[k])) +
                   ty.l1 * (t.l0 * (p[ty.i1 + t.i0] / n10[k]) + t.l1 * (p[ty.i1 + t.i1] / n11[k]));
        }
        add_run(acc + ((int64_t)c * H + Y) * W + X0, v, n, vec != 0, 1.f);
    }
}

int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        dtt_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return DTT_OK;
}

// grid of `rows` x ceil(cols / RUN) pixel items and C classes
dim3 grid_for(int rows, int cols, int C, int *runs, int *cchunk)
{
    *runs = (cols + RUN - 1) / RUN;
    const int64_t bx = ((int64_t)rows * *runs + NTHR - 1) / NTHR;
    int64_t split = 1;
    if (bx < 2048) {
        split = (2048 + bx - 1) / bx;
        const int64_t most = C / 8 > 1 ? C / 8 : 1;
        split = split > most ? most : split;
    }
    *cchunk = (int)((C + split - 1) / split);
    return dim3((unsigned)bx, (unsigned)((C + *cchunk - 1) / *cchunk));
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int dtt_merge(const float *z, int C, int h, int w, int Hm, int Wm, int align_inner, int flip, float *acc, int H, int W,
                         int align_outer, float weight, void *stream)
{
    if (!dtt_shape_ok(C, h, w, Hm, Wm, H, W)) {
        dtt_set_error("dtt_merge: shape not taken (dtt_supported)");
        return DTT_EINVAL;
    }
    if (!z || !acc) {
        dtt_set_error("dtt_merge: a tensor is null");
        return DTT_EINVAL;
    }
    int runs, cchunk;
    const dim3 grid = grid_for(H, W, C, &runs, &cchunk);
    const int vec = aligned16(acc) && (W % RUN) == 0;
    const Axis iy = make_axis(h, Hm, align_inner), ix = make_axis(w, Wm, align_inner);
    const Axis oy = make_axis(Hm, H, align_outer), ox = make_axis(Wm, W, align_outer);
    if (h == Hm && w == Wm)
        hipLaunchKernelGGL(k_tta_merge<true>, grid, dim3(NTHR), 0, (hipStream_t)stream, z, C, h, w, iy, ix, Wm, flip ? 1 : 0, oy, ox, acc,
                           H, W, runs, cchunk, weight, vec);
    else
        hipLaunchKernelGGL(k_tta_merge<false>, grid, dim3(NTHR), 0, (hipStream_t)stream, z, C, h, w, iy, ix, Wm, flip ? 1 : 0, oy, ox, acc,
                           H, W, runs, cchunk, weight, vec);
    return launched("dtt_merge");
}

extern "C" int dtt_window_accum(const float *z, const float *zf, int C, int h, int w, int ch, int cw, int align_inner, float *canvas,
                                int Hc, int Wc, int h0, int w0, int wh, int ww, void *stream)
{
    if (!dtt_shape_ok(C, h, w, ch, cw, Hc, Wc)) {
        dtt_set_error("dtt_window_accum: shape not taken (dtt_supported)");
        return DTT_EINVAL;
    }
    if (!z || !canvas) {
        dtt_set_error("dtt_window_accum: a tensor is null");
        return DTT_EINVAL;
    }
    if (wh < 1 || ww < 1 || wh > ch || ww > cw || h0 < 0 || w0 < 0 || (int64_t)h0 + wh > Hc || (int64_t)w0 + ww > Wc) {
        dtt_set_error("dtt_window_accum: window [%d + %d, %d + %d] outside the %d x %d canvas or larger than the %d x %d crop", h0, wh,
                      w0, ww, Hc, Wc, ch, cw);
        return DTT_EINVAL;
    }
    int runs, cchunk;
    const dim3 grid = grid_for(wh, ww, C, &runs, &cchunk);
    const int vec = aligned16(canvas) && (Wc % RUN) == 0 && (w0 % RUN) == 0;
    const Axis ay = make_axis(h, ch, align_inner), ax = make_axis(w, cw, align_inner);
    if (zf)
        hipLaunchKernelGGL(k_tta_window<true>, grid, dim3(NTHR), 0, (hipStream_t)stream, z, zf, C, h, w, ay, ax, cw, canvas, Hc, Wc, h0,
                           w0, wh, ww, runs, cchunk, vec);
    else
        hipLaunchKernelGGL(k_tta_window<false>, grid, dim3(NTHR), 0, (hipStream_t)stream, z, zf, C, h, w, ay, ax, cw, canvas, Hc, Wc, h0,
                           w0, wh, ww, runs, cchunk, vec);
    return launched("dtt_window_accum");
}

extern "C" int dtt_canvas_merge(const float *canvas, const int32_t *rowcnt, const int32_t *colcnt, int C, int Hc, int Wc, float *acc,
                                int H, int W, int align, void *stream)
{
    if (!dtt_shape_ok(C, Hc, Wc, Hc, Wc, H, W)) {
        dtt_set_error("dtt_canvas_merge: shape not taken (dtt_supported)");
        return DTT_EINVAL;
    }
    if (!canvas || !rowcnt || !colcnt || !acc) {
        dtt_set_error("dtt_canvas_merge: a tensor is null");
        return DTT_EINVAL;
    }
    int runs, cchunk;
    const dim3 grid = grid_for(H, W, C, &runs, &cchunk);
    const int vec = aligned16(acc) && (W % RUN) == 0;
    hipLaunchKernelGGL(k_tta_canvas, grid, dim3(NTHR), 0, (hipStream_t)stream, canvas, rowcnt, colcnt, C, Hc, Wc,
                       make_axis(Hc, H, align), make_axis(Wc, W, align), acc, H, W, runs, cchunk, vec);
    return launched("dtt_canvas_merge");
}
