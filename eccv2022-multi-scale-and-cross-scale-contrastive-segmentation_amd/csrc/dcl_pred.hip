// dcl_pred.hip -- prediction maps straight from the low-resolution logits (include/dcl_pred.h): the reference (managers/BaseManager.py
// save_output) resizes the logits to the image size, takes a softmax and its arg-max, and indexes two tables on the host; here one
// launch reads the [N, C, h, w] map (small: it stays in cache) and stores one to five bytes per output pixel.  The softmax is
// monotonic and is skipped.
//
// As in dcl_tta.hip a thread owns DPR_RUN = 4 consecutive output pixels of one row: it forms their tap indices and weights once,
// outside the loop over the classes, then walks the C planes with a running (max, arg-max) per pixel (torch.argmax's rule, as
// k_confusion of dcl_metrics.hip).  The taps are plain scalar loads (neighbouring lanes read neighbouring or identical addresses);
// the run is stored as 4-byte words where base and row length allow, else byte by byte.  No atomics: one thread per output byte,
// offsets in 64 bits.  Pixel items fill grid x, the images grid y.
//
// A launch with few pixels and many classes (ADE20K: 512 x 512, C = 150) would leave most of the chip idle behind 150 dependent
// steps per thread: there the classes are split over 2, 4 or 8 slices of the workgroup (dpr_class_split), every slice keeps its own
// (max, arg-max), and slice 0 folds the others in through LDS in ascending class order with the same update rule, so the first
// maximal index still wins.  No atomics, and still exactly one storing thread per output byte.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcl_pred_plan.h"

namespace {

constexpr int NTHR = 256;
constexpr int RUN = DPR_RUN;

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

// torch.argmax update rule for one candidate: replace when v > best, or when v is NaN and best is not
__device__ __forceinline__ void consider(float v, int c, float &best, int &arg)
{
    const bool take = (v > best) || (v != v && best == best);
    best = take ? v : best;
    arg = take ? c : arg;
}

// p[0 .. n) = v[0 .. n): one 4-byte store for a whole run at an aligned address, else byte by byte
__device__ __forceinline__ void store_run1(uint8_t *__restrict__ p, const uint32_t (&v)[RUN], int n, bool vec)
{
    if (vec && n == RUN) {
        *reinterpret_cast<uint32_t *>(p) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < RUN; ++k)
            if (k < n)
                p[k] = (uint8_t)v[k];
    }
}

// p[0 .. 3 n) = the three bytes of c[0 .. n) (0x00BBGGRR each): three 4-byte stores for a whole run at an aligned address
__device__ __forceinline__ void store_run3(uint8_t *__restrict__ p, const uint32_t (&c)[RUN], int n, bool vec)
{
    if (vec && n == RUN) {
        uint32_t *q = reinterpret_cast<uint32_t *>(p);
        q[0] = c[0] | (c[1] << 24);                 // R0 G0 B0 R1
        q[1] = (c[1] >> 8) | (c[2] << 16);          // G1 B1 R2 G2
        q[2] = (c[2] >> 16) | (c[3] << 8);          // B2 R3 G3 B3
    } else {
#pragma unroll
        for (int k = 0; k < RUN; ++k)
            if (k < n) {
                p[3 * k + 0] = (uint8_t)(c[k] & 255u);
                p[3 * k + 1] = (uint8_t)((c[k] >> 8) & 255u);
                p[3 * k + 2] = (uint8_t)((c[k] >> 16) & 255u);
            }
    }
}

__device__ __forceinline__ uint32_t colour(const uint8_t *__restrict__ pal, uint32_t id)
{
    const uint8_t *e = pal + 3 * id;
    return (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16);
}

// IDENT: h == H and w == W, the map is read as it is (no interpolation arithmetic: exactly torch.argmax).
// blockDim = (NTHR / split, split): thread (tx, ty) owns run blockIdx.x * blockDim.x + tx and the classes of slice ty.
template <bool IDENT>
__global__ __launch_bounds__(NTHR) void k_predict(const float *__restrict__ z, int C, int h, int w, Axis ay, Axis ax,
                                                  const uint8_t *__restrict__ lut, const uint8_t *__restrict__ pal,
                                                  uint8_t *__restrict__ ids, uint8_t *__restrict__ mapped, uint8_t *__restrict__ rgb,
                                                  int H, int W, int runs, int cchunk, int vec_z, int vec_ids, int vec_mapped,
                                                  int vec_rgb)
{
    __shared__ float s_best[NTHR * RUN];
    __shared__ int s_arg[NTHR * RUN];
    const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = item < (int64_t)H * runs;
    const int Y = active ? (int)(item / runs) : 0, X0 = active ? (int)(item - (int64_t)Y * runs) * RUN : 0;
    const int n = min(RUN, W - X0);
    const int c0 = threadIdx.y * cchunk, c1 = min(C, c0 + cchunk);
    const int64_t plane = (int64_t)h * w;
    const float *__restrict__ zn = z + (int64_t)blockIdx.y * C * plane;
    float best[RUN] = {0.f, 0.f, 0.f, 0.f};
    int arg[RUN] = {c0, c0, c0, c0};
    if (active && c0 < c1) {
        if (IDENT) {
            const float *__restrict__ p = zn + (int64_t)Y * w + X0;
            if (vec_z && n == RUN) {
                float4 v = *reinterpret_cast<const float4 *>(p + (int64_t)c0 * plane);
                best[0] = v.x, best[1] = v.y, best[2] = v.z, best[3] = v.w;
                for (int c = c0 + 1; c < c1; ++c) {
                    v = *reinterpret_cast<const float4 *>(p + (int64_t)c * plane);
                    consider(v.x, c, best[0], arg[0]);
                    consider(v.y, c, best[1], arg[1]);
                    consider(v.z, c, best[2], arg[2]);
                    consider(v.w, c, best[3], arg[3]);
                }
            } else {
                int off[RUN];
#pragma unroll
                for (int k = 0; k < RUN; ++k) {
                    off[k] = min(k, n - 1);             // columns past the row's end repeat its last one (never stored)
                    best[k] = p[(int64_t)c0 * plane + off[k]];
                }
                for (int c = c0 + 1; c < c1; ++c) {
                    const float *__restrict__ pc = p + (int64_t)c * plane;
#pragma unroll
                    for (int k = 0; k < RUN; ++k)
                        consider(pc[off[k]], c, best[k], arg[k]);
                }
            }
        } else {
            Tap ty = tap(ay, Y);
            ty.i0 *= w, ty.i1 *= w;
            Tap tx[RUN];
#pragma unroll
            for (int k = 0; k < RUN; ++k)
                tx[k] = tap(ax, min(X0 + k, W - 1));
            for (int c = c0; c < c1; ++c) {
                const float *__restrict__ zc = zn + (int64_t)c * plane;
#pragma unroll
                for (int k = 0; k < RUN; ++k) {
                    const Tap t = tx[k];
                    const float v = ty.l0 * (t.l0 * zc[ty.i0 + t.i0] + t.l1 * zc[ty.i0 + t.i1]) +
                                    ty.l1 * (t.l0 * zc[ty.i1 + t.i0] + t.l1 * zc[ty.i1 + t.i1]);
                    if (c == c0)
                        best[k] = v;
                    else
                        consider(v, c, best[k], arg[k]);
                }
            }
        }
    }
    if (blockDim.y > 1) {                           // (uniform over the workgroup: every thread reaches the barrier)
        const int slot = (threadIdx.y * blockDim.x + threadIdx.x) * RUN;
        if (threadIdx.y > 0) {
#pragma unroll
            for (int k = 0; k < RUN; ++k)
                s_best[slot + k] = best[k], s_arg[slot + k] = arg[k];
        }
        __syncthreads();
        if (threadIdx.y > 0)
            return;
        for (int s = 1; s < (int)blockDim.y; ++s) {
            if (s * cchunk >= C)                    // a slice without classes holds nothing
                break;
            const int o = (s * blockDim.x + threadIdx.x) * RUN;
#pragma unroll
            for (int k = 0; k < RUN; ++k)
                consider(s_best[o + k], s_arg[o + k], best[k], arg[k]);
        }
    }
    if (!active)
        return;
    const int64_t o = ((int64_t)blockIdx.y * H + Y) * W + X0;
    uint32_t v[RUN];
#pragma unroll
    for (int k = 0; k < RUN; ++k)
        v[k] = (uint32_t)arg[k];
    store_run1(ids + o, v, n, vec_ids != 0);
    if (mapped) {
        uint32_t m[RUN];
#pragma unroll
        for (int k = 0; k < RUN; ++k)
            m[k] = lut[v[k]];
        store_run1(mapped + o, m, n, vec_mapped != 0);
    }
    if (rgb) {
        uint32_t c3[RUN];
#pragma unroll
        for (int k = 0; k < RUN; ++k)
            c3[k] = colour(pal, v[k]);
        store_run3(rgb + 3 * o, c3, n, vec_rgb != 0);
    }
}

__device__ __forceinline__ int load_label(const void *t, int tbytes, int64_t i)
{
    if (tbytes == 8) {
        const long long v = ((const long long *)t)[i];
        return (v < 0 || v > 255) ? -1 : (int)v;
    }
    if (tbytes == 4)
        return ((const int *)t)[i];
    return (int)((const unsigned char *)t)[i];
}

struct Norm {
    float mean[3], std[3];
};

// item = (row, panel, run): panel 0 the image, 1 the label's colours, 2 the prediction's
__global__ __launch_bounds__(NTHR) void k_panel(const float *__restrict__ img, const void *__restrict__ label, int lbytes,
                                                const uint8_t *__restrict__ ids, const uint8_t *__restrict__ pal, int H, int W, Norm nm,
                                                int label_ignore, int ids_ignore, uint8_t *__restrict__ out, int runs, int vec)
{
    const int64_t item = (int64_t)blockIdx.x * NTHR + threadIdx.x;
    if (item >= (int64_t)H * 3 * runs)
        return;
    const int Y = (int)(item / (3 * runs)), r = (int)(item - (int64_t)Y * 3 * runs);
    const int panel = r / runs, X0 = (r - panel * runs) * RUN;
    const int n = min(RUN, W - X0);
    const int64_t plane = (int64_t)H * W, pix = (int64_t)Y * W + X0;
    uint32_t c3[RUN];
#pragma unroll
    for (int k = 0; k < RUN; ++k) {
        const int64_t i = pix + min(k, n - 1);
        if (panel == 0) {
            uint32_t c = 0;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float p = img[ch * plane + i] * nm.std[ch];
                asm volatile("" : "+v"(p));         // product and sum are rounded separately (the torch composition's two operations)
                const float u = fminf(fmaxf(p + nm.mean[ch], 0.f), 1.f);
                c |= (uint32_t)rintf(u * 255.f) << (8 * ch);
            }
            c3[k] = c;
        } else if (panel == 1) {
            const int t = load_label(label, lbytes, i);
            c3[k] = (t < 0 || t > 255 || t == label_ignore) ? 0u : colour(pal, (uint32_t)t);
        } else {
            const int t = ids[i];
            c3[k] = t == ids_ignore ? 0u : colour(pal, (uint32_t)t);
        }
    }
    store_run3(out + 3 * ((int64_t)Y * 3 * W + (int64_t)panel * W + X0), c3, n, vec != 0);
}

int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        dpr_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return DPR_OK;
}

}  // namespace

extern "C" int dpr_predict(const float *z, int N, int C, int h, int w, int H, int W, int align_corners, const uint8_t *lut,
                           const uint8_t *palette, uint8_t *ids, uint8_t *mapped, uint8_t *rgb, void *stream)
{
    if (!dpr_shape_ok(N, C, h, w, H, W, rgb ? 1 : 0)) {
        dpr_set_error("dpr_predict: shape not taken (dpr_supported)");
        return DPR_EINVAL;
    }
    if (!z || !ids) {
        dpr_set_error("dpr_predict: a tensor is null");
        return DPR_EINVAL;
    }
    if ((lut == nullptr) != (mapped == nullptr) || (palette == nullptr) != (rgb == nullptr)) {
        dpr_set_error("dpr_predict: a table without its output, or an output without its table");
        return DPR_EINVAL;
    }
    const int runs = dpr_runs(W);
    const int split = dpr_class_split((int64_t)H * runs, N, C), cchunk = (C + split - 1) / split;
    const dim3 block(NTHR / split, split);
    const dim3 grid((unsigned)(((int64_t)H * runs + block.x - 1) / block.x), (unsigned)N);
    const int vec_z = ((uintptr_t)z & 15) == 0 && (W % RUN) == 0;
    const int v1 = dpr_vec_ok((uintptr_t)ids, W), v2 = mapped ? dpr_vec_ok((uintptr_t)mapped, W) : 0;
    const int v3 = rgb ? dpr_vec_ok((uintptr_t)rgb, W) : 0;
    const Axis ay = make_axis(h, H, align_corners), ax = make_axis(w, W, align_corners);
    if (h == H && w == W)
        hipLaunchKernelGGL(k_predict<true>, grid, block, 0, (hipStream_t)stream, z, C, h, w, ay, ax, lut, palette, ids, mapped, rgb, H, W,
                           runs, cchunk, vec_z, v1, v2, v3);
    else
        hipLaunchKernelGGL(k_predict<false>, grid, block, 0, (hipStream_t)stream, z, C, h, w, ay, ax, lut, palette, ids, mapped, rgb, H, W,
                           runs, cchunk, vec_z, v1, v2, v3);
    return launched("dpr_predict");
}

extern "C" int dpr_panel(const float *img, const void *label, int label_bytes, const uint8_t *ids, const uint8_t *palette, int H,
                         int W, float mean0, float mean1, float mean2, float std0, float std1, float std2, int label_ignore,
                         int ids_ignore, uint8_t *panel, void *stream)
{
    if (!dpr_panel_ok(H, W, label_bytes)) {
        dpr_set_error("dpr_panel: shape not taken (dpr_panel_supported)");
        return DPR_EINVAL;
    }
    if (!img || !label || !ids || !palette || !panel) {
        dpr_set_error("dpr_panel: a tensor is null");
        return DPR_EINVAL;
    }
    const int runs = dpr_runs(W);
    const dim3 grid((unsigned)(((int64_t)H * 3 * runs + NTHR - 1) / NTHR));
    Norm nm = {{mean0, mean1, mean2}, {std0, std1, std2}};
    hipLaunchKernelGGL(k_panel, grid, dim3(NTHR), 0, (hipStream_t)stream, img, label, label_bytes, ids, palette, H, W, nm, label_ignore,
                       ids_ignore, panel, runs, dpr_vec_ok((uintptr_t)panel, W));
    return launched("dpr_panel");
}
