// dcl_eval.hip -- evaluation at the original label size (include/dcl_eval.h): the reference (managers/HRNet_Manager.py
// post_process_output) slices the fit_stride padding off the full-size logits, resizes them to the image's original size, and its
// confusion matrix takes their arg-max against the label map that was never resized.  Here one launch reads the [C, h, w] map and
// leaves one byte per original pixel and the counts; neither the [C, Hp, Wp] nor the [C, H0, W0] map exists.
//
// The direct form, on the shape of dcl_pred.hip: a thread owns DVE_RUN = 4 consecutive output pixels of one row.  Outside the loop
// over the classes it forms the stage-2 taps (into the crop: 2 rows, 8 columns) and, for those rows and columns, the stage-1 taps
// (into the input); per class it evaluates the 2 x 8 stage-1 values (each rounded to f32: the value a caller would read from the
// materialised map) and from them its 4 outputs, with a running (max, arg-max) per pixel.  That is 16 scalar loads per pixel and
// class, all within a few cache lines of its neighbours'; the input map is small and stays in cache.  A stage whose sizes are
// equal is compiled out (ID1, ID2): its values are read as they are, which is what makes the identity bitwise (0 * Inf).
//
// Few pixels and many classes (ADE20K: 375 x 500, C = 150): the classes are split over 2, 4 or 8 slices of the workgroup, as in
// dcl_pred.hip; slice 0 folds the others in through LDS in ascending class order, so the first maximal index still wins.
//
// The confusion matrix is the histogram half of k_confusion_pred (dcl_metrics.hip), fed from registers: the storing thread loads
// its run's labels, merges equal neighbouring (prediction, target) pairs of the run, and adds them to the workgroup's LDS
// histogram (flushed once, non-empty cells only) while C * cols <= DVE_LDS_CELLS, else to the matrix itself.  Integer atomics only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcl_eval_plan.h"

namespace {

constexpr int NTHR = 256;
constexpr int RUN = DVE_RUN;

struct Axis {
    float scale;
    int align;
    int in, out;
};

struct Args {
    const float *z;             // [C, h, w]
    int C, h, w;
    Axis y1, x1;                // stage 1: (h, w) -> (Hp, Wp)
    Axis y2, x2;                // stage 2: (rh, rw) -> (H0, W0)
    int H0, W0, runs, cchunk;
    const void *label;          // [H0, W0] or null
    int lbytes;
    const uint8_t *lut;         // uint8[256] or null
    int cols;
    int *cm, *oob;
    uint8_t *ids;               // [H0, W0] or null
    int vec_ids, hist_lds;
};

Axis make_axis(int in_size, int out_size, int align)
{
    Axis a;
    a.align = align ? 1 : 0;
    a.in = in_size;
    a.out = out_size;
    a.scale = dcl_bilinear_scale(in_size, out_size, a.align);
    return a;
}

__device__ __forceinline__ DveTap tap(const Axis a, int dst) { return dve_tap(a.in, a.out, a.scale, a.align, dst); }

// torch.argmax update rule for one candidate: replace when v > best, or when v is NaN and best is not
__device__ __forceinline__ void consider(float v, int c, float &best, int &arg)
{
    const bool take = (v > best) || (v != v && best == best);
    best = take ? v : best;
    arg = take ? c : arg;
}

__device__ __forceinline__ int load_label(const void *t, int tbytes, int64_t i)
{
    if (tbytes == 8) {
        const long long v = ((const long long *)t)[i];
        return (v < 0 || v > 0x7fffffff) ? -1 : (int)v;
    }
    if (tbytes == 4)
        return ((const int *)t)[i];
    return (int)((const unsigned char *)t)[i];
}

// ID1: (h, w) == (Hp, Wp), the input is the stage-1 map.  ID2: (rh, rw) == (H0, W0), the crop is the output.
// blockDim = (NTHR / split, split): thread (tx, ty) owns run blockIdx.x * blockDim.x + tx and the classes of slice ty.
template <bool ID1, bool ID2>
__global__ __launch_bounds__(NTHR) void k_evaluate(const Args a)
{
    constexpr int NR = ID2 ? 1 : 2, NC = ID2 ? RUN : 2 * RUN;      // stage-1 rows and columns a run needs
    __shared__ float s_best[NTHR * RUN];
    __shared__ int s_arg[NTHR * RUN];
    __shared__ int hist[DVE_LDS_CELLS];
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    const int cells = a.C * a.cols;
    const bool lds = a.label != nullptr && a.hist_lds;             // (uniform over the launch)
    if (lds)
        for (int i = tid; i < cells; i += NTHR)
            hist[i] = 0;
    const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = item < (int64_t)a.H0 * a.runs;
    const int Y = active ? (int)(item / a.runs) : 0, X0 = active ? (int)(item - (int64_t)Y * a.runs) * RUN : 0;
    const int n = min(RUN, a.W0 - X0);
    const int c0 = threadIdx.y * a.cchunk, c1 = min(a.C, c0 + a.cchunk);
    const int64_t plane = (int64_t)a.h * a.w;
    float best[RUN] = {0.f, 0.f, 0.f, 0.f};
    int arg[RUN] = {c0, c0, c0, c0};
    if (active && c0 < c1) {
        // stage 2: rows ry[] and columns cx[] of the crop (all below rh, rw: the taps clamp at the crop's last index)
        int ry[NR], cx[NC];
        DveTap t2y = {0, 0, 1.f, 0.f}, t2x[RUN];
        if (ID2) {
            ry[0] = Y;
#pragma unroll
            for (int k = 0; k < RUN; ++k)
                cx[k] = min(X0 + k, a.W0 - 1);                     // columns past the row's end repeat its last one (never stored)
        } else {
            t2y = tap(a.y2, Y);
            ry[0] = t2y.i0, ry[NR - 1] = t2y.i1;
#pragma unroll
            for (int k = 0; k < RUN; ++k) {
                t2x[k] = tap(a.x2, min(X0 + k, a.W0 - 1));
                cx[(NC / RUN) * k] = t2x[k].i0, cx[(NC / RUN) * k + NC / RUN - 1] = t2x[k].i1;
            }
        }
        // stage 1: for those rows and columns, the taps into the input (row offsets in elements)
        DveTap r1[NR], q1[NC];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            r1[r] = tap(a.y1, ry[r]);
            r1[r].i0 *= a.w, r1[r].i1 *= a.w;
        }
#pragma unroll
        for (int j = 0; j < NC; ++j)
            q1[j] = tap(a.x1, cx[j]);
        for (int c = c0; c < c1; ++c) {
            const float *__restrict__ zc = a.z + (int64_t)c * plane;
            float s[NR][NC];
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
                for (int j = 0; j < NC; ++j) {
                    if (ID1)
                        s[r][j] = zc[r1[r].i0 + q1[j].i0];
                    else
                        s[r][j] = r1[r].l0 * (q1[j].l0 * zc[r1[r].i0 + q1[j].i0] + q1[j].l1 * zc[r1[r].i0 + q1[j].i1]) +
                                  r1[r].l1 * (q1[j].l0 * zc[r1[r].i1 + q1[j].i0] + q1[j].l1 * zc[r1[r].i1 + q1[j].i1]);
                }
#pragma unroll
            for (int k = 0; k < RUN; ++k) {
                float v;
                if (ID2)
                    v = s[0][k];
                else
                    v = t2y.l0 * (t2x[k].l0 * s[0][(NC / RUN) * k] + t2x[k].l1 * s[0][(NC / RUN) * k + NC / RUN - 1]) +
                        t2y.l1 * (t2x[k].l0 * s[NR - 1][(NC / RUN) * k] + t2x[k].l1 * s[NR - 1][(NC / RUN) * k + NC / RUN - 1]);
                if (c == c0)
                    best[k] = v;
                else
                    consider(v, c, best[k], arg[k]);
            }
        }
    }
    if (threadIdx.y > 0) {
        const int slot = tid * RUN;
#pragma unroll
        for (int k = 0; k < RUN; ++k)
            s_best[slot + k] = best[k], s_arg[slot + k] = arg[k];
    }
    __syncthreads();                                               // the slices' results, and the zeroed histogram
    if (active && threadIdx.y == 0) {
        for (int sl = 1; sl < (int)blockDim.y; ++sl) {
            if (sl * a.cchunk >= a.C)                              // a slice without classes holds nothing
                break;
            const int o = (sl * blockDim.x + threadIdx.x) * RUN;
#pragma unroll
            for (int k = 0; k < RUN; ++k)
                consider(s_best[o + k], s_arg[o + k], best[k], arg[k]);
        }
        const int64_t o = (int64_t)Y * a.W0 + X0;
        if (a.ids) {
            uint8_t *__restrict__ p = a.ids + o;
            if (a.vec_ids && n == RUN) {
                *reinterpret_cast<uint32_t *>(p) =
                    (uint32_t)arg[0] | ((uint32_t)arg[1] << 8) | ((uint32_t)arg[2] << 16) | ((uint32_t)arg[3] << 24);
            } else {
#pragma unroll
                for (int k = 0; k < RUN; ++k)
                    if (k < n)
                        p[k] = (uint8_t)arg[k];
            }
        }
        if (a.label) {
            int key[RUN + 1], bad = 0;
#pragma unroll
            for (int k = 0; k < RUN; ++k) {
                key[k] = -1;
                if (k < n) {
                    int t = load_label(a.label, a.lbytes, o + k);
                    if (a.lut)
                        t = a.lut[t & 255];                        // (label_bytes == 1: t is a byte)
                    if ((unsigned)t < (unsigned)a.cols)
                        key[k] = arg[k] * a.cols + t;
                    else
                        ++bad;
                }
            }
            key[RUN] = -1;
            int *__restrict__ dst = lds ? hist : a.cm;
            int cnt = 0;
#pragma unroll
            for (int k = 0; k < RUN; ++k)
                if (key[k] >= 0) {
                    ++cnt;
                    if (key[k + 1] != key[k]) {                    // equal neighbours of the run go as one addition
                        atomicAdd(dst + key[k], cnt);
                        cnt = 0;
                    }
                }
            if (bad)
                atomicAdd(a.oob, bad);
        }
    }
    if (lds) {
        __syncthreads();
        for (int i = tid; i < cells; i += NTHR)
            if (hist[i])
                atomicAdd(a.cm + i, hist[i]);
    }
}

}  // namespace

extern "C" int dve_evaluate(const float *z, int C, int h, int w, int Hp, int Wp, int align_mid, int rh, int rw, int H0, int W0,
                            int align_out, const void *label, int label_bytes, const uint8_t *label_lut, int cols, int32_t *cm,
                            int32_t *oob, uint8_t *ids, void *stream)
{
    if (!dve_shape_ok(C, h, w, Hp, Wp, rh, rw, H0, W0, cols)) {
        dve_set_error("dve_evaluate: shape not taken (dve_supported)");
        return DVE_EINVAL;
    }
    if (rh > Hp || rw > Wp) {
        dve_set_error("dve_evaluate: the crop %d x %d is larger than the stage-1 map %d x %d", rh, rw, Hp, Wp);
        return DVE_EINVAL;
    }
    if (!z) {
        dve_set_error("dve_evaluate: the logits are null");
        return DVE_EINVAL;
    }
    if ((label != nullptr) != (cm != nullptr) || (cm != nullptr) != (oob != nullptr)) {
        dve_set_error("dve_evaluate: a label without cm and oob, or cm / oob without a label");
        return DVE_EINVAL;
    }
    if (!cm && !ids) {
        dve_set_error("dve_evaluate: neither cm nor ids: nothing to do");
        return DVE_EINVAL;
    }
    if (label && label_bytes != 1 && label_bytes != 4 && label_bytes != 8) {
        dve_set_error("dve_evaluate: label_bytes must be 1, 4 or 8");
        return DVE_EINVAL;
    }
    if (label_lut && (!label || label_bytes != 1)) {
        dve_set_error("dve_evaluate: label_lut needs a uint8 label (label_bytes == 1)");
        return DVE_EINVAL;
    }
    Args a;
    a.z = z, a.C = C, a.h = h, a.w = w;
    a.y1 = make_axis(h, Hp, align_mid), a.x1 = make_axis(w, Wp, align_mid);
    a.y2 = make_axis(rh, H0, align_out), a.x2 = make_axis(rw, W0, align_out);
    a.H0 = H0, a.W0 = W0, a.runs = dve_runs(W0);
    const int64_t items = (int64_t)H0 * a.runs;
    const int split = dve_class_split(items, C);
    a.cchunk = (C + split - 1) / split;
    a.label = label, a.lbytes = label_bytes, a.lut = label_lut, a.cols = cols, a.cm = cm, a.oob = oob, a.ids = ids;
    a.vec_ids = ids ? dve_vec_ok((uintptr_t)ids, W0) : 0;
    a.hist_lds = dve_hist_in_lds(C, cols);
    const dim3 block(NTHR / split, split);
    const dim3 grid((unsigned)((items + block.x - 1) / block.x));
    const bool id1 = h == Hp && w == Wp, id2 = rh == H0 && rw == W0;
    hipStream_t st = (hipStream_t)stream;
    if (id1 && id2)
        hipLaunchKernelGGL((k_evaluate<true, true>), grid, block, 0, st, a);
    else if (id1)
        hipLaunchKernelGGL((k_evaluate<true, false>), grid, block, 0, st, a);
    else if (id2)
        hipLaunchKernelGGL((k_evaluate<false, true>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((k_evaluate<false, false>), grid, block, 0, st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        dve_set_error("dve_evaluate: launch failed: %s", hipGetErrorString(e));
        return (int)e;
    }
    return DVE_OK;
}
