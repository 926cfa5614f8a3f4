// dcl_bilinear.h -- the index arithmetic of bilinear resizing, the only place it is written.  dcl_resize.hip, dcl_upce.hip,
// dcl_tta.hip, dcl_pred.hip, dcl_eval.hip, the plan exports of libdcl_tta / libdcl_pred / libdcl_eval and the host tests all call
// these functions, so that training logits, merged test-time-augmentation views, saved predictions and the evaluation at the
// original label size agree bit for bit with each other and with F.interpolate.  Host-compilable: plain functions and <math.h>, no HIP header and no library's public header (DCL_BILINEAR_HD is
// empty unless a HIP compiler reads this, where it lets the kernels call the same code, inlined).
//
// The arithmetic restates ATen's (UpSample.h: area_pixel_compute_scale / _source_index, f32):
//   align_corners: scale = (in-1)/(out-1) (0 if out == 1), src = scale * dst
//   otherwise    : scale = in/out,                         src = max(scale * (dst + 0.5) - 0.5, 0)
//   i0 = (int)src, i1 = i0 + (i0 < in-1), l1 = src - i0, l0 = 1 - l1
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define DCL_BILINEAR_HD __host__ __device__ __attribute__((always_inline))        // (= __forceinline__, without a HIP header)
#else
#define DCL_BILINEAR_HD
#endif

// ATen's area_pixel_compute_scale (f32)
DCL_BILINEAR_HD static inline float dcl_bilinear_scale(int in_size, int out_size, int align)
{
    if (align)
        return out_size > 1 ? (float)(in_size - 1) / (float)(out_size - 1) : 0.f;
    return (float)in_size / (float)out_size;
}

// ATen's area_pixel_compute_source_index + the index pair and weights of upsample_bilinear2d
DCL_BILINEAR_HD static inline void dcl_bilinear_src_index(float scale, int align, int dst, int in_size, int *i0, int *i1, float *l0,
                                                          float *l1)
{
    const float s = align ? scale * (float)dst : fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
    int a = (int)s;
    if (a > in_size - 1)
        a = in_size - 1;
    *i0 = a;
    *i1 = a + (a < in_size - 1 ? 1 : 0);
    *l1 = s - (float)a;
    *l0 = 1.f - *l1;
}

// weight of input index `i` in output index `o` along one axis (the gather-form backward's weight)
DCL_BILINEAR_HD static inline float dcl_bilinear_weight(float scale, int align, int o, int in_size, int i)
{
    int i0, i1;
    float l0, l1;
    dcl_bilinear_src_index(scale, align, o, in_size, &i0, &i1, &l0, &l1);
    return (i0 == i ? l0 : 0.f) + (i1 == i ? l1 : 0.f);
}

// candidate output range [lo, hi] touching input index i.  Conservative -- the weights decide -- and it has to be: an output with a
// non-zero dcl_bilinear_weight outside the range is a gradient term dropped without an error (tests/bilinear_main.cpp)
DCL_BILINEAR_HD static inline void dcl_bilinear_out_range(float scale, int align, int i, int in_size, int out_size, int *lo, int *hi)
{
    // src(o) is non-decreasing in o; input i is touched when src(o) in (i-1, i+1)
    const float inv = scale > 0.f ? 1.f / scale : 0.f;
    float flo, fhi;
    if (align) {
        flo = ((float)i - 1.f) * inv;
        fhi = ((float)i + 1.f) * inv;
    } else {
        flo = ((float)i - 1.f + 0.5f) * inv - 0.5f;
        fhi = ((float)i + 1.f + 0.5f) * inv - 0.5f;
    }
    *lo = (int)floorf(flo) - 1;
    *hi = (int)ceilf(fhi) + 1;
    if (scale <= 0.f) {
        *lo = 0;
        *hi = out_size - 1;
    }
    *lo = *lo < 0 ? 0 : *lo;
    *hi = *hi > out_size - 1 ? out_size - 1 : *hi;
}
