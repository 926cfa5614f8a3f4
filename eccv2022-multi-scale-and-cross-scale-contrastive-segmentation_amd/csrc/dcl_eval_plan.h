// dcl_eval_plan.h -- what dcl_eval.hip, dcl_eval_capi.cpp and the host tests share: the shape test, the two-stage taps of one axis,
// the run / word-store decision, the histogram rule and the class split.  Host-compilable: plain functions, no HIP.
#pragma once
#include <stdint.h>

#include "../../include/dcl_eval.h"
#include "dcl_bilinear.h"

void dve_set_error(const char *fmt, ...);

static inline bool dve_shape_ok(int C, int h, int w, int Hp, int Wp, int rh, int rw, int H0, int W0, int cols)
{
    if (C < 1 || C > DVE_MAX_C || cols < C || cols > C + 1)
        return false;
    if (h < 1 || w < 1 || Hp < 1 || Wp < 1 || rh < 1 || rw < 1 || H0 < 1 || W0 < 1)
        return false;
    // (every product of two sizes is below 2^62, so the division keeps the test in 64 bits; C >= 1 covers H0 * W0 itself)
    const int64_t lim = ((1ll << 31) + C - 1) / C;
    return (int64_t)h * w < lim && (int64_t)Hp * Wp < lim && (int64_t)H0 * W0 < lim;
}

// One stage of one axis: output index dst of a resize from in_size to out_size; equal sizes are the identity (q, q; 1, 0)
struct DveTap {
    int i0, i1;
    float l0, l1;
};

DCL_BILINEAR_HD static inline DveTap dve_tap(int in_size, int out_size, float scale, int align, int dst)
{
    DveTap t;
    if (in_size == out_size) {
        t.i0 = t.i1 = dst;
        t.l0 = 1.f;
        t.l1 = 0.f;
    } else {
        dcl_bilinear_src_index(scale, align, dst, in_size, &t.i0, &t.i1, &t.l0, &t.l1);
    }
    return t;
}

// runs of DVE_RUN pixels per row
static inline int dve_runs(int W0) { return (int)(((int64_t)W0 + DVE_RUN - 1) / DVE_RUN); }

// a run of ids starts on a 4-byte boundary in every row, and is whole, when the base does and W0 is a multiple of the run: then one
// word store replaces DVE_RUN byte stores
static inline int dve_vec_ok(uint64_t base, int W0) { return (base & 3) == 0 && (W0 % DVE_RUN) == 0 ? 1 : 0; }

static inline int dve_hist_in_lds(int C, int cols) { return (int64_t)C * cols <= DVE_LDS_CELLS ? 1 : 0; }

// slices the classes are split into (1, 2, 4 or 8; a workgroup of 256 threads is 256 / split runs x split slices): as many as
// bring the launch to about 2048 workgroups, every slice at least 8 classes
static inline int dve_class_split(int64_t items, int C)
{
    const int64_t blocks = (items + 255) / 256;
    int split = 1;
    while (split < 8 && blocks * split < 2048 && C / (2 * split) >= 8)
        split *= 2;
    return split;
}
