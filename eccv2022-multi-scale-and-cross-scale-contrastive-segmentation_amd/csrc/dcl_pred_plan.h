// dcl_pred_plan.h -- what dcl_pred.hip, dcl_pred_capi.cpp and the host tests share: the shape tests, the run / word-store decision
// and (dcl_bilinear.h) the bilinear source index.  Host-compilable: plain functions, no HIP.
#pragma once
#include <stdint.h>

#include "../../include/dcl_pred.h"
#include "dcl_bilinear.h"

void dpr_set_error(const char *fmt, ...);

static inline bool dpr_shape_ok(int N, int C, int h, int w, int H, int W, int with_rgb)
{
    if (C < 1 || C > DPR_MAX_C || N < 1 || N > DPR_MAX_N || h < 1 || w < 1 || H < 1 || W < 1)
        return false;
    const int64_t lim = 1ll << 31;
    // (h * w and H * W are below 2^62; N * C <= 2^24 and 3 N < 2^18, so the divisions keep every product in 64 bits)
    const int64_t nc = (int64_t)N * C, no = (int64_t)N * (with_rgb ? 3 : 1);
    return (int64_t)h * w < (lim + nc - 1) / nc && (int64_t)H * W < (lim + no - 1) / no;
}

static inline bool dpr_panel_ok(int H, int W, int label_bytes)
{
    if (H < 1 || W < 1 || (label_bytes != 1 && label_bytes != 4 && label_bytes != 8))
        return false;
    return (int64_t)H * W < ((1ll << 31) + 8) / 9;
}

// runs of DPR_RUN pixels per row
static inline int dpr_runs(int W) { return (int)(((int64_t)W + DPR_RUN - 1) / DPR_RUN); }

// a run of pixel_bytes-byte pixels starts on a 4-byte boundary in every row, and is whole, when the base does and W is a multiple of
// the run: then DPR_RUN * pixel_bytes / 4 word stores replace DPR_RUN * pixel_bytes byte stores
static inline int dpr_vec_ok(uint64_t base, int W) { return (base & 3) == 0 && (W % DPR_RUN) == 0 ? 1 : 0; }

// slices the classes of a launch are split into (1, 2, 4 or 8; a workgroup of 256 threads is 256 / split runs x split slices):
// as many as bring the launch to about 2048 workgroups, every slice at least 8 classes
static inline int dpr_class_split(int64_t items, int N, int C)
{
    const int64_t blocks = ((items + 255) / 256) * N;
    int split = 1;
    while (split < 8 && blocks * split < 2048 && C / (2 * split) >= 8)
        split *= 2;
    return split;
}
