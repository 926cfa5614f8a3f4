// dcl_eval_capi.cpp -- host-only entries of libdcl_eval.so (include/dcl_eval.h): error text, version, shape test, the plan exports.
#include "dcl_eval_plan.h"
#include "dcl_error.h"

DCL_DEFINE_ERROR_TEXT(dve)

extern "C" int dve_version(void) { return 1; }

extern "C" int dve_supported(int C, int h, int w, int Hp, int Wp, int rh, int rw, int H0, int W0, int cols)
{
    return dve_shape_ok(C, h, w, Hp, Wp, rh, rw, H0, W0, cols) ? 1 : 0;
}

extern "C" int dve_plan_taps(int in_size, int mid, int crop, int out, int align_mid, int align_out, int dst, int *j, float *m, int *i,
                             float *l)
{
    if (in_size < 1 || mid < 1 || crop < 1 || crop > mid || out < 1 || dst < 0 || dst >= out || !j || !m || !i || !l) {
        dve_set_error("dve_plan_taps: bad arguments");
        return DVE_EINVAL;
    }
    const int a1 = align_mid ? 1 : 0, a2 = align_out ? 1 : 0;
    const DveTap t2 = dve_tap(crop, out, dcl_bilinear_scale(crop, out, a2), a2, dst);
    j[0] = t2.i0, j[1] = t2.i1, m[0] = t2.l0, m[1] = t2.l1;
    const float s1 = dcl_bilinear_scale(in_size, mid, a1);
    for (int k = 0; k < 2; ++k) {
        const DveTap t1 = dve_tap(in_size, mid, s1, a1, j[k]);
        i[2 * k] = t1.i0, i[2 * k + 1] = t1.i1, l[2 * k] = t1.l0, l[2 * k + 1] = t1.l1;
    }
    return DVE_OK;
}

extern "C" int dve_plan_hist_in_lds(int C, int cols) { return dve_hist_in_lds(C, cols); }

extern "C" int dve_plan_runs(int W0, uint64_t base, int *vec)
{
    if (W0 < 1 || !vec)
        return 0;
    *vec = dve_vec_ok(base, W0);
    return dve_runs(W0);
}

extern "C" int dve_plan_class_split(int64_t items, int C) { return dve_class_split(items, C); }
