// dcl_tta_capi.cpp -- host-only entries of libdcl_tta.so (include/dcl_tta.h): error text, version, shape test, the plan exports.
#include "dcl_tta_plan.h"
#include "dcl_error.h"

DCL_DEFINE_ERROR_TEXT(dtt)

extern "C" int dtt_version(void) { return 1; }

extern "C" int dtt_supported(int C, int h, int w, int Hm, int Wm, int H, int W) { return dtt_shape_ok(C, h, w, Hm, Wm, H, W) ? 1 : 0; }

extern "C" int dtt_plan_cts_size(int H, int W, int base_size, double scale, int *new_h, int *new_w)
{
    if (H < 1 || W < 1 || base_size < 1 || !(scale > 0.0) || !(scale * base_size < 1e9) || !new_h || !new_w) {
        dtt_set_error("dtt_plan_cts_size: bad arguments");
        return DTT_EINVAL;
    }
    dtt_cts_size(H, W, base_size, scale, new_h, new_w);
    return DTT_OK;
}

extern "C" int dtt_plan_windows(int n, int crop, int stride, int cap, int *lo, int *hi, int32_t *cnt)
{
    if (n < 1 || crop < 1 || stride < 1)
        return 0;
    const int count = dtt_window_count(n, crop, stride);
    if (count < 1 || count > cap)
        return count;
    for (int r = 0; r < count; ++r)
        dtt_window(n, crop, stride, r, lo + r, hi + r);
    if (cnt)
        dtt_window_counts(n, crop, stride, cnt);
    return count;
}

extern "C" int dtt_plan_src_index(int in_size, int out_size, int align, int dst, int *i0, int *i1, float *l0, float *l1)
{
    if (in_size < 1 || out_size < 1 || dst < 0 || dst >= out_size || !i0 || !i1 || !l0 || !l1) {
        dtt_set_error("dtt_plan_src_index: bad arguments");
        return DTT_EINVAL;
    }
    dcl_bilinear_src_index(dcl_bilinear_scale(in_size, out_size, align ? 1 : 0), align ? 1 : 0, dst, in_size, i0, i1, l0, l1);
    return DTT_OK;
}
