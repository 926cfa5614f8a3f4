// dcl_pred_capi.cpp -- host-only entries of libdcl_pred.so (include/dcl_pred.h): error text, version, shape tests, the plan exports.
#include "dcl_pred_plan.h"
#include "dcl_error.h"

DCL_DEFINE_ERROR_TEXT(dpr)

extern "C" int dpr_version(void) { return 1; }

extern "C" int dpr_supported(int N, int C, int h, int w, int H, int W, int with_rgb)
{
    return dpr_shape_ok(N, C, h, w, H, W, with_rgb) ? 1 : 0;
}

extern "C" int dpr_panel_supported(int H, int W, int label_bytes) { return dpr_panel_ok(H, W, label_bytes) ? 1 : 0; }

extern "C" int dpr_plan_src_index(int in_size, int out_size, int align, int dst, int *i0, int *i1, float *l0, float *l1)
{
    if (in_size < 1 || out_size < 1 || dst < 0 || dst >= out_size || !i0 || !i1 || !l0 || !l1) {
        dpr_set_error("dpr_plan_src_index: bad arguments");
        return DPR_EINVAL;
    }
    dcl_bilinear_src_index(dcl_bilinear_scale(in_size, out_size, align ? 1 : 0), align ? 1 : 0, dst, in_size, i0, i1, l0, l1);
    return DPR_OK;
}

extern "C" int dpr_plan_runs(int W, uint64_t base, int pixel_bytes, int *vec)
{
    if (W < 1 || (pixel_bytes != 1 && pixel_bytes != 3) || !vec)
        return 0;
    *vec = dpr_vec_ok(base, W);
    return dpr_runs(W);
}
