// dcl_slide_capi.cpp -- host-only entries of libdcl_slide.so (include/dcl_slide.h): error text, version, shape test, the plan exports.
#include "dcl_slide_plan.h"
#include "dcl_error.h"

DCL_DEFINE_ERROR_TEXT(dsw)

extern "C" int dsw_version(void) { return 1; }

extern "C" int dsw_supported(int Cin, int H, int W, int C, int h, int w, int wh, int ww, int R, int Q, int Hc, int Wc)
{
    return dsw_crops_ok(Cin, H, W, 1, 1, R, Q, wh, ww) && dsw_gather_ok(C, h, w, wh, ww, R, Q, Hc, Wc) ? 1 : 0;
}

extern "C" int dsw_plan_pc_windows(int n, int crop, int stride, int cap, int *lo, int *hi)
{
    if (n < 1 || crop < 1 || stride < 1)
        return 0;
    const int count = dsw_pc_window_count(n, crop, stride);
    if (count < 1 || count > cap)
        return count;
    for (int r = 0; r < count; ++r)
        dsw_pc_window(n, crop, stride, r, lo + r, hi + r);
    return count;
}

extern "C" int dsw_plan_cover(int n, int wh, const int *lo, int R, int32_t *cnt) { return dsw_cover(n, wh, lo, R, cnt); }
