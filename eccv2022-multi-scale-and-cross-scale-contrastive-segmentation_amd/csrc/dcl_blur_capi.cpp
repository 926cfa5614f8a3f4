// dcl_blur_capi.cpp -- host-only entries of libdcl_blur.so (include/dcl_blur.h): error text, version, the limits, the box of a radius.
#include "dcl_blur_plan.h"
#include "dcl_error.h"

DCL_DEFINE_ERROR_TEXT(dbl)

extern "C" int dbl_version(void) { return 1; }

extern "C" int dbl_supported(int C, int h, int w, int radius) { return dbl_blur_ok(C, h, w, radius) ? 1 : 0; }

extern "C" int dbl_box(int radius, int *l, float *ww, float *fw)
{
    if (radius < 1 || radius > DBL_MAX_RADIUS || !l || !ww || !fw)
        return DBL_EINVAL;
    const DblBox b = dbl_box_of(radius);
    *l = b.l;
    *ww = b.ww;
    *fw = b.fw;
    return DBL_OK;
}
