// dcl_ohem_capi.cpp -- host-only entries of libdcl_ohem.so (include/dcl_ohem.h): error text, version, shape test, the plan exports.
#include "dcl_ohem_plan.h"
#include "dcl_error.h"

DCL_DEFINE_ERROR_TEXT(doh)

extern "C" int doh_version(void) { return 1; }

extern "C" int doh_supported(int N, int C, int h, int w, int H, int W) { return doh_shape_ok(N, C, h, w, H, W) ? 1 : 0; }

extern "C" int64_t doh_workspace_bytes(int N, int H) { return doh_ws_bytes(N, H); }

extern "C" int doh_plan_layout(int *off, int *bins)
{
    if (!off || !bins) {
        doh_set_error("doh_plan_layout: null pointer");
        return DOH_EINVAL;
    }
    for (int pass = 0; pass < DOH_PASSES; ++pass) {
        off[pass] = doh_ws_hist(pass);
        bins[pass] = doh_bins(pass);
    }
    off[3] = DOH_WS_STATE;
    off[4] = DOH_WS_PART;
    return DOH_OK;
}
