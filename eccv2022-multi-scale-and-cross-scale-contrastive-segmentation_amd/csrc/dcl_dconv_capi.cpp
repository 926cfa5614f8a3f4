// dcl_dconv_capi.cpp -- host-only entries of libdcl_dconv.so (include/dcl_dconv.h): error text, version, shape test, live taps,
// slab count, workspace and fragment sizes.
#include "dcl_dconv_plan.h"
#include "dcl_error.h"

DCL_DEFINE_ERROR_TEXT(ddc)

extern "C" int ddc_version(void) { return 1; }

extern "C" int ddc_supported(int N, int Ci, int Co, int H, int W, int d) { return ddc_shape_ok(N, Ci, Co, H, W, d) ? 1 : 0; }

extern "C" unsigned ddc_live_taps(int H, int W, int d) { return ddc_live_mask(H, W, d); }

extern "C" int ddc_wgrad_slabs(int N, int Ci, int Co, int H, int W, int d)
{
    return ddc_shape_ok(N, Ci, Co, H, W, d) ? ddc_slab_count(N, Ci, Co, H, W, d) : 0;
}

extern "C" int64_t ddc_workspace_bytes(int op, int N, int Ci, int Co, int H, int W, int d)
{
    return ddc_ws_bytes(op, N, Ci, Co, H, W, d);
}

extern "C" int64_t ddc_packed_bytes(int Co, int Ci, int transposed) { return ddc_pack_bytes(Co, Ci, transposed); }
