// dcl_attn_capi.cpp -- host-only entries of libdcl_attn.so (include/dcl_attn.h): error text, version, shape test, workspace size.
#include "dcl_attn_plan.h"
#include "dcl_error.h"

DCL_DEFINE_ERROR_TEXT(dat)

extern "C" int dat_version(void) { return 1; }

extern "C" int dat_supported(int B, int N, int heads, int D) { return dat_shape_ok(B, N, heads, D) ? 1 : 0; }

extern "C" int64_t dat_workspace_bytes(int B, int N, int heads, int D, int backward)
{
    DatLayout lay;
    if (!dat_layout(B, N, heads, D, backward, &lay))
        return -1;
    return lay.bytes;
}
