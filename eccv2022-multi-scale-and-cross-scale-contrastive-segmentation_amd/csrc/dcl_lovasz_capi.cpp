// dcl_lovasz_capi.cpp -- host-only entries of libdcl_lovasz.so (include/dcl_lovasz.h): error text, version, workspace size.
#include "dcl_lovasz_plan.h"
#include "dcl_error.h"

DCL_DEFINE_ERROR_TEXT(dlv)

extern "C" int dlv_version(void) { return 1; }

extern "C" int64_t dlv_workspace_bytes(int N, int C, int HW, int per_image)
{
    DlvLayout lay;
    if (!dlv_layout(N, C, HW, per_image, &lay))
        return -1;
    return lay.bytes;
}
