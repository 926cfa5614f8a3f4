// dcl_lovasz_capi.cpp -- host-only entries of libdcl_lovasz.so (include/dcl_lovasz.h): error text, version, workspace size.
#include <stdarg.h>
#include <stdio.h>

#include "dcl_lovasz_plan.h"

static thread_local char g_err[512] = "";

void dlv_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char *dlv_last_error(void) { return g_err; }

extern "C" int dlv_version(void) { return 1; }

extern "C" int64_t dlv_workspace_bytes(int N, int C, int HW, int per_image)
{
    DlvLayout lay;
    if (!dlv_layout(N, C, HW, per_image, &lay))
        return -1;
    return lay.bytes;
}
