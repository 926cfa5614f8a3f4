// dcl_convbwd_capi.cpp -- host-only entries of libdcl_convbwd.so (include/dcl_convbwd.h): error text, version, shape test, plan.
#include "dcl_convbwd_plan.h"
#include "dcl_error.h"

DCL_DEFINE_ERROR_TEXT(dcb)

// The shared headers (dcl_common.h: DCL_CHECK_ARG, DCL_LAUNCH_CHECK) report through the main library's names: this library's own
// definitions, writing the same per-thread text.  (The kernel-name trace is the main library's: nothing to note here.)
void dcl_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
void dcl_note_kernel(const char *, ...) {}

extern "C" int dcb_version(void) { return 1; }

extern "C" int dcb_supported(int N, int Cin, int Cout, int H, int W, int pre)
{
    (void)pre;          // the PRE forms serve the same shapes
    return dcb_shape_ok(N, Cin, Cout, H, W) ? 1 : 0;
}

extern "C" int dcb_plan(int N, int Cin, int Cout, int H, int W, int tile_r, int tile_p, int wg_target, int *out)
{
    if (!out) {
        dcb_set_error("dcb_plan: null pointer");
        return DCL_EINVAL;
    }
    const DcbPlan d = dcb_make_plan(N, Cin, Cout, H, W, tile_r, tile_p, wg_target);
    if (!d.ok) {
        dcb_set_error("dcb_plan: shape, tile or workgroup target not taken");
        return DCL_EUNSUPPORTED;
    }
    out[0] = (int)d.nd;
    out[1] = (int)d.nd8;
    out[2] = (int)d.w.grid;
    out[3] = d.w.slabs;
    out[4] = d.w.wave_mode;
    out[5] = d.R;
    out[6] = d.P;
    out[7] = d.target;
    return 0;
}

extern "C" int dcb_wgrad_splits(int N, int Cin, int Cout, int H, int W, int tile_r, int tile_p, int wg_target)
{
    const DcbPlan d = dcb_make_plan(N, Cin, Cout, H, W, tile_r, tile_p, wg_target);
    return d.ok ? d.w.slabs : 0;
}
