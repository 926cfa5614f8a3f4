// dcl_aug_capi.cpp -- host-only entries of libdcl_aug.so (include/dcl_aug.h): error text, version, plan test, the index-rule exports.
#include "dcl_aug_plan.h"
#include "dcl_error.h"

DCL_DEFINE_ERROR_TEXT(dau)

extern "C" int dau_version(void) { return 1; }

extern "C" int dau_supported(const dau_plan *plan) { return dau_plan_ok(plan) ? 1 : 0; }

extern "C" int dau_plan_taps(int S, int D, int o, int cap, int *k0, float *w)
{
    if (S < 1 || D < 1 || o < 0 || o >= D || !k0)
        return -1;
    const DauAxis a = dau_axis(S, D);
    int lo, hi;
    double centre;
    const double sum = dau_tap_range(a, o, &lo, &hi, &centre);
    *k0 = lo;
    if (w && hi - lo <= cap)
        for (int k = lo; k < hi; ++k)
            w[k - lo] = dau_tap_weight(a, centre, sum, k);
    return hi - lo;
}

extern "C" int dau_plan_nearest(int S, int D, int o)
{
    if (S < 1 || D < 1 || o < 0 || o >= D)
        return -1;
    return dau_nearest(S, D, o);
}
