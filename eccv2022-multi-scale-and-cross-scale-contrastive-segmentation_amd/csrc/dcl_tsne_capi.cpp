// dcl_tsne_capi.cpp -- host-only entries of libdcl_tsne.so (include/dcl_tsne.h): error text, version, shape test, the plan exports.
#include "dcl_tsne_plan.h"
#include "dcl_error.h"

DCL_DEFINE_ERROR_TEXT(dts)

extern "C" int dts_version(void) { return 1; }

extern "C" int dts_supported(int64_t N, int D, double perplexity) { return dts_shape_ok(N, D, perplexity) ? 1 : 0; }

static bool n_ok(int N) { return N >= 2 && (int64_t)N * N < (1ll << 31); }

extern "C" int dts_plan_row_in_lds(int N) { return n_ok(N) ? dts_row_in_lds(N) : 0; }
extern "C" int dts_plan_sym_groups(int N) { return n_ok(N) ? dts_sym_groups(N) : 0; }
extern "C" int dts_plan_z_parts(int N) { return n_ok(N) ? dts_z_parts(N) : 0; }
extern "C" int dts_plan_grad_groups(int N) { return n_ok(N) ? dts_grad_groups(N) : 0; }
extern "C" int dts_plan_upd_groups(int N) { return n_ok(N) ? dts_upd_groups(N) : 0; }
extern "C" int dts_plan_grad_vec(uint64_t p_base, int N) { return n_ok(N) ? dts_grad_vec(p_base, N) : 0; }
extern "C" int64_t dts_plan_ws_floats(int N) { return n_ok(N) ? dts_ws_floats(N) : 0; }
extern "C" int dts_plan_kl_slots(int n_iter) { return dts_kl_slots(n_iter); }
