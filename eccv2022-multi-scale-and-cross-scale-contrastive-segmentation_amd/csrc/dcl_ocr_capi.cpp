// dcl_ocr_capi.cpp -- host-only entries of libdcl_ocr.so (include/dcl_ocr.h): error text, version, shape test, workspace size.
#include "dcl_ocr_plan.h"
#include "dcl_error.h"

DCL_DEFINE_ERROR_TEXT(dco)

extern "C" int dco_version(void) { return 1; }

extern "C" int dco_supported(int B, int C, int K, int N) { return dco_shape_ok(B, C, K, N) ? 1 : 0; }

extern "C" int dco_splits(int B, int C, int N) { return dco_shape_ok(B, C, 1, N) ? dco_split_count(B, C, N) : 0; }

extern "C" int64_t dco_workspace_bytes(int op, int B, int C, int K, int N) { return dco_ws_bytes(op, B, C, K, N); }
