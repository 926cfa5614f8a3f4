"""ctypes binding of libdcl_eval.so (C ABI: include/dcl_eval.h), evaluation at the original label size.

A library of its own next to libdcl_hip.so, built by the same Makefile target (``_lib.build()``).  As there, a missing
library or a failed call raises: the caller decides beforehand whether the HIP path applies (utils/evaluate.py)."""
import ctypes
import os

from ._lib import CSRC_DIR, _PKG_DIR, ptr, stream_ptr  # noqa: F401  (re-exported for callers of this module)
from ._lib import load_library, raise_on_error

LIB_PATH = os.path.join(_PKG_DIR, "libdcl_eval.so")
MAX_C = 256           # DVE_MAX_C
RUN = 4               # DVE_RUN
LDS_CELLS = 4096      # DVE_LDS_CELLS

_vp = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64
_u64 = ctypes.c_uint64
_ip = ctypes.POINTER(ctypes.c_int)
_fp = ctypes.POINTER(ctypes.c_float)

# name -> argtypes (int results); mirrors include/dcl_eval.h one to one
SIGNATURES = {
    "dve_version": [],
    "dve_supported": [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i],
    "dve_evaluate": [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp],
    "dve_plan_taps": [_i, _i, _i, _i, _i, _i, _i, _ip, _fp, _ip, _fp],
    "dve_plan_hist_in_lds": [_i, _i],
    "dve_plan_runs": [_i, _u64, _ip],
    "dve_plan_class_split": [_i64, _i],
}

# device entries issued by this process (tests assert that the HIP path was taken)
calls = {"evaluate": 0}

_lib = None


def lib():
    """The loaded library; raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "dve", "original-size evaluation kernels")
    return _lib


def check(rc: int, what: str):
    raise_on_error(rc, what, lib().dve_last_error)


def supported(c: int, h: int, w: int, Hp: int, Wp: int, rh: int, rw: int, H0: int, W0: int, cols: int) -> bool:
    """Whether dve_evaluate takes z [c, h, w] -> Hp x Wp, cropped to rh x rw, -> H0 x W0 (host arithmetic only: include/dcl_eval.h)."""
    return bool(lib().dve_supported(c, h, w, Hp, Wp, rh, rw, H0, W0, cols))


def plan_taps(in_size: int, mid: int, crop: int, out: int, align_mid: bool, align_out: bool, dst: int):
    """One axis, output index dst: ((j0, j1), (m0, m1), (i00, i01, i10, i11), (l00, l01, l10, l11)): the stage-2 pair into the crop
    and its weights, then for each of the two the stage-1 pair into the input and its weights."""
    j, m, i, l = (ctypes.c_int * 2)(), (ctypes.c_float * 2)(), (ctypes.c_int * 4)(), (ctypes.c_float * 4)()
    check(lib().dve_plan_taps(in_size, mid, crop, out, 1 if align_mid else 0, 1 if align_out else 0, dst, j, m, i, l), "dve_plan_taps")
    return tuple(j), tuple(m), tuple(i), tuple(l)


def plan_hist_in_lds(c: int, cols: int) -> bool:
    return bool(lib().dve_plan_hist_in_lds(c, cols))


def plan_runs(W0: int, base: int = 0):
    """(runs per row, whether ids at byte address ``base`` is stored as 4-byte words); (0, False) on bad arguments."""
    vec = ctypes.c_int()
    runs = lib().dve_plan_runs(W0, base, ctypes.byref(vec))
    return runs, bool(vec.value) if runs > 0 else False


def plan_class_split(items: int, c: int) -> int:
    return int(lib().dve_plan_class_split(items, c))
