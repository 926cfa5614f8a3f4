"""ctypes binding of libdcl_pred.so (C ABI: include/dcl_pred.h), prediction maps from logits.

A library of its own next to libdcl_hip.so, built by the same Makefile target (``_lib.build()``).  As there, a missing
library or a failed call raises: the caller decides beforehand whether the HIP path applies (utils/predict.py)."""
import ctypes
import os

from ._lib import CSRC_DIR, _PKG_DIR, ptr, stream_ptr  # noqa: F401  (re-exported for callers of this module)
from ._lib import load_library, raise_on_error

LIB_PATH = os.path.join(_PKG_DIR, "libdcl_pred.so")
MAX_C = 256           # DPR_MAX_C
MAX_N = 65535         # DPR_MAX_N
RUN = 4               # DPR_RUN

_vp = ctypes.c_void_p
_i = ctypes.c_int
_f = ctypes.c_float
_u64 = ctypes.c_uint64
_ip = ctypes.POINTER(ctypes.c_int)
_fp = ctypes.POINTER(ctypes.c_float)

# name -> argtypes (int results); mirrors include/dcl_pred.h one to one
SIGNATURES = {
    "dpr_version": [],
    "dpr_supported": [_i, _i, _i, _i, _i, _i, _i],
    "dpr_predict": [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp],
    "dpr_panel_supported": [_i, _i, _i],
    "dpr_panel": [_vp, _vp, _i, _vp, _vp, _i, _i, _f, _f, _f, _f, _f, _f, _i, _i, _vp, _vp],
    "dpr_plan_src_index": [_i, _i, _i, _i, _ip, _ip, _fp, _fp],
    "dpr_plan_runs": [_i, _u64, _i, _ip],
}

# device entries issued by this process (tests assert that the HIP path was taken)
calls = {"predict": 0, "panel": 0}

_lib = None


def lib():
    """The loaded library; raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "dpr", "prediction-map kernels")
    return _lib


def check(rc: int, what: str):
    raise_on_error(rc, what, lib().dpr_last_error)


def supported(n: int, c: int, h: int, w: int, H: int, W: int, with_rgb: bool = True) -> bool:
    """Whether dpr_predict takes z [n, c, h, w] resized to H x W (host arithmetic only: include/dcl_pred.h)."""
    return bool(lib().dpr_supported(n, c, h, w, H, W, 1 if with_rgb else 0))


def panel_supported(H: int, W: int, label_bytes: int) -> bool:
    return bool(lib().dpr_panel_supported(H, W, label_bytes))


def plan_src_index(in_size: int, out_size: int, align: bool, dst: int):
    """(i0, i1, l0, l1) of output index dst."""
    i0, i1, l0, l1 = ctypes.c_int(), ctypes.c_int(), ctypes.c_float(), ctypes.c_float()
    check(lib().dpr_plan_src_index(in_size, out_size, 1 if align else 0, dst, ctypes.byref(i0), ctypes.byref(i1), ctypes.byref(l0),
                                   ctypes.byref(l1)), "dpr_plan_src_index")
    return i0.value, i1.value, l0.value, l1.value


def plan_runs(W: int, base: int = 0, pixel_bytes: int = 1):
    """(runs per row, whether a buffer at byte address ``base`` is stored as 4-byte words); (0, False) on bad arguments."""
    vec = ctypes.c_int()
    runs = lib().dpr_plan_runs(W, base, pixel_bytes, ctypes.byref(vec))
    return runs, bool(vec.value) if runs > 0 else False
