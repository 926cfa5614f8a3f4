"""ctypes binding of libdcl_tta.so (C ABI: include/dcl_tta.h), the merge of test-time-augmentation views.

A library of its own next to libdcl_hip.so, built by the same Makefile target (``_lib.build()``).  As there, a missing
library or a failed call raises: the caller decides beforehand whether the HIP path applies (models/ops_tta.py)."""
import ctypes
import os

from ._lib import CSRC_DIR, _PKG_DIR, ptr, stream_ptr  # noqa: F401  (re-exported for callers of this module)
from ._lib import load_library, raise_on_error

LIB_PATH = os.path.join(_PKG_DIR, "libdcl_tta.so")
MAX_C = 1024          # DTT_MAX_C
RUN = 4               # DTT_RUN

_vp = ctypes.c_void_p
_i = ctypes.c_int
_f = ctypes.c_float
_d = ctypes.c_double
_ip = ctypes.POINTER(ctypes.c_int)
_fp = ctypes.POINTER(ctypes.c_float)

# name -> argtypes (int results); mirrors include/dcl_tta.h one to one
SIGNATURES = {
    "dtt_version": [],
    "dtt_supported": [_i, _i, _i, _i, _i, _i, _i],
    "dtt_merge": [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _i, _f, _vp],
    "dtt_window_accum": [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "dtt_canvas_merge": [_vp, _vp, _vp, _i, _i, _i, _vp, _i, _i, _i, _vp],
    "dtt_plan_cts_size": [_i, _i, _i, _d, _ip, _ip],
    "dtt_plan_windows": [_i, _i, _i, _i, _ip, _ip, _ip],
    "dtt_plan_src_index": [_i, _i, _i, _i, _ip, _ip, _fp, _fp],
}

# device entries issued by this process (tests assert that the HIP path was taken)
calls = {"merge": 0, "window_accum": 0, "canvas_merge": 0}

_lib = None


def lib():
    """The loaded library; raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "dtt", "test-time-augmentation kernels")
    return _lib


def check(rc: int, what: str):
    raise_on_error(rc, what, lib().dtt_last_error)


def supported(c: int, h: int, w: int, hm: int, wm: int, H: int, W: int) -> bool:
    """Whether the kernels take z [c, h, w] resized to hm x wm and merged into [c, H, W] (host arithmetic only: include/dcl_tta.h)."""
    return bool(lib().dtt_supported(c, h, w, hm, wm, H, W))


def plan_cts_size(H: int, W: int, base_size: int, scale: float):
    """(new_h, new_w) of the Cityscapes image-size rule."""
    nh, nw = ctypes.c_int(), ctypes.c_int()
    check(lib().dtt_plan_cts_size(H, W, base_size, float(scale), ctypes.byref(nh), ctypes.byref(nw)), "dtt_plan_cts_size")
    return nh.value, nw.value


def plan_windows(n: int, crop: int, stride: int):
    """(count, [(lo, hi), ...], [windows over each of the n positions]) of one axis; count < 1: no window, empty lists."""
    L = lib()
    count = L.dtt_plan_windows(n, crop, stride, 0, None, None, None)
    if count < 1:
        return count, [], []
    lo, hi, cnt = (ctypes.c_int * count)(), (ctypes.c_int * count)(), (ctypes.c_int * n)()
    assert L.dtt_plan_windows(n, crop, stride, count, lo, hi, cnt) == count
    return count, list(zip(lo, hi)), list(cnt)


def plan_src_index(in_size: int, out_size: int, align: bool, dst: int):
    """(i0, i1, l0, l1) of output index dst."""
    i0, i1, l0, l1 = ctypes.c_int(), ctypes.c_int(), ctypes.c_float(), ctypes.c_float()
    check(lib().dtt_plan_src_index(in_size, out_size, 1 if align else 0, dst, ctypes.byref(i0), ctypes.byref(i1), ctypes.byref(l0),
                                   ctypes.byref(l1)), "dtt_plan_src_index")
    return i0.value, i1.value, l0.value, l1.value
