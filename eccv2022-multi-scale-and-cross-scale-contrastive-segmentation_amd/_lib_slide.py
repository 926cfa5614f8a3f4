"""ctypes binding of libdcl_slide.so (C ABI: include/dcl_slide.h), sliding-window test-time augmentation with equal-size windows.

A library of its own next to libdcl_hip.so, built by the same Makefile target (``_lib.build()``).  As there, a missing
library or a failed call raises: the caller decides beforehand whether the HIP path applies (models/ops_slide.py)."""
import ctypes
import os

from ._lib import CSRC_DIR, _PKG_DIR, ptr, stream_ptr  # noqa: F401  (re-exported for callers of this module)
from ._lib import load_library, raise_on_error

LIB_PATH = os.path.join(_PKG_DIR, "libdcl_slide.so")
MAX_C = 1024          # DSW_MAX_C
MAX_CIN = 8           # DSW_MAX_CIN
MAX_WIN = 64          # DSW_MAX_WIN
RUN = 4               # DSW_RUN

_vp = ctypes.c_void_p
_i = ctypes.c_int
_ip = ctypes.POINTER(ctypes.c_int)
_fp = ctypes.POINTER(ctypes.c_float)

# name -> argtypes (int results); mirrors include/dcl_slide.h one to one
SIGNATURES = {
    "dsw_version": [],
    "dsw_supported": [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i],
    "dsw_crops": [_vp, _i, _i, _i, _i, _i, _ip, _i, _ip, _i, _i, _i, _fp, _i, _vp, _vp],
    "dsw_gather": [_vp, _vp, _i, _i, _i, _i, _i, _i, _ip, _i, _ip, _i, _vp, _i, _i, _vp],
    "dsw_plan_pc_windows": [_i, _i, _i, _i, _ip, _ip],
    "dsw_plan_cover": [_i, _i, _ip, _i, _ip],
}

# device entries issued by this process (tests assert that the HIP path was taken)
calls = {"crops": 0, "gather": 0}

_lib = None


def lib():
    """The loaded library; raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "dsw", "sliding-window test-time-augmentation kernels")
    return _lib


def check(rc: int, what: str):
    raise_on_error(rc, what, lib().dsw_last_error)


def ints(values):
    """a host ``int`` array for a window table"""
    values = [int(v) for v in values]
    return (ctypes.c_int * max(len(values), 1))(*values)


def floats(values):
    values = [float(v) for v in values]
    return (ctypes.c_float * max(len(values), 1))(*values)


def supported(cin: int, H: int, W: int, c: int, h: int, w: int, wh: int, ww: int, R: int, Q: int, hc: int, wc: int) -> bool:
    """Whether the kernels take one scale's shapes (host arithmetic only: include/dcl_slide.h)."""
    return bool(lib().dsw_supported(cin, H, W, c, h, w, wh, ww, R, Q, hc, wc))


def plan_pc_windows(n: int, crop: int, stride: int):
    """(count, [(lo, hi), ...]) of one axis, already padded to the crop; count < 1: no window, an empty list."""
    L = lib()
    count = L.dsw_plan_pc_windows(n, crop, stride, 0, None, None)
    if count < 1:
        return count, []
    lo, hi = (ctypes.c_int * count)(), (ctypes.c_int * count)()
    assert L.dsw_plan_pc_windows(n, crop, stride, count, lo, hi) == count
    return count, list(zip(lo, hi))


def plan_cover(n: int, wh: int, los):
    """(smallest count, [windows over each of the n positions]); -1 and an empty list for a table the kernels refuse."""
    cnt = (ctypes.c_int * max(n, 1))()
    least = lib().dsw_plan_cover(n, wh, ints(los), len(los), cnt)
    return least, (list(cnt)[:n] if least >= 0 else [])
