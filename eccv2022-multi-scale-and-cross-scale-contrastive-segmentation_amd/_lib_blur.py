"""ctypes binding of libdcl_blur.so (C ABI: include/dcl_blur.h): the steps of the input augmentation that follow the crop -- PIL's
Gaussian blur, the reflected row padding, the colour operations on planes.

A library of its own next to libdcl_hip.so, built by the same Makefile target (``_lib.build()``).  As there, a missing
library or a failed call raises: the caller decides beforehand whether the HIP path applies (datasets/augment.py)."""
import ctypes
import os

from ._lib import CSRC_DIR, _PKG_DIR, ptr, stream_ptr  # noqa: F401  (re-exported for callers of this module)
from ._lib import load_library, raise_on_error

LIB_PATH = os.path.join(_PKG_DIR, "libdcl_blur.so")
MAX_RADIUS = 8        # DBL_MAX_RADIUS
MAX_CHANNELS = 4      # DBL_MAX_CHANNELS
ROW_TILE_H = 4        # DBL_ROW_TILE_H
ROW_TILE_W = 256      # DBL_ROW_TILE_W
COL_TILE_H = 64       # DBL_COL_TILE_H
COL_TILE_W = 64       # DBL_COL_TILE_W
WS_INTS = 576         # DBL_WS_INTS
WS_TICKET = 32        # DBL_WS_TICKET
WS_MEAN = 33          # DBL_WS_MEAN
WS_PART = 64          # DBL_WS_PART
MAX_BLOCKS = 256      # DBL_MAX_BLOCKS

_vp = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64
_ip = ctypes.POINTER(ctypes.c_int)
_fp = ctypes.POINTER(ctypes.c_float)


class CColourPlan(ctypes.Structure):
    """``dbl_colour_plan`` of include/dcl_blur.h, field for field."""
    _fields_ = [("h", ctypes.c_int32), ("w", ctypes.c_int32), ("ncolor", ctypes.c_int32), ("perm", ctypes.c_int32 * 4),
                ("b", ctypes.c_float), ("c", ctypes.c_float), ("s", ctypes.c_float), ("delta", ctypes.c_float)]


_pp = ctypes.POINTER(CColourPlan)

# name -> argtypes (int results); mirrors include/dcl_blur.h one to one
SIGNATURES = {
    "dbl_version": [],
    "dbl_supported": [_i, _i, _i, _i],
    "dbl_box": [_i, _ip, _fp, _fp],
    "dbl_blur": [_vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "dbl_pad_rows": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "dbl_gray_mean": [_vp, _pp, _vp, _vp],
    "dbl_colour": [_vp, _pp, _vp, _vp],
    "dbl_from_unit": [_vp, _vp, _i64, _vp],
    "dbl_normalise": [_vp, _vp, _i, _i64, _vp],
}

# device entries issued by this process (tests assert which path was taken)
calls = {"blur": 0, "pad_rows": 0, "gray_mean": 0, "colour": 0, "from_unit": 0, "normalise": 0}

_lib = None


def lib():
    """The loaded library; raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "dbl", "blur / pad / colour kernels of the input augmentation")
    return _lib


def check(rc: int, what: str):
    raise_on_error(rc, what, lib().dbl_last_error)


def colour_plan(plan, h: int, w: int) -> CColourPlan:
    """The colour operations of a ``datasets.augment.Plan`` on planes of h x w."""
    cp = CColourPlan()
    cp.h, cp.w = int(h), int(w)
    cp.ncolor = len(plan.perm)
    for k, op in enumerate(plan.perm[:4]):
        cp.perm[k] = int(op)
    cp.b, cp.c, cp.s, cp.delta = float(plan.b), float(plan.c), float(plan.s), float(plan.delta)
    return cp


def supported(C: int, h: int, w: int, radius) -> bool:
    """Whether ``blur`` takes the shape and the radius (host arithmetic only: include/dcl_blur.h, "Limits")."""
    return radius == int(radius) and bool(lib().dbl_supported(int(C), int(h), int(w), int(radius)))


def box(radius: int):
    """(l, ww, fw) of the extended box of a radius: the library's own host arithmetic."""
    l, ww, fw = ctypes.c_int(), ctypes.c_float(), ctypes.c_float()
    check(lib().dbl_box(int(radius), ctypes.byref(l), ctypes.byref(ww), ctypes.byref(fw)), "dbl_box")
    return l.value, ww.value, fw.value


def blur(src, dst, scratch, radius: int, stream):
    calls["blur"] += 1
    C, h, w = src.shape
    check(lib().dbl_blur(ptr(src), ptr(dst), ptr(scratch), C, h, w, int(radius), stream), "dbl_blur")


def pad_rows(src, dst, lbl_src, lbl_dst, top: int, bottom: int, stream):
    calls["pad_rows"] += 1
    C, h, w = src.shape
    check(lib().dbl_pad_rows(ptr(src), ptr(dst), ptr(lbl_src), ptr(lbl_dst), C, h, w, int(top), int(bottom), stream), "dbl_pad_rows")


def gray_mean(planes, cp: CColourPlan, ws, stream):
    calls["gray_mean"] += 1
    check(lib().dbl_gray_mean(ptr(planes), ctypes.byref(cp), ptr(ws), stream), "dbl_gray_mean")


def colour(planes, cp: CColourPlan, ws, stream):
    calls["colour"] += 1
    check(lib().dbl_colour(ptr(planes), ctypes.byref(cp), ptr(ws), stream), "dbl_colour")


def from_unit(src, dst, stream):
    calls["from_unit"] += 1
    check(lib().dbl_from_unit(ptr(src), ptr(dst), src.numel(), stream), "dbl_from_unit")


def normalise(planes, out, normalise: bool, stream):
    calls["normalise"] += 1
    check(lib().dbl_normalise(ptr(planes), ptr(out), 1 if normalise else 0, planes.shape[1] * planes.shape[2], stream), "dbl_normalise")
