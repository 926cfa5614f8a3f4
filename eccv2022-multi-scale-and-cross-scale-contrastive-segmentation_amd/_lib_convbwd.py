"""ctypes binding of libdcl_convbwd.so (C ABI: include/dcl_convbwd.h): the backward of a 3x3 / stride 1 / pad 1 convolution, data and
weight gradient, in one launch.

A library of its own next to libdcl_hip.so, built by the same Makefile target (``_lib.build()``).  As there, a missing
library or a failed call raises: the caller decides beforehand whether the fused launch applies (models/ops_conv.py)."""
import ctypes
import os

from ._lib import CSRC_DIR, _PKG_DIR, ptr, stream_ptr  # noqa: F401  (re-exported for callers of this module)
from ._lib import load_library, raise_on_error

LIB_PATH = os.path.join(_PKG_DIR, "libdcl_convbwd.so")
CUS = 256             # DCB_CUS
PLAN_FIELDS = ("nd", "nd8", "wgrad_grid", "slabs", "wave_mode", "tile_r", "tile_p", "wg_target")

_vp = ctypes.c_void_p
_i = ctypes.c_int

# name -> argtypes (int results); mirrors include/dcl_convbwd.h one to one
SIGNATURES = {
    "dcb_version": [],
    "dcb_supported": [_i, _i, _i, _i, _i, _i],
    "dcb_plan": [_i, _i, _i, _i, _i, _i, _i, _i, ctypes.POINTER(_i)],
    "dcb_wgrad_splits": [_i, _i, _i, _i, _i, _i, _i, _i],
    "dcb_conv3x3_bwd_f16x3": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp],
}

calls = {"bwd": 0}      # device entries issued by this process (tests assert that the fused path was taken)

_lib = None


def lib():
    """The loaded library; raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "dcb", "fused convolution backward")
    return _lib


def built() -> bool:
    return os.path.exists(LIB_PATH)


def check(rc: int, what: str):
    raise_on_error(rc, what, lib().dcb_last_error)


def supported(n: int, ci: int, co: int, h: int, w: int, pre: bool = False) -> bool:
    """Whether the fused launch serves the shape under its automatic plan (host arithmetic only: include/dcl_convbwd.h)."""
    return bool(lib().dcb_supported(n, ci, co, h, w, 1 if pre else 0))


def plan(n: int, ci: int, co: int, h: int, w: int, tile_r: int = 0, tile_p: int = 0, wg_target: int = 0):
    """The plan of a launch as a dict of PLAN_FIELDS, or None for a shape / tile the kernels do not take."""
    out = (_i * 8)()
    if lib().dcb_plan(n, ci, co, h, w, tile_r, tile_p, wg_target, out) != 0:
        return None
    return dict(zip(PLAN_FIELDS, out))


def wgrad_splits(n: int, ci: int, co: int, h: int, w: int, tile_r: int = 0, tile_p: int = 0, wg_target: int = 0) -> int:
    return int(lib().dcb_wgrad_splits(n, ci, co, h, w, tile_r, tile_p, wg_target))
