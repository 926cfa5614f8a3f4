"""ctypes binding of libdcl_dconv.so (C ABI: include/dcl_dconv.h), the dilated 3x3 convolution kernels of DeepLabv3.

A library of its own next to libdcl_hip.so, built by the same Makefile target (``_lib.build()``).  As there, a missing
library or a failed call raises: the caller decides beforehand whether the HIP path applies (models/ops_dconv.py)."""
import ctypes
import os

from ._lib import CSRC_DIR, _PKG_DIR, ptr, stream_ptr  # noqa: F401  (re-exported for callers of this module)
from ._lib import load_library, raise_on_error

LIB_PATH = os.path.join(_PKG_DIR, "libdcl_dconv.so")
TILE_P = 128          # DDC_TILE_P
TILE_CO = 64          # DDC_TILE_CO
CHUNK_CI = 16         # DDC_CHUNK_CI
WG_TILE = 32          # DDC_WG_TILE
WG_CHUNK_P = 16       # DDC_WG_CHUNK_P
MAX_SLABS = 64        # DDC_MAX_SLABS
SLAB_MIN_UNITS = 32   # DDC_SLAB_MIN_UNITS
WG_TARGET = 2048      # DDC_WG_TARGET
FWD, DGRAD, WGRAD = 0, 1, 2      # DDC_OP_*

_vp = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64

# name -> argtypes (int results except where noted in lib()); mirrors include/dcl_dconv.h one to one
SIGNATURES = {
    "ddc_version": [],
    "ddc_supported": [_i, _i, _i, _i, _i, _i],
    "ddc_live_taps": [_i, _i, _i],
    "ddc_wgrad_slabs": [_i, _i, _i, _i, _i, _i],
    "ddc_workspace_bytes": [_i, _i, _i, _i, _i, _i, _i],
    "ddc_packed_bytes": [_i, _i, _i],
    "ddc_pack": [_vp, _i, _i, _vp, _vp, _vp, _vp],
    "ddc_fwd": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _i64, _vp, _vp],
    "ddc_dgrad": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _i64, _vp, _vp],
    "ddc_wgrad": [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _i64, _vp, _vp],
}

calls = {"fwd": 0, "dgrad": 0, "wgrad": 0}      # device entries issued by this process (tests assert that the HIP path was taken)

_lib = None


def lib():
    """The loaded library; raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "ddc", "dilated convolution kernels",
                            restypes={"ddc_live_taps": ctypes.c_uint, "ddc_workspace_bytes": _i64, "ddc_packed_bytes": _i64})
    return _lib


def check(rc: int, what: str):
    raise_on_error(rc, what, lib().ddc_last_error)


def supported(n: int, ci: int, co: int, h: int, w: int, d: int) -> bool:
    """Whether the kernels take the shape (host arithmetic only: include/dcl_dconv.h)."""
    return bool(lib().ddc_supported(n, ci, co, h, w, d))


def live_taps(h: int, w: int, d: int) -> int:
    """Bit 3 ky + kx is set when tap (ky, kx) reaches the image."""
    return int(lib().ddc_live_taps(h, w, d))


def wgrad_slabs(n: int, ci: int, co: int, h: int, w: int, d: int) -> int:
    return int(lib().ddc_wgrad_slabs(n, ci, co, h, w, d))


def workspace_bytes(op: int, n: int, ci: int, co: int, h: int, w: int, d: int) -> int:
    """Bytes the entry ``op`` (FWD, DGRAD, WGRAD) needs (formulas: include/dcl_dconv.h); -1 for a shape the kernels do not take."""
    return int(lib().ddc_workspace_bytes(op, n, ci, co, h, w, d))


def packed_bytes(co: int, ci: int, transposed: bool) -> int:
    return int(lib().ddc_packed_bytes(co, ci, 1 if transposed else 0))
