"""ctypes binding of libdcl_lovasz.so (C ABI: include/dcl_lovasz.h), the Lovasz-Softmax kernels.

A library of its own next to libdcl_hip.so, built by the same Makefile target (``_lib.build()``).  As there, a missing
library or a failed call raises: the caller decides beforehand whether the HIP path applies (losses/LovaszSoftmax.py)."""
import ctypes
import os

from ._lib import CSRC_DIR, _PKG_DIR, ptr, stream_ptr  # noqa: F401  (re-exported for callers of this module)
from ._lib import load_library, raise_on_error

LIB_PATH = os.path.join(_PKG_DIR, "libdcl_lovasz.so")
MAX_CLASSES = 256     # DLV_MAX_CLASSES
TILE = 4096           # DLV_TILE

_vp = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64

# name -> argtypes (int results except where noted in lib()); mirrors include/dcl_lovasz.h one to one
SIGNATURES = {
    "dlv_version": [],
    "dlv_workspace_bytes": [_i, _i, _i, _i],
    "dlv_lovasz_fwd": [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _i64, _vp, _vp, _vp],
    "dlv_lovasz_bwd": [_vp, _vp, _vp, _i, _i, _i, _vp, _vp],
}

_lib = None


def lib():
    """The loaded library; raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "dlv", "Lovasz-Softmax kernels",
                            restypes={"dlv_workspace_bytes": _i64})
    return _lib


def check(rc: int, what: str):
    raise_on_error(rc, what, lib().dlv_last_error)


def workspace_bytes(n: int, c: int, hw: int, per_image: bool) -> int:
    """Bytes dlv_lovasz_fwd needs (formula: include/dcl_lovasz.h); -1 for a shape the kernels do not take."""
    return int(lib().dlv_workspace_bytes(n, c, hw, 1 if per_image else 0))
