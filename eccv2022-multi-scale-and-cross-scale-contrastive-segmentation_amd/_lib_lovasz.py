"""ctypes binding of libdcl_lovasz.so (C ABI: include/dcl_lovasz.h), the Lovasz-Softmax kernels.

A library of its own next to libdcl_hip.so, built by the same Makefile target (``_lib.build()``).  As there, a missing
library or a failed call raises: the caller decides beforehand whether the HIP path applies (losses/LovaszSoftmax.py)."""
import ctypes
import os

from ._lib import CSRC_DIR, _PKG_DIR, ptr, stream_ptr  # noqa: F401  (re-exported for callers of this module)

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
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found. The Lovasz-Softmax kernels have no fallback once selected: build the HIP "
                f"libraries first (python -c 'import __graft_entry__ as g; g.build()' or make -C {CSRC_DIR}).")
        l = ctypes.CDLL(LIB_PATH)
        for name, argtypes in SIGNATURES.items():
            fn = getattr(l, name)
            fn.argtypes = argtypes
            fn.restype = ctypes.c_int
        l.dlv_workspace_bytes.restype = ctypes.c_int64
        l.dlv_last_error.restype = ctypes.c_char_p
        l.dlv_last_error.argtypes = []
        _lib = l
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().dlv_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def workspace_bytes(n: int, c: int, hw: int, per_image: bool) -> int:
    """Bytes dlv_lovasz_fwd needs (formula: include/dcl_lovasz.h); -1 for a shape the kernels do not take."""
    return int(lib().dlv_workspace_bytes(n, c, hw, 1 if per_image else 0))
