"""ctypes binding of libdcl_ocr.so (C ABI: include/dcl_ocr.h), the OCR context core: spatial gather and object attention.

A library of its own next to libdcl_hip.so, built by the same Makefile target (``_lib.build()``).  As there, a missing
library or a failed call raises: the caller decides beforehand whether the HIP path applies (models/ops_ocr.py)."""
import ctypes
import os

from ._lib import CSRC_DIR, _PKG_DIR, ptr, stream_ptr  # noqa: F401  (re-exported for callers of this module)
from ._lib import load_library, raise_on_error

LIB_PATH = os.path.join(_PKG_DIR, "libdcl_ocr.so")
TILE_N = 64           # DCO_TILE_N
CHUNK_C = 64          # DCO_CHUNK_C
MAX_SPLIT = 16        # DCO_MAX_SPLIT
GATHER_FWD, GATHER_BWD, ATTN_FWD, ATTN_BWD = 0, 1, 2, 3      # DCO_OP_*

_vp = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64
_f = ctypes.c_float

# name -> argtypes (int results except where noted in lib()); mirrors include/dcl_ocr.h one to one
SIGNATURES = {
    "dco_version": [],
    "dco_supported": [_i, _i, _i, _i],
    "dco_splits": [_i, _i, _i],
    "dco_workspace_bytes": [_i, _i, _i, _i, _i],
    "dco_gather_fwd": [_vp, _vp, _i, _i, _i, _i, _f, _vp, _i64, _vp, _vp, _vp],
    "dco_gather_bwd": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _i64, _vp, _vp, _vp],
    "dco_attn_fwd": [_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _i64, _vp, _vp],
    "dco_attn_bwd": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _i64, _vp, _vp, _vp, _vp],
}

# device entries issued by this process (tests assert that the HIP path was taken)
calls = {"gather_fwd": 0, "gather_bwd": 0, "attn_fwd": 0, "attn_bwd": 0}

_lib = None


def lib():
    """The loaded library; raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "dco", "OCR context kernels",
                            restypes={"dco_workspace_bytes": _i64})
    return _lib


def check(rc: int, what: str):
    raise_on_error(rc, what, lib().dco_last_error)


def supported(b: int, c: int, k: int, n: int) -> bool:
    """Whether the kernels take the shape; c is the gather's channel count or the attention's key width (host arithmetic only:
    include/dcl_ocr.h)."""
    return bool(lib().dco_supported(b, c, k, n))


def splits(b: int, c: int, n: int) -> int:
    return int(lib().dco_splits(b, c, n))


def workspace_bytes(op: int, b: int, c: int, k: int, n: int) -> int:
    """Bytes the entry ``op`` (GATHER_FWD ... ATTN_BWD) needs (formulas: include/dcl_ocr.h); -1 for a shape the kernels do not take."""
    return int(lib().dco_workspace_bytes(op, b, c, k, n))
