"""ctypes binding of libdcl_attn.so (C ABI: include/dcl_attn.h), the global self-attention kernels.

A library of its own next to libdcl_hip.so, built by the same Makefile target (``_lib.build()``).  As there, a missing
library or a failed call raises: the caller decides beforehand whether the HIP path applies (models/ops_attn.py)."""
import ctypes
import os

from ._lib import CSRC_DIR, _PKG_DIR, ptr, stream_ptr  # noqa: F401  (re-exported for callers of this module)
from ._lib import load_library, raise_on_error

LIB_PATH = os.path.join(_PKG_DIR, "libdcl_attn.so")
MAX_HEAD_DIM = 256    # DAT_MAX_HEAD_DIM
QUERY_BLOCK = 128     # DAT_QUERY_BLOCK

_vp = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64
_f = ctypes.c_float

# name -> argtypes (int results except where noted in lib()); mirrors include/dcl_attn.h one to one
SIGNATURES = {
    "dat_version": [],
    "dat_supported": [_i, _i, _i, _i],
    "dat_workspace_bytes": [_i, _i, _i, _i, _i],
    "dat_attn_fwd": [_vp, _i, _i, _i, _i, _f, _vp, _i64, _vp, _vp, _vp],
    "dat_attn_bwd": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _i64, _vp, _vp],
}

calls = {"fwd": 0, "bwd": 0}      # device entries issued by this process (tests assert that the HIP path was taken)

_lib = None


def lib():
    """The loaded library; raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "dat", "attention kernels",
                            restypes={"dat_workspace_bytes": _i64})
    return _lib


def check(rc: int, what: str):
    raise_on_error(rc, what, lib().dat_last_error)


def supported(b: int, n: int, heads: int, d: int) -> bool:
    """Whether the kernels take the shape (host arithmetic only: include/dcl_attn.h)."""
    return bool(lib().dat_supported(b, n, heads, d))


def workspace_bytes(b: int, n: int, heads: int, d: int, backward: bool) -> int:
    """Bytes dat_attn_fwd / dat_attn_bwd need (formula: include/dcl_attn.h); -1 for a shape the kernels do not take."""
    return int(lib().dat_workspace_bytes(b, n, heads, d, 1 if backward else 0))
