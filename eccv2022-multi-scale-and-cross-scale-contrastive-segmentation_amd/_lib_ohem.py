"""ctypes binding of libdcl_ohem.so (C ABI: include/dcl_ohem.h): the hard-pixel mining of OhemCrossEntropy -- target probability,
exact k-th-smallest selection by radix select, masked reduction.

A library of its own next to libdcl_hip.so, built by the same Makefile target (``_lib.build()``).  As there, a missing
library or a failed call raises: the caller decides beforehand whether the HIP path applies (losses/OhemCrossEntropy.py)."""
import ctypes
import os

from ._lib import CSRC_DIR, _PKG_DIR, ptr, stream_ptr  # noqa: F401  (re-exported for callers of this module)
from ._lib import load_library, raise_on_error

LIB_PATH = os.path.join(_PKG_DIR, "libdcl_ohem.so")
MAX_C = 255            # DOH_MAX_C
INVALID_BITS = -1      # DOH_INVALID_BITS as int32
RES_WORDS = 8          # DOH_RES_WORDS
RES_LOSS, RES_DENOM, RES_V, RES_THR, RES_N, RES_M, RES_K, RES_EMPTY = range(8)      # DOH_RES_*

_vp = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64
_f = ctypes.c_float
_ip = ctypes.POINTER(ctypes.c_int)

# name -> argtypes (int results except where noted in lib()); mirrors include/dcl_ohem.h one to one
SIGNATURES = {
    "doh_version": [],
    "doh_supported": [_i, _i, _i, _i, _i, _i],
    "doh_workspace_bytes": [_i, _i],
    "doh_target_prob": [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp],
    "doh_select": [_vp, _i64, _i, _f, _vp, _vp],
    "doh_reduce": [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp],
    "doh_plan_layout": [_ip, _ip],
}

# device entries issued by this process (tests assert which path was taken)
calls = {"target_prob": 0, "select": 0, "reduce": 0}

_lib = None


def lib():
    """The loaded library; raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "doh", "hard-pixel mining kernels of OhemCrossEntropy",
                            restypes={"doh_workspace_bytes": _i64})
    return _lib


def check(rc: int, what: str):
    raise_on_error(rc, what, lib().doh_last_error)


def supported(N: int, C: int, h: int, w: int, H: int, W: int) -> bool:
    """Whether the entries (and dcl_upsample_ce_fwd / _bwd around them) take the shape: host arithmetic only."""
    return bool(lib().doh_supported(int(N), int(C), int(h), int(w), int(H), int(W)))


def workspace_bytes(N: int, H: int) -> int:
    return int(lib().doh_workspace_bytes(int(N), int(H)))


def layout():
    """({'hist0', 'hist1', 'hist2', 'state', 'part'} -> word offset, bins of the three passes)"""
    off, bins = (ctypes.c_int * 5)(), (ctypes.c_int * 3)()
    check(lib().doh_plan_layout(off, bins), "doh_plan_layout")
    return dict(zip(("hist0", "hist1", "hist2", "state", "part"), off)), list(bins)


def target_prob(z, size, align_corners, target, weight, ignore_index, lse, p, l, ws, stream):
    calls["target_prob"] += 1
    N, C, h, w = z.shape
    check(lib().doh_target_prob(ptr(z), N, C, h, w, int(size[0]), int(size[1]), 1 if align_corners else 0, ptr(target), ptr(weight),
                                int(ignore_index), ptr(lse), ptr(p), ptr(l), ptr(ws), stream), "doh_target_prob")


def select(p, min_kept: int, thresh: float, ws, stream):
    calls["select"] += 1
    check(lib().doh_select(ptr(p), p.numel(), int(min(max(min_kept, 1), 2 ** 31 - 1)), float(thresh), ptr(ws), stream), "doh_select")


def reduce(p, l, target, ignore_index, ws, hard, kept8, res, stream):
    calls["reduce"] += 1
    N, H, W = p.shape
    check(lib().doh_reduce(ptr(p), ptr(l), ptr(target), N, H, W, int(ignore_index), ptr(ws), ptr(hard), ptr(kept8), ptr(res), stream),
          "doh_reduce")
