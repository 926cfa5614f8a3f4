"""ctypes binding of libdcl_aug.so (C ABI: include/dcl_aug.h), the on-device input augmentation.

A library of its own next to libdcl_hip.so, built by the same Makefile target (``_lib.build()``).  As there, a missing
library or a failed call raises: the caller decides beforehand whether the HIP path applies (datasets/augment.py)."""
import ctypes
import os

from ._lib import CSRC_DIR, _PKG_DIR, ptr, stream_ptr  # noqa: F401  (re-exported for callers of this module)
from ._lib import load_library, raise_on_error

LIB_PATH = os.path.join(_PKG_DIR, "libdcl_aug.so")
MAX_CAND = 10         # DAU_MAX_CAND
MAX_TAPS = 18         # DAU_MAX_TAPS
WS_INTS = 576         # DAU_WS_INTS
WS_TICKET = 32        # DAU_WS_TICKET
WS_MEAN = 33          # DAU_WS_MEAN
WS_PART = 64          # DAU_WS_PART
MAX_BLOCKS = 256      # DAU_MAX_BLOCKS

_vp = ctypes.c_void_p
_i = ctypes.c_int
_ip = ctypes.POINTER(ctypes.c_int)
_fp = ctypes.POINTER(ctypes.c_float)


class CPlan(ctypes.Structure):
    """``dau_plan`` of include/dcl_aug.h, field for field."""
    _fields_ = [("H", ctypes.c_int32), ("W", ctypes.c_int32), ("rh", ctypes.c_int32), ("rw", ctypes.c_int32),
                ("Hc", ctypes.c_int32), ("Wc", ctypes.c_int32), ("pt", ctypes.c_int32), ("pl", ctypes.c_int32),
                ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("flip", ctypes.c_int32), ("P", ctypes.c_int32),
                ("ci", ctypes.c_int32 * MAX_CAND), ("cj", ctypes.c_int32 * MAX_CAND),
                ("ncolor", ctypes.c_int32), ("perm", ctypes.c_int32 * 4),
                ("b", ctypes.c_float), ("c", ctypes.c_float), ("s", ctypes.c_float), ("delta", ctypes.c_float),
                ("normalise", ctypes.c_int32), ("ignore", ctypes.c_int32), ("max_ratio", ctypes.c_double)]


_pp = ctypes.POINTER(CPlan)

# name -> argtypes (int results); mirrors include/dcl_aug.h one to one
SIGNATURES = {
    "dau_version": [],
    "dau_supported": [_pp],
    "dau_crop_select": [_vp, _vp, _pp, _vp, _vp],
    "dau_gray_mean": [_vp, _pp, _vp, _vp],
    "dau_apply": [_vp, _vp, _vp, _pp, _vp, _vp, _vp, _vp],
    "dau_plan_taps": [_i, _i, _i, _i, _ip, _fp],
    "dau_plan_nearest": [_i, _i, _i],
}

# device entries issued by this process (tests assert that the HIP path was taken)
calls = {"crop_select": 0, "gray_mean": 0, "apply": 0}

_lib = None


def lib():
    """The loaded library; raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "dau", "input-augmentation kernels")
    return _lib


def check(rc: int, what: str):
    raise_on_error(rc, what, lib().dau_last_error)


def c_plan(plan) -> CPlan:
    """The C form of a ``datasets.augment.Plan`` (candidates beyond MAX_CAND cannot be expressed: P is kept, so that
    ``supported`` refuses the plan)."""
    cp = CPlan()
    for k in ("H", "W", "rh", "rw", "Hc", "Wc", "pt", "pl", "h", "w"):
        setattr(cp, k, int(getattr(plan, k)))
    cp.flip = 1 if plan.flip else 0
    cp.P = len(plan.corners)
    for p, (i, j) in enumerate(plan.corners[:MAX_CAND]):
        cp.ci[p], cp.cj[p] = int(i), int(j)
    cp.ncolor = len(plan.perm)
    for k, op in enumerate(plan.perm[:4]):
        cp.perm[k] = int(op)
    cp.b, cp.c, cp.s, cp.delta = float(plan.b), float(plan.c), float(plan.s), float(plan.delta)
    cp.normalise = 1 if plan.normalise else 0
    cp.ignore = int(plan.ignore)
    cp.max_ratio = float(plan.max_ratio) if plan.max_ratio else 0.0
    return cp


def supported(cp: CPlan) -> bool:
    """Whether the kernels take the plan (host arithmetic only: include/dcl_aug.h, "Limits")."""
    return bool(lib().dau_supported(ctypes.byref(cp)))


def crop_select(lbl, lut, cp: CPlan, ws, stream):
    calls["crop_select"] += 1
    check(lib().dau_crop_select(ptr(lbl), ptr(lut), ctypes.byref(cp), ptr(ws), stream), "dau_crop_select")


def gray_mean(img, cp: CPlan, ws, stream):
    calls["gray_mean"] += 1
    check(lib().dau_gray_mean(ptr(img), ctypes.byref(cp), ptr(ws), stream), "dau_gray_mean")


def apply(img, lbl, lut, cp: CPlan, ws, out_img, out_lbl, stream):
    calls["apply"] += 1
    check(lib().dau_apply(ptr(img), ptr(lbl), ptr(lut), ctypes.byref(cp), ptr(ws), ptr(out_img), ptr(out_lbl), stream), "dau_apply")


def plan_taps(S: int, D: int, o: int):
    """(first tap, [normalised fp32 weights]) of output index o along an axis resized from S to D."""
    k0 = ctypes.c_int()
    w = (ctypes.c_float * MAX_TAPS)()
    n = lib().dau_plan_taps(S, D, o, MAX_TAPS, ctypes.byref(k0), w)
    if n < 0 or n > MAX_TAPS:
        raise RuntimeError(f"dau_plan_taps({S}, {D}, {o}) = {n}")
    return k0.value, list(w[:n])


def plan_nearest(S: int, D: int, o: int) -> int:
    r = lib().dau_plan_nearest(S, D, o)
    if r < 0:
        raise RuntimeError(f"dau_plan_nearest({S}, {D}, {o}): bad arguments")
    return r
