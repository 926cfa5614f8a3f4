"""ctypes binding of libdcl_tsne.so (C ABI: include/dcl_tsne.h), exact t-SNE of sampled pixel features (demo_tsne).

A library of its own next to libdcl_hip.so, built by the same Makefile target (``_lib.build()``).  As there, a missing
library or a failed call raises: the caller decides beforehand whether the HIP path applies (utils/tsne.py)."""
import ctypes
import os

from ._lib import CSRC_DIR, _PKG_DIR, ptr, stream_ptr  # noqa: F401  (re-exported for callers of this module)
from ._lib import load_library, raise_on_error

LIB_PATH = os.path.join(_PKG_DIR, "libdcl_tsne.so")
MAX_D = 64            # DTS_MAX_D
LDS_ROW = 8192        # DTS_LDS_ROW
SYM_TILE = 32         # DTS_SYM_TILE
SYM_GROUPS = 1024     # DTS_SYM_GROUPS
Z_ROWS = 256          # DTS_Z_ROWS
Z_COLS = 1024         # DTS_Z_COLS
GRAD_ROWS = 8         # DTS_GRAD_ROWS
UPD_ROWS = 256        # DTS_UPD_ROWS

_vp = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64
_u64 = ctypes.c_uint64
_f = ctypes.c_float
_d = ctypes.c_double

# name -> argtypes (int results unless in RESTYPES); mirrors include/dcl_tsne.h one to one
SIGNATURES = {
    "dts_version": [],
    "dts_supported": [_i64, _i, _d],
    "dts_plan_row_in_lds": [_i],
    "dts_plan_sym_groups": [_i],
    "dts_plan_z_parts": [_i],
    "dts_plan_grad_groups": [_i],
    "dts_plan_upd_groups": [_i],
    "dts_plan_grad_vec": [_u64, _i],
    "dts_plan_ws_floats": [_i],
    "dts_plan_kl_slots": [_i],
    "dts_cond_p": [_vp, _i, _i, _f, _i, _vp, _vp, _vp],
    "dts_symmetrize": [_vp, _i, _vp, _vp],
    "dts_zsum": [_vp, _i, _vp, _vp],
    "dts_gradient": [_vp, _vp, _i, _f, _vp, _vp, _vp, _vp, _vp],
    "dts_update": [_vp, _vp, _vp, _vp, _i, _f, _vp, _vp, _vp, _vp],
    "dts_run": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp],
}
RESTYPES = {"dts_plan_ws_floats": _i64}

# device entries issued by this process (tests assert that the HIP path was taken)
calls = {"cond_p": 0, "symmetrize": 0, "zsum": 0, "gradient": 0, "update": 0, "run": 0}

_lib = None


def lib():
    """The loaded library; raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "dts", "t-SNE kernels", restypes=RESTYPES)
    return _lib


def check(rc: int, what: str):
    raise_on_error(rc, what, lib().dts_last_error)


def supported(n: int, d: int, perplexity: float) -> bool:
    """Whether the kernels take X [n, d] at this perplexity (host arithmetic only: include/dcl_tsne.h)."""
    return bool(lib().dts_supported(int(n), int(d), float(perplexity)))


def plan(n: int) -> dict:
    """The counts of csrc/dcl_tsne_plan.h for n points."""
    L = lib()
    return {"row_in_lds": bool(L.dts_plan_row_in_lds(n)), "sym_groups": L.dts_plan_sym_groups(n), "z_parts": L.dts_plan_z_parts(n),
            "grad_groups": L.dts_plan_grad_groups(n), "upd_groups": L.dts_plan_upd_groups(n), "ws_floats": int(L.dts_plan_ws_floats(n))}


def plan_grad_vec(base: int, n: int) -> bool:
    return bool(lib().dts_plan_grad_vec(base, n))


def plan_kl_slots(n_iter: int) -> int:
    return int(lib().dts_plan_kl_slots(n_iter))


# ---- the device entries on torch tensors (f32, CUDA, contiguous: the callers check; outputs are the caller's) ---------------------
def cond_p(X, perplexity, P, beta, scratch=False):
    check(lib().dts_cond_p(ptr(X), X.shape[0], X.shape[1], float(perplexity), 1 if scratch else 0, ptr(P), ptr(beta),
                           stream_ptr(X.device)), "dts_cond_p")
    calls["cond_p"] += 1


def symmetrize(P, part):
    check(lib().dts_symmetrize(ptr(P), P.shape[0], ptr(part), stream_ptr(P.device)), "dts_symmetrize")
    calls["symmetrize"] += 1


def zsum(Y, zpart):
    check(lib().dts_zsum(ptr(Y), Y.shape[0], ptr(zpart), stream_ptr(Y.device)), "dts_zsum")
    calls["zsum"] += 1


def gradient(P, Y, exaggeration, zpart, dY, klpart=None, z_out=None):
    check(lib().dts_gradient(ptr(P), ptr(Y), Y.shape[0], float(exaggeration), ptr(zpart), ptr(dY), ptr(klpart), ptr(z_out),
                             stream_ptr(Y.device)), "dts_gradient")
    calls["gradient"] += 1


def update(dY, iY, gains, Y, momentum, colpart, klpart=None, kl_out=None):
    check(lib().dts_update(ptr(dY), ptr(iY), ptr(gains), ptr(Y), Y.shape[0], float(momentum), ptr(colpart), ptr(klpart), ptr(kl_out),
                           stream_ptr(Y.device)), "dts_update")
    calls["update"] += 1


def run(P, Y, iY, gains, dY, ws, first, last, kl_hist=None):
    check(lib().dts_run(ptr(P), ptr(Y), ptr(iY), ptr(gains), ptr(dY), ptr(ws), Y.shape[0], int(first), int(last), ptr(kl_hist),
                        stream_ptr(Y.device)), "dts_run")
    calls["run"] += 1
