"""Shared cases, float64 reference and derived bounds of the bilinear resize tests (tests/test_resize_reference.py on the CPU,
tests/test_resize_fp64.py and the resize tests of tests/test_model_ops_parity.py on the GPU).  Importable without a GPU.

Reference.  ``weights(in, out, align)`` is the dense [out, in] matrix of ATen's f32 bilinear weights along one axis, promoted to
float64 (CPU F.interpolate in fp32 applied to the unit vectors of the axis: every output is then l0 * 1 + l1 * 0, exact).  The
reference is  y = Wy . x . Wx^T (+ add)  and  dx = Wy^T . dy . Wx  by einsum in float64: it shares the f32 weights with the kernels
(csrc/dcl_bilinear.h restates ATen's) and nothing else, so what is left to compare is the kernels' accumulation.

Bound, elementwise:  |got - ref| <= gamma_k * A,  gamma_k = k u / (1 - k u),  u = 2^-24,  A the same contraction over absolute
values (Wy |x| Wx^T + |add|;  Wy^T |dy| Wx).  k = the number of f32 roundings on the longest chain a term passes through, counted
in csrc/dcl_resize.hip:
  forward  (k_upsample_fwd, ``v[k] = ly0 * (lx0 * r0[x0] + lx1 * r0[x1]) + ly1 * (...)``): product by lx, sum of the pair, product
           by ly, sum of the two rows = 4, + 1 for the addend's sum.  The ReLU is 1-Lipschitz: the same bound holds behind it.
  backward (k_upsample_bwd: ``rowacc += wx * g`` over the nx outputs of a row, ``acc += wy * rowacc`` over the ny rows;
           k_upsample_bwd_rows: ``acc += wy * v`` over the ny rows into LDS, ``acc += wx * tmp[ox]`` over the nx columns): a
           product and at most n - 1 inexact sums per pass (the first sum adds to 0, a term of weight 0 adds 0: both exact) =
           ny + nx, with ny, nx the largest number of non-zero weights in a column of Wy, Wx.  K_BWD_EXTRA = 4 on top.
The bound holds for any association of the sums and with or without FMA contraction (a contraction removes a rounding).  Where A
is 0 it is 0: the output has to be exactly 0.
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
K_FWD = 4                 # + 1 with an addend
K_BWD_EXTRA = 4
MAX_AMBIGUOUS = 1e-3      # share of a ReLU case's elements whose sign the forward bound leaves open

ROWS_MAXW = 4096          # csrc/dcl_resize.hip
MAXC = 16                 # k_upsample_bwd: footprints up to this many columns are unrolled

Case = collections.namedtuple("Case", "name n c h w H W add relu bwd nx_gt_maxc")

# name, (n, c, h, w) -> (H, W), addend, relu, the backward form upsample_bwd() picks, whether some footprint exceeds MAXC columns
# (under at least one of the two align_corners values: 2 -> 17 and 3 -> 17 give 17 with it, 15 without).
# The comment names the branch of csrc/dcl_resize.hip the case is there for.
CASES = [
    # k_upsample_fwd: W = 4 -> tpr = 1, 256 rows per workgroup, 300 rows: the second workgroup's `row >= nrows` tail
    Case("fwd_w4_row_tail", 1, 3, 50, 2, 100, 4, True, False, "rows", False),
    # k_upsample_fwd: W = 1040 > 1024 -> second trip of `ox4 += tpr * 4` on the 16-byte path;
    # k_upsample_bwd_rows: 256 threads, second trip of the vertical pass (W > 1024) and of the horizontal one (w = 260 > 256)
    Case("w1040_two_trips_rows_both_loops", 1, 2, 2, 260, 4, 1040, True, False, "rows", False),
    # k_upsample_fwd: vec == false, one trip, ragged last quad (33 = 8 * 4 + 1); k_upsample_bwd with nx <= MAXC
    Case("w33_scalar_elem_small_nx", 1, 4, 8, 8, 30, 33, True, False, "elem", False),
    # k_upsample_fwd: vec == false, second trip, ragged last quad (1030 = 257 * 4 + 2); k_upsample_bwd `nx > MAXC` loop (x10)
    Case("w1030_scalar_two_trips", 1, 2, 3, 103, 5, 1030, True, False, "elem", True),
    # relu x addend on the 16-byte path; _UpsampleBilinear.backward's threshold_backward mask
    Case("relu0_add0", 1, 3, 7, 10, 28, 40, False, False, "rows", False),
    Case("relu0_add1", 1, 3, 7, 10, 28, 40, True, False, "rows", False),
    Case("relu1_add0", 1, 3, 7, 10, 28, 40, False, True, "rows", False),
    Case("relu1_add1", 1, 3, 7, 10, 28, 40, True, True, "rows", False),
    # the same on the scalar path
    Case("relu1_add1_scalar", 1, 2, 8, 8, 30, 33, True, True, "elem", False),
    Case("relu1_add0_scalar", 1, 2, 8, 8, 30, 33, False, True, "elem", False),
    # k_upsample_bwd_rows with 64 threads (W <= 256), more than one image
    Case("rows_64_threads", 2, 2, 5, 12, 10, 48, True, False, "rows", False),
    # k_upsample_bwd_rows at ROWS_MAXW: four trips of either pass (W = 4096, w = 1024), 16 KiB of LDS
    Case("rows_w4096", 1, 1, 2, 1024, 3, 4096, True, False, "rows", False),
    # upsample_bwd: W = 4100 > ROWS_MAXW falls through to k_upsample_bwd although W % 4 == 0; forward: five trips
    Case("w4100_falls_to_elem", 1, 1, 2, 1025, 3, 4100, True, False, "elem", False),
    # k_upsample_bwd `nx > MAXC`: one input pixel under 17 / 35 outputs; align_corners: in-size 1 -> scale 0 -> the full range
    Case("elem_1_to_17", 1, 2, 1, 1, 17, 17, True, False, "elem", True),
    Case("elem_3_to_35", 1, 2, 3, 3, 35, 35, True, False, "elem", True),
    # the same scale-0 full range on k_upsample_bwd_rows (W % 4 == 0)
    Case("rows_1_to_20", 1, 2, 1, 1, 20, 20, True, False, "rows", False),
    # UPerNet's pyramid pooling bins onto a 16- and a 17-wide map
    Case("ppm_1_to_16", 1, 2, 1, 1, 16, 16, False, False, "rows", False),
    Case("ppm_2_to_16", 1, 2, 2, 2, 16, 16, False, False, "rows", False),
    Case("ppm_3_to_16", 1, 2, 3, 3, 16, 16, False, False, "rows", False),
    Case("ppm_6_to_16", 1, 2, 6, 6, 16, 16, False, False, "rows", False),
    Case("ppm_1_to_17", 1, 2, 1, 1, 17, 17, False, False, "elem", True),
    Case("ppm_2_to_17", 1, 2, 2, 2, 17, 17, False, False, "elem", True),
    Case("ppm_3_to_17", 1, 2, 3, 3, 17, 17, False, False, "elem", True),
    Case("ppm_6_to_17", 1, 2, 6, 6, 17, 17, False, False, "elem", False),
    # down-scaling on both axes (inverse scale < 1 in dcl_bilinear_out_range)
    Case("down_20x24_to_7x9", 1, 2, 20, 24, 7, 9, True, False, "elem", False),
    # mixed, W % 4 == 0: only the `H >= h && W >= w` guard of upsample_bwd keeps them off the row form
    Case("mixed_20x24_to_7x48", 1, 2, 20, 24, 7, 48, True, False, "elem", False),
    Case("mixed_5x24_to_20x8", 1, 2, 5, 24, 20, 8, True, False, "elem", False),
    # out-size 1: align_corners -> `scale == 0` branch of dcl_bilinear_out_range on that axis
    Case("out1_rows", 1, 2, 5, 8, 1, 16, True, False, "elem", False),
    Case("out1_cols", 1, 2, 5, 8, 10, 1, True, False, "elem", False),
    Case("out1_both", 1, 2, 5, 8, 1, 1, True, False, "elem", False),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
ALIGNS = [True, False]

# channel slices through the C ABI (dcl_upsample_bilinear_{fwd,bwd}_slice): N, ctot, c0, C, (h, w) -> (H, W).  wide_plane() with
# N > 1 and c0 > 0; the second target sends the forward down the scalar path and the backward to k_upsample_bwd
SLICES = [("slice_rows", 2, 11, 3, 5, 9, 13, 36, 52, "rows"), ("slice_scalar_elem", 2, 11, 3, 5, 9, 13, 30, 33, "elem")]

# upsample_concat: target (H, W), channel counts and sizes of the maps (the first has the target size).  "both_forms": an
# up-scaled map takes k_upsample_bwd_rows, the down-scaled one k_upsample_bwd at c0 = 10, in one call; "ragged": W % 4 != 0
CONCATS = [("concat_both_forms", 2, (12, 20), [(3, 12, 20), (5, 6, 10), (2, 5, 7), (4, 16, 24)]),
           ("concat_ragged", 2, (30, 33), [(2, 30, 33), (3, 8, 8), (4, 9, 13)])]


def gamma(k):
    return k * U / (1.0 - k * U)


@functools.lru_cache(maxsize=None)
def weights(n_in, n_out, align):
    """[n_out, n_in] float64: ATen's f32 weight of input i in output o along an axis of n_in -> n_out"""
    eye = torch.eye(n_in, dtype=torch.float32).view(1, n_in, 1, n_in)            # channel i = unit vector i
    m = F.interpolate(eye, size=(1, n_out), mode="bilinear", align_corners=bool(align))[0, :, 0, :]
    return m.t().contiguous().double()


def _src_np(n_in, n_out, align):
    f = np.float32
    d = np.arange(n_out, dtype=np.float32)
    if align:
        sc = f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0)
        return sc, (sc * d).astype(np.float32)
    sc = f(n_in) / f(n_out)
    # scale * (dst + 0.5) - 0.5 is ONE fused multiply-add where it is compiled with contraction: the device code of
    # csrc/dcl_bilinear.h (v_fma_f32) and ATen's vectorised CPU kernels.  Its product of two f32 values and the shift are
    # exact in float64, so one rounding to f32 restates the fused form; an unfused evaluation differs by up to 4 ulp(src)
    fused = (sc.astype(np.float64) * (d + f(0.5)).astype(np.float64) - 0.5).astype(np.float32)
    return sc, np.maximum(fused, f(0))


def weights_np(n_in, n_out, align):
    """ATen's three formulas (area_pixel_compute_scale, _source_index, the index pair and lambdas) in numpy.float32"""
    _, s = _src_np(n_in, n_out, align)
    a = np.minimum(s.astype(np.int64), n_in - 1)
    b = a + (a < n_in - 1)
    l1 = (s - a.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1) - l1).astype(np.float32)
    m = np.zeros((n_out, n_in), np.float32)
    o = np.arange(n_out)
    m[o, a] += l0
    m[o, b] += l1                       # a == b at the border: l0 + l1 in f32, as dcl_bilinear_weight() adds them
    return torch.from_numpy(m.astype(np.float64))


def src_max(n_in, n_out, align):
    """largest f32 source coordinate of the axis (its rounding error is what separates f32 from exact weights)"""
    return float(_src_np(n_in, n_out, align)[1].max())


def out_range_np(n_in, n_out, align):
    """[n_in, 2]: dcl_bilinear_out_range restated in numpy.float32 (what `nx` of k_upsample_bwd is: hi - lo + 1)"""
    f = np.float32
    sc, _ = _src_np(n_in, n_out, align)
    i = np.arange(n_in, dtype=np.float32)
    if sc <= 0:
        return np.stack([np.zeros(n_in, np.int64), np.full(n_in, n_out - 1, np.int64)], 1)
    inv = f(1) / sc
    if align:
        flo, fhi = (i - f(1)) * inv, (i + f(1)) * inv
    else:
        flo, fhi = (i - f(1) + f(0.5)) * inv - f(0.5), (i + f(1) + f(0.5)) * inv - f(0.5)
    lo = np.floor(flo).astype(np.int64) - 1
    hi = np.ceil(fhi).astype(np.int64) + 1
    return np.stack([np.clip(lo, 0, None), np.clip(hi, None, n_out - 1)], 1)


def backward_form(h, w, H, W):
    """upsample_bwd()'s choice for a 16-byte aligned gradient"""
    return "rows" if W % 4 == 0 and W <= ROWS_MAXW and H >= h and W >= w else "elem"


def k_bwd(h, w, H, W, align):
    ny = int((weights(h, H, align) != 0).sum(0).max())
    nx = int((weights(w, W, align) != 0).sum(0).max())
    return ny + nx + K_BWD_EXTRA


def forward_ref(x, add, size, align):
    """(pre-activation reference, bound), float64.  x [n, c, h, w], add [n, c, H, W] or None: CPU tensors"""
    h, w = x.shape[-2:]
    wy, wx = weights(h, size[0], align), weights(w, size[1], align)
    pre = torch.einsum("ah,nchw,bw->ncab", wy, x.double(), wx)
    mag = torch.einsum("ah,nchw,bw->ncab", wy, x.double().abs(), wx)
    k = K_FWD
    if add is not None:
        pre, mag, k = pre + add.double(), mag + add.double().abs(), k + 1
    return pre, gamma(k) * mag


def backward_ref(dy, hw, align):
    """(dx reference, bound), float64.  dy [n, c, H, W]: the gradient that reaches the interpolation (behind the ReLU's mask)"""
    h, w = hw
    H, W = dy.shape[-2:]
    wy, wx = weights(h, H, align), weights(w, W, align)
    dx = torch.einsum("ah,ncab,bw->nchw", wy, dy.double(), wx)
    mag = torch.einsum("ah,ncab,bw->nchw", wy, dy.double().abs(), wx)
    return dx, gamma(k_bwd(h, w, H, W, align)) * mag


def exact_ref(x, add, size, align):
    """interpolation with float64 weights (exact up to float64 rounding)"""
    y = F.interpolate(x.double(), size=tuple(size), mode="bilinear", align_corners=bool(align))
    return y if add is None else y + add.double()


@functools.lru_cache(maxsize=None)
def inputs(name, align):
    """(x, add or None, dy): f32 CPU tensors of the case; the addend is randn - 0.3 (a ReLU then cuts a good third)"""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(1000 * CASES.index(c) + int(align))
    x = torch.randn(c.n, c.c, c.h, c.w, generator=g)
    add = torch.randn(c.n, c.c, c.H, c.W, generator=g) - 0.3 if c.add else None
    dy = torch.randn(c.n, c.c, c.H, c.W, generator=g)
    return x, add, dy


@functools.lru_cache(maxsize=None)
def reference(name, align):
    """(pre, bound): forward_ref of the case's inputs, computed once"""
    c = BY_NAME[name]
    x, add, _ = inputs(name, align)
    return forward_ref(x, add, (c.H, c.W), align)


def ambiguous(pre, bound):
    """elements whose sign (the ReLU's mask) the forward bound leaves open"""
    return pre.abs() <= bound


def _worst(err, bound):
    """largest err / bound (inf where err > 0 = bound); for the printed figure"""
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                          torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


def check_close(got, ref, bound, what):
    err = (got.double().cpu() - ref).abs()
    worst = _worst(err, bound)
    print(f"{what}: worst |got - ref| / bound = {worst:.3f}, max err {float(err.max()):.3e}")
    bad = err > bound
    assert not bool(bad.any()), (what, int(bad.sum()), "elements outside the bound; worst ratio", worst,
                                 "first at", tuple(int(v) for v in bad.nonzero()[0]))


def verify(name, align, y, dx, dadd, dx_again=None):
    """Hold one implementation's results for a case to the reference: y [n, c, H, W], dx, dadd (None without addend), all for the
    case's inputs() and the gradient dy.  dx_again: dx of a second run, bitwise the first."""
    c = BY_NAME[name]
    x, add, dy = inputs(name, align)
    pre, fb = reference(name, align)
    y = y.detach().cpu()
    check_close(y, pre.clamp_min(0) if c.relu else pre, fb, f"{name} y")
    g = dy
    if c.relu:
        # the mask is the implementation's own sign of y where the reference cannot tell, the reference's elsewhere
        amb = ambiguous(pre, fb)
        assert float(amb.double().mean()) <= MAX_AMBIGUOUS, (name, "ambiguous share", float(amb.double().mean()))
        mask = torch.where(amb, y > 0, pre > 0)
        assert torch.equal(y > 0, mask), (name, "ReLU mask differs where the reference decides it")
        g = torch.where(mask, dy, torch.zeros_like(dy))
    if c.add:
        assert dadd is not None and torch.equal(dadd.cpu(), g), (name, "the addend's gradient is not exactly the (masked) dy")
    dref, bb = backward_ref(g, (c.h, c.w), align)
    check_close(dx, dref, bb, f"{name} dx")
    if dx_again is not None:
        assert torch.equal(dx, dx_again), (name, "dx differs between two runs")
