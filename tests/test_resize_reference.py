"""The float64 reference of the bilinear resize tests (tests/_resize_cases.py) is itself held to two independent evaluations on the
CPU, for every case of the list, so that the GPU tests cannot be green because the reference is wrong:
  - ATen's own fp32 CPU kernels (forward and autograd backward, with the ReLU and the addend) are inside the derived bound;
  - the f32-weight reference is within 4 * 2^-24 * max(src) of interpolation with exact float64 weights.
And the case list is held to the dispatch it claims: the backward form, the `nx > MAXC` loop, the forward path."""
import pytest
import torch
import torch.nn.functional as F

import _resize_cases as rc

_ALL = [(c.name, a) for c in rc.CASES for a in rc.ALIGNS]
_IDS = [f"{n}-{'align' if a else 'half'}" for n, a in _ALL]


def _axes():
    seen = set()
    for c in rc.CASES:
        seen |= {(c.h, c.H), (c.w, c.W)}
    for s in rc.SLICES:
        seen |= {(s[5], s[7]), (s[6], s[8])}
    for _, _, (H, W), maps in rc.CONCATS:
        for _, h, w in maps[1:]:
            seen |= {(h, H), (w, W)}
    seen |= {(260, 1040), (128, 512), (256, 1024), (20, 7), (8, 30), (8, 33)}
    return sorted(seen)


@pytest.mark.parametrize("align", rc.ALIGNS)
def test_weights_are_atens_formulas_and_close_to_exact(align):
    """the unit-vector weights equal the numpy.float32 restatement of ATen's three formulas (with the fused multiply-add of the
    half-pixel shift) bit for bit; every row sums to 1 within one rounding; each weight is within 4 u max(src, 1/2) of the
    float64-weight one (at most three roundings in the source coordinate -- the scale, its product, the half-pixel shift -- and one
    in l0 = 1 - l1)"""
    for n_in, n_out in _axes():
        wm = rc.weights(n_in, n_out, align)
        assert wm.shape == (n_out, n_in)
        assert torch.equal(wm, rc.weights_np(n_in, n_out, align)), (n_in, n_out, align)
        assert bool(((wm != 0).sum(1) <= 2).all()) and bool((wm >= 0).all())
        assert float((wm.sum(1) - 1).abs().max()) <= rc.U, (n_in, n_out, align)
        eye = torch.eye(n_in, dtype=torch.float64).view(1, n_in, 1, n_in)
        w64 = F.interpolate(eye, size=(1, n_out), mode="bilinear", align_corners=align)[0, :, 0, :].t()
        err = float((wm - w64).abs().max())
        assert err <= 4 * rc.U * max(rc.src_max(n_in, n_out, align), 0.5), (n_in, n_out, align, err)


@pytest.mark.parametrize("name,align", _ALL, ids=_IDS)
def test_aten_fp32_cpu_is_inside_the_bound_of_the_reference(name, align):
    """rc.verify() -- the very function the GPU tests call -- on ATen's fp32 CPU results"""
    c = rc.BY_NAME[name]
    x, add, dy = rc.inputs(name, align)
    xa = x.clone().requires_grad_(True)
    aa = add.clone().requires_grad_(True) if add is not None else None
    y = F.interpolate(xa, size=(c.H, c.W), mode="bilinear", align_corners=align)
    y = y if aa is None else aa + y
    y = torch.relu(y) if c.relu else y
    y.backward(dy)
    rc.verify(name, align, y, xa.grad, aa.grad if aa is not None else None)


@pytest.mark.parametrize("name,align", _ALL, ids=_IDS)
def test_reference_is_close_to_exact_interpolation(name, align):
    c = rc.BY_NAME[name]
    x, add, _ = rc.inputs(name, align)
    pre, _ = rc.reference(name, align)
    exact = rc.exact_ref(x, add, (c.H, c.W), align)
    smax = max(rc.src_max(c.h, c.H, align), rc.src_max(c.w, c.W, align))
    err = float((pre - exact).abs().max())
    scale = max(float(exact.abs().max()), float(x.abs().max()))
    print(f"{name}: |f32-weight ref - exact| = {err:.3e}, 4 u max(src) max|.| = {4 * rc.U * smax * scale:.3e}")
    assert err <= 4 * rc.U * smax * scale + 1e-15 * scale, (name, align, err)


@pytest.mark.parametrize("name,align", [(c.name, a) for c in rc.CASES if c.relu for a in rc.ALIGNS])
def test_relu_cases_leave_few_signs_open(name, align):
    """the share of elements whose pre-activation reference lies inside the forward bound (either mask is accepted there)"""
    pre, fb = rc.reference(name, align)
    share = float(rc.ambiguous(pre, fb).double().mean())
    assert share <= rc.MAX_AMBIGUOUS, (name, align, share)
    assert 0.2 <= float((pre > 0).double().mean()) <= 0.8            # and the ReLU does cut: both branches are well populated


def test_cases_reach_the_branches_they_name():
    """the predicates of upsample_fwd / upsample_bwd (csrc/dcl_resize.hip) restated, against what each case declares"""
    for c in rc.CASES:
        assert rc.backward_form(c.h, c.w, c.H, c.W) == c.bwd, c.name
        assert c.n * c.c * max(c.h * c.w, c.H * c.W) <= 100_000, c.name
        nx = max(int((r[:, 1] - r[:, 0] + 1).max()) for r in (rc.out_range_np(c.w, c.W, a) for a in rc.ALIGNS))
        if c.bwd == "elem":
            assert (nx > rc.MAXC) == c.nx_gt_maxc, (c.name, nx)
        for align in rc.ALIGNS:
            # the range is conservative: it covers every non-zero weight
            for n_in, n_out in ((c.h, c.H), (c.w, c.W)):
                wm = rc.weights(n_in, n_out, align)
                rr = rc.out_range_np(n_in, n_out, align)
                for i in range(n_in):
                    nz = wm[:, i].nonzero().flatten()
                    assert nz.numel() == 0 or (rr[i, 0] <= int(nz.min()) and int(nz.max()) <= rr[i, 1]), (c.name, align, i)
    names = {c.name: c for c in rc.CASES}
    # forward: tpr = min(256, 2^ceil(log2(W / 4))), trips = ceil(W / (4 tpr)); 16-byte path iff W % 4 == 0
    def trips(W):
        tpr = 1
        while tpr < 256 and tpr * 4 < W:
            tpr *= 2
        return tpr, -(-W // (4 * tpr))
    assert trips(4) == (1, 1) and (names["fwd_w4_row_tail"].c * names["fwd_w4_row_tail"].H) % 256 != 0
    assert trips(1040) == (256, 2) and trips(1030) == (256, 2) and 1030 % 4 == 2 and trips(33) == (16, 1)
    assert trips(4096)[1] == 4 and trips(4100)[1] == 5
    for s in rc.SLICES:
        assert rc.backward_form(s[5], s[6], s[7], s[8]) == s[9]
    (_, _, (H, W), maps), (_, _, (H2, W2), maps2) = rc.CONCATS
    assert {rc.backward_form(h, w, H, W) for _, h, w in maps[1:]} == {"rows", "elem"}
    assert rc.backward_form(*maps[-1][1:], H, W) == "elem" and sum(m[0] for m in maps[:-1]) > 0
    assert {rc.backward_form(h, w, H2, W2) for _, h, w in maps2[1:]} == {"elem"}
