"""csrc/dcl_resize.hip (bilinear resize forward / backward, channel slices, the fan-out sum) against the float64 reference of
tests/_resize_cases.py at its derived elementwise bound, one case per dispatch route: see the comments of the case list there.
Through models.ops.upsample_bilinear / upsample_concat / fan_out, and through the C ABI where the wrappers cannot reach a route
(channel slices off the concat's happy path, an unaligned result)."""
import pytest
import torch

import _resize_cases as rc

pytestmark = pytest.mark.gpu

_ALL = [(c.name, a) for c in rc.CASES for a in rc.ALIGNS]
_IDS = [f"{n}-{'align' if a else 'half'}" for n, a in _ALL]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib
    _lib.lib()                                   # fails loudly if libdcl_hip.so is missing
    return torch.device("cuda:0")


def _run(dev, x, add, dy, size, align, relu):
    """(y, dx, dadd) of ops.upsample_bilinear on the HIP kernels (not its F.interpolate branch)"""
    from mscs_amd.models.ops import upsample_bilinear
    xg = x.to(dev).requires_grad_(True)
    ag = add.to(dev).requires_grad_(True) if add is not None else None
    y = upsample_bilinear(xg, size, align, add=ag, relu=relu)
    assert type(y.grad_fn).__name__ == "_UpsampleBilinearBackward", type(y.grad_fn).__name__
    y.backward(dy.to(dev))
    return y.detach().cpu(), xg.grad.cpu(), (ag.grad.cpu() if ag is not None else None)


@pytest.mark.parametrize("name,align", _ALL, ids=_IDS)
def test_resize_routes_match_fp64(dev, name, align):
    c = rc.BY_NAME[name]
    x, add, dy = rc.inputs(name, align)
    y, dx, dadd = _run(dev, x, add, dy, (c.H, c.W), align, c.relu)
    _, dx2, _ = _run(dev, x, add, dy, (c.H, c.W), align, c.relu)
    rc.verify(name, align, y, dx, dadd, dx_again=dx2)


@pytest.mark.parametrize("align", rc.ALIGNS)
@pytest.mark.parametrize("offset", [1, 2])
def test_addend_at_an_odd_storage_offset(dev, align, offset):
    """W % 4 == 0 and a contiguous addend 4 / 8 bytes off a 16-byte boundary: upsample_fwd must leave the 16-byte path"""
    g = torch.Generator().manual_seed(40 + offset)
    x = torch.randn(1, 2, 5, 6, generator=g)
    add = torch.randn(1, 2, 10, 24, generator=g)
    dy = torch.randn(1, 2, 10, 24, generator=g)
    from mscs_amd.models.ops import upsample_bilinear
    base = torch.zeros(add.numel() + 4, device=dev)
    view = base[offset:offset + add.numel()].view(add.shape)
    view.copy_(add)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * offset
    xg = x.to(dev).requires_grad_(True)
    y = upsample_bilinear(xg, (10, 24), align, add=view)
    assert type(y.grad_fn).__name__ == "_UpsampleBilinearBackward"
    y.backward(dy.to(dev))
    pre, fb = rc.forward_ref(x, add, (10, 24), align)
    rc.check_close(y.detach(), pre, fb, "y")
    dref, bb = rc.backward_ref(dy, (5, 6), align)
    rc.check_close(xg.grad, dref, bb, "dx")
    assert not base[:offset].any() and not base[offset + add.numel():].any()


@pytest.mark.parametrize("align", rc.ALIGNS)
def test_result_at_an_odd_storage_offset(dev, align):
    """the C ABI with y 4 bytes off a 16-byte boundary (W % 4 == 0): scalar stores, nothing outside y touched"""
    from mscs_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(44)
    x = torch.randn(1, 3, 4, 5, generator=g)
    xg = x.to(dev)
    n = 3 * 8 * 20
    base = torch.full((n + 8,), 7.0, device=dev)
    y = base[1:1 + n].view(1, 3, 8, 20)
    assert y.data_ptr() % 16 == 4
    _lib.check(L.dcl_upsample_bilinear_fwd(_lib.ptr(xg), None, 3, 4, 5, 8, 20, 1 if align else 0, 0, _lib.ptr(y),
                                           _lib.stream_ptr(dev)), "dcl_upsample_bilinear_fwd")
    pre, fb = rc.forward_ref(x, None, (8, 20), align)
    rc.check_close(y, pre, fb, "y")
    assert bool((base[:1] == 7.0).all()) and bool((base[1 + n:] == 7.0).all())


@pytest.mark.parametrize("align", rc.ALIGNS)
@pytest.mark.parametrize("case", rc.SLICES, ids=[s[0] for s in rc.SLICES])
def test_channel_slices_match_fp64(dev, case, align):
    """dcl_upsample_bilinear_fwd_slice / _bwd_slice with N = 2 and c0 > 0: the slice of the wide tensor holds the reference, the
    channels around it keep their contents; the backward reads its gradient out of the slice in place"""
    from mscs_amd import _lib
    L = _lib.lib()
    _, N, ctot, c0, C, h, w, H, W, _ = case
    g = torch.Generator().manual_seed(50)
    x = torch.randn(N, C, h, w, generator=g)
    dyw = torch.randn(N, ctot, H, W, generator=g)
    xg, st, a = x.to(dev), _lib.stream_ptr(dev), 1 if align else 0
    wide = torch.full((N, ctot, H, W), 7.0, device=dev)
    _lib.check(L.dcl_upsample_bilinear_fwd_slice(_lib.ptr(xg), N, C, h, w, H, W, a, _lib.ptr(wide), ctot, c0, st), "fwd_slice")
    pre, fb = rc.forward_ref(x, None, (H, W), align)
    rc.check_close(wide[:, c0:c0 + C], pre, fb, "y slice")
    assert bool((wide[:, :c0] == 7.0).all()) and bool((wide[:, c0 + C:] == 7.0).all())
    dyg = dyw.to(dev)
    dxs = []
    for _ in range(2):
        dx = torch.full((N, C, h, w), 7.0, device=dev)
        _lib.check(L.dcl_upsample_bilinear_bwd_slice(_lib.ptr(dyg), ctot, c0, N, C, h, w, H, W, a, _lib.ptr(dx), st), "bwd_slice")
        dxs.append(dx.cpu())
    dref, bb = rc.backward_ref(dyw[:, c0:c0 + C], (h, w), align)
    rc.check_close(dxs[0], dref, bb, "dx")
    assert torch.equal(dxs[0], dxs[1])


@pytest.mark.parametrize("align", rc.ALIGNS)
@pytest.mark.parametrize("case", rc.CONCATS, ids=[s[0] for s in rc.CONCATS])
def test_upsample_concat_off_the_happy_path(dev, case, align):
    """ops.upsample_concat onto a target that sends one map to the row backward and a down-scaled one (c0 > 0) to the element
    backward in the same call, and onto one with W % 4 != 0"""
    from mscs_amd.models import ops
    _, N, (H, W), maps = case
    g = torch.Generator().manual_seed(60)
    xs = [torch.randn(N, c, h, w, generator=g) for c, h, w in maps]
    dy = torch.randn(N, sum(m[0] for m in maps), H, W, generator=g)
    grads = []
    for _ in range(2):
        ts = [t.to(dev).requires_grad_(True) for t in xs]
        y = ops.upsample_concat(ts, align)
        assert type(y.grad_fn).__name__ == "_UpsampleConcatBackward"
        y.backward(dy.to(dev))
        grads.append([t.grad.cpu() for t in ts])
    y, c0 = y.detach().cpu(), 0
    for i, (x, (c, h, w)) in enumerate(zip(xs, maps)):
        if i == 0:
            assert torch.equal(y[:, :c], x) and torch.equal(grads[0][0], dy[:, :c])
        else:
            pre, fb = rc.forward_ref(x, None, (H, W), align)
            rc.check_close(y[:, c0:c0 + c], pre, fb, f"y map {i}")
            dref, bb = rc.backward_ref(dy[:, c0:c0 + c], (h, w), align)
            rc.check_close(grads[0][i], dref, bb, f"dx map {i}")
            assert torch.equal(grads[0][i], grads[1][i])
        c0 += c


def test_fan_out_sums_unaligned_gradients(dev):
    """the gradients of a 630-element tensor's three consumers arrive as dim-0 narrows of torch.cat's gradient, at byte offsets 0,
    2520 and 5040: contiguous, the second off a 16-byte boundary.  Bitwise the left-to-right sum, no error from dcl_add_n."""
    from mscs_amd.models import ops
    g = torch.Generator().manual_seed(70)
    for k in (3, 5):
        x = torch.randn(630, generator=g).to(dev).requires_grad_(True)
        gy = torch.randn(k * 630, generator=g).to(dev)
        outs = ops.fan_out(x, k)
        assert len(outs) == k and all(type(o.grad_fn).__name__ == "_FanOutBackward" for o in outs)
        torch.cat(outs).backward(gy)
        ref = gy[:630].clone()
        for i in range(1, k):
            ref = ref + gy[630 * i:630 * (i + 1)]
        assert any(gy[630 * i:].data_ptr() % 16 for i in range(k))
        assert torch.equal(x.grad, ref)
