"""Footprint of the dilated-convolution entries at the C ABI (include/dcl_dconv.h): ddc_pack / ddc_fwd / ddc_dgrad / ddc_wgrad on
guarded buffers (tests/_footprint.py): every band intact, every output fully written, finite and independent of what lies outside
the inputs, workspaces of exactly ddc_workspace_bytes whose bands stay untouched, and a workspace one byte short refused before
anything is launched."""
import pytest
import torch

from _footprint import run_both

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_dconv
    _lib_dconv.lib()
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else t.data_ptr()


# (N, Ci, Co, H, W, d): partly live taps; centre tap only; several tiles, chunks and slabs with partial last ones
CASES = [(2, 48, 16, 13, 17, 6), (1, 16, 16, 8, 8, 12), (2, 48, 80, 23, 29, 4)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_dconv_entries_footprint(dev, case):
    from mscs_amd import _lib_dconv as ld
    from mscs_amd.models.ops_dconv import DilatedConv2d, _DilatedConv3x3
    N, Ci, Co, H, W, d = case
    L = ld.lib()
    st = ld.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(sum(case))
    x = torch.randn(N, Ci, H, W, device=dev, generator=g)
    w = torch.randn(Co, Ci, 3, 3, device=dev, generator=g) / (3.0 * Ci ** 0.5)
    bias = torch.randn(Co, device=dev, generator=g)
    dy = torch.randn(N, Co, H, W, device=dev, generator=g)
    nf, nd, nw = (ld.workspace_bytes(op, *case) for op in (ld.FWD, ld.DGRAD, ld.WGRAD))
    bp, bpt = ld.packed_bytes(Co, Ci, False), ld.packed_bytes(Co, Ci, True)
    assert nf == 256 and nd == 256 and nw > 512 and bp > 0 and bpt > 0

    def body(ar):
        wg = ar.inp(w, "w")
        wamax = ar.out((1,), name="wamax")
        wp, wpt = ar.out(bp, torch.uint8, "wp"), ar.out(bpt, torch.uint8, "wpt")
        ld.check(L.ddc_pack(_p(wg), Co, Ci, _p(wamax), _p(wp), _p(wpt), st), "ddc_pack")
        xg, dyg, bg = ar.inp(x, "x"), ar.inp(dy, "dy"), ar.inp(bias, "bias")
        w1 = ar.out(nf, torch.uint8, "workspace fwd")
        assert w1.data_ptr() % 256 == 0
        y = ar.out((N, Co, H, W), name="y")
        ld.check(L.ddc_fwd(_p(xg), _p(wp), _p(wamax), _p(bg), N, Ci, Co, H, W, d, _p(w1), nf, _p(y), st), "ddc_fwd")
        w2 = ar.out(nd, torch.uint8, "workspace dgrad")
        dx = ar.out((N, Ci, H, W), name="dx")
        ld.check(L.ddc_dgrad(_p(dyg), _p(wpt), _p(wamax), N, Ci, Co, H, W, d, _p(w2), nd, _p(dx), st), "ddc_dgrad")
        w3 = ar.out(nw, torch.uint8, "workspace wgrad")
        assert w3.data_ptr() % 256 == 0
        dw = ar.out((Co, Ci, 3, 3), name="dw")
        ld.check(L.ddc_wgrad(_p(xg), _p(dyg), N, Ci, Co, H, W, d, _p(w3), nw, _p(dw), st), "ddc_wgrad")
        return {"wamax": wamax, "wp": wp, "wpt": wpt, "y": y, "dx": dx, "dw": dw}
    got = run_both(dev, body, ("dconv", case))
    assert float(got["wamax"]) == float(w.abs().max())

    # and the values are those of the autograd Function (which takes the same entries through torch-allocated buffers)
    mod = DilatedConv2d(Ci, Co, 3, padding=d, dilation=d).to(dev)
    with torch.no_grad():
        mod.weight.copy_(w)
        mod.bias.copy_(bias)
    xa = x.clone().requires_grad_(True)
    y = _DilatedConv3x3.apply(xa, mod.weight, mod.bias, mod)
    y.backward(dy)
    assert torch.equal(got["y"], y.detach()) and torch.equal(got["dx"], xa.grad) and torch.equal(got["dw"], mod.weight.grad)
    _, wp, wpt = mod.packed_weights()
    assert torch.equal(got["wp"], wp) and torch.equal(got["wpt"], wpt)

    # a too small workspace is refused before anything is launched
    ws = torch.empty(nw, dtype=torch.uint8, device=dev)
    wamax = got["wamax"]
    scratch = torch.empty_like(y), torch.empty_like(x), torch.empty_like(w)
    assert L.ddc_fwd(_p(x), _p(wp), _p(wamax), None, N, Ci, Co, H, W, d, _p(ws), nf - 1, _p(scratch[0]), st) != 0
    assert b"workspace" in L.ddc_last_error()
    assert L.ddc_dgrad(_p(dy), _p(wpt), _p(wamax), N, Ci, Co, H, W, d, _p(ws), nd - 1, _p(scratch[1]), st) != 0
    assert b"workspace" in L.ddc_last_error()
    assert L.ddc_wgrad(_p(x), _p(dy), N, Ci, Co, H, W, d, _p(ws), nw - 1, _p(scratch[2]), st) != 0
    assert b"workspace" in L.ddc_last_error()
