"""The fused convolution backward (libdcl_convbwd.so, include/dcl_convbwd.h) straight at the C ABI: one launch whose grid holds the
data-gradient tiles and, behind them, the weight-gradient workgroups.

For every case: (a) gx is bit for bit the separate dcl_conv3x3_f16x3 launch with the same tile, with and without addend; (b) with
the weight gradient planned for 256 workgroups dw is bit for bit dcl_wgrad3x3_f16x3 / dcl_wgrad3x3_pre_f16x3; (c) under the
automatic plan dw is within 3e-6 of max of the float64 weight gradient (the bar of test_direct_conv3x3_wgrad_matches_fp64) and the
same bits from call to call; (d) on guarded buffers (tests/_footprint.py) nothing outside gx, part and dw is written, no sentinel is
left in them and the results do not depend on what lies next to the inputs; (e) one _Conv3x3Direct backward with the switch on and
off: same gx bits, gw within the same bar, GradToken addend consumed.

Shapes: the flat form on N = 3, 96 -> 96, 20 x 40 -- ragged row tiles and strips, 6 x 2 tile pairs, data-gradient grids of 12 and 18
workgroups (no multiples of 8: the padding workgroups run) -- with the tile forced to (3, 4) and (3, 2); the wave form on N = 1,
384 -> 384, 8 x 16 (192 tile pairs)."""
import pytest
import torch

from _footprint import run_both

pytestmark = pytest.mark.gpu

BAR = 3e-6
# (N, C, H, W, tile_p, pre)
CASES = [(3, 96, 20, 40, 4, False), (3, 96, 20, 40, 2, False), (3, 96, 20, 40, 4, True), (3, 96, 20, 40, 2, True),
         (1, 384, 8, 16, 2, False), (1, 384, 8, 16, 4, True)]
IDS = [f"{n}x{c}x{h}x{w}-3x{p}{'-pre' if pre else ''}" for n, c, h, w, p, pre in CASES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib, _lib_convbwd
    _lib.lib()
    _lib_convbwd.lib()
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else t.data_ptr()


def wgrad64(op, gy):
    """float64 weight gradient of conv2d(op, w, padding=1) on the device: one batched matrix product per tap"""
    n, ci, h, w = op.shape
    co = gy.shape[1]
    xp = torch.nn.functional.pad(op.double(), (1, 1, 1, 1))
    g = gy.double().flatten(2)
    dw = torch.empty(co, ci, 3, 3, dtype=torch.float64, device=op.device)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = torch.einsum("nop,nip->oi", g, xp[:, :, ky:ky + h, kx:kx + w].flatten(2))
    return dw


_DATA = {}


def data(dev, case):
    """inputs of a case and its references (separate launches, float64), computed once and left unchanged"""
    if case in _DATA:
        return _DATA[case]
    from mscs_amd import _lib
    from mscs_amd.models import ops_conv
    n, c, h, w, tp, pre = case
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(sum(case[:5]) + 7 * int(pre))
    d = {}
    d["x"] = x = (torch.randn(n, c, h, w, device=dev, generator=g).relu_() * 2.5) if not pre else torch.randn(n, c, h, w, device=dev, generator=g) * 2.5
    d["w"] = wt = torch.randn(c, c, 3, 3, device=dev, generator=g) / (3.0 * c ** 0.5)
    d["gy"] = gy = torch.randn(n, c, h, w, device=dev, generator=g) * 3e-5
    d["addend"] = addend = torch.randn(n, c, h, w, device=dev, generator=g) * 1e-4
    d["sc"] = sc = (torch.rand(c, device=dev, generator=g) + 0.5) if pre else None
    d["sh"] = sh = (torch.randn(c, device=dev, generator=g) * 0.5) if pre else None
    op = torch.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)) if pre else x
    d["xamax"] = xa = op.abs().max().reshape(1)
    d["gamax"] = ga = gy.abs().max().reshape(1)
    d["wamax"] = wa = wt.abs().max().reshape(1)
    d["wpt"] = wpt = ops_conv.conv3x3_pack(wt, wa, transposed=True)
    # the separate launches: data gradient with the same tile, weight gradient at its own plan
    for key, ad in (("gx", None), ("gx_add", addend)):
        out = torch.empty_like(x)
        _lib.check(L.dcl_conv3x3_f16x3(_p(gy), n, c, h, w, _p(wpt), c, _p(ga), 1, _p(wa), _p(ad), None, _p(out), 1, 1, h, w, 3, tp, st),
                   "dcl_conv3x3_f16x3")
        d[key] = out
    part = torch.empty(L.dcl_wgrad3x3_splits(n, c, c, h, w, 1) * 9 * c * c, device=dev)
    dw = torch.empty(c, c, 3, 3, device=dev)
    if pre:
        _lib.check(L.dcl_wgrad3x3_pre_f16x3(_p(x), _p(gy), n, c, c, h, w, _p(xa), 1, _p(ga), 1, _p(sc), _p(sh), 1, _p(part), _p(dw), st),
                   "dcl_wgrad3x3_pre_f16x3")
    else:
        _lib.check(L.dcl_wgrad3x3_f16x3(_p(x), _p(gy), n, c, c, h, w, _p(xa), 1, _p(ga), 1, 1, _p(part), _p(dw), st), "dcl_wgrad3x3_f16x3")
    d["dw"] = dw
    d["dw64"] = wgrad64(op, gy)
    torch.cuda.synchronize()
    _DATA[case] = d
    return d


def fused(dev, case, d, addend, wg_target, bufs=None):
    """one dcb_conv3x3_bwd_f16x3 call; bufs = (tensors by name, gx, part, dw) on buffers of the caller's"""
    from mscs_amd import _lib_convbwd as cb
    n, c, h, w, tp, pre = case
    L, st = cb.lib(), cb.stream_ptr(dev)
    slabs = cb.wgrad_splits(n, c, c, h, w, 3, tp, wg_target)
    assert slabs > 0
    if bufs is None:
        t = d
        gx, part, dw = torch.empty_like(d["x"]), torch.empty(slabs * 9 * c * c, device=dev), torch.empty(c, c, 3, 3, device=dev)
    else:
        t, gx, part, dw = bufs
    cb.check(L.dcb_conv3x3_bwd_f16x3(_p(t["gy"]), _p(t["wpt"]), _p(t["x"]), n, c, c, h, w, _p(t["gamax"]), 1, _p(t["wamax"]),
                                     _p(t["xamax"]), 1, _p(addend), _p(t["sc"]), _p(t["sh"]), 3, tp, wg_target, _p(gx), _p(part), _p(dw),
                                     st), "dcb_conv3x3_bwd_f16x3")
    return gx, part, dw


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fused_equals_separate_launches(dev, case):
    d = data(dev, case)
    gx, _, dw = fused(dev, case, d, None, 256)
    assert torch.equal(gx, d["gx"]), "data gradient differs from dcl_conv3x3_f16x3"
    assert torch.equal(dw, d["dw"]), "weight gradient at the 256-workgroup plan differs from the separate entry"
    gx, _, dw = fused(dev, case, d, d["addend"], 256)
    assert torch.equal(gx, d["gx_add"]) and torch.equal(dw, d["dw"])
    gx, _, _ = fused(dev, case, d, d["addend"], 0)
    assert torch.equal(gx, d["gx_add"]), "the data gradient must not depend on the weight gradient's plan"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_automatic_plan_matches_fp64(dev, case):
    from mscs_amd import _lib_convbwd as cb
    n, c, h, w, tp, pre = case
    p = cb.plan(n, c, c, h, w, 3, tp, 0)
    assert p["nd"] % 8 != 0 and p["nd8"] + p["wgrad_grid"] <= cb.CUS and bool(p["wave_mode"]) == (c == 384)
    d = data(dev, case)
    _, _, dw = fused(dev, case, d, None, 0)
    err = ((dw.double() - d["dw64"]).abs().max() / d["dw64"].abs().max()).item()
    print(f"{IDS[CASES.index(case)]}: plan {p}, |dw - dw64| / max = {err:.3e}")
    assert err < BAR
    assert torch.equal(dw, fused(dev, case, d, d["addend"], 0)[2]), "not the same bits from call to call"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_footprint(dev, case):
    from mscs_amd import _lib_convbwd as cb
    n, c, h, w, tp, pre = case
    d = data(dev, case)
    slabs = cb.wgrad_splits(n, c, c, h, w, 3, tp, 0)

    def body(ar):
        t = {k: (ar.inp(d[k], k) if d[k] is not None else None) for k in ("gy", "wpt", "x", "gamax", "wamax", "xamax", "sc", "sh")}
        addend = ar.inp(d["addend"], "addend")
        gx, part, dw = ar.out((n, c, h, w), name="gx"), ar.out(slabs * 9 * c * c, name="part"), ar.out((c, c, 3, 3), name="dw")
        fused(dev, case, d, addend, 0, (t, gx, part, dw))
        return {"gx": gx, "part": part, "dw": dw}
    got = run_both(dev, body, ("convbwd", case))
    assert torch.equal(got["gx"], d["gx_add"])
    assert ((got["dw"].double() - d["dw64"]).abs().max() / d["dw64"].abs().max()).item() < BAR


def test_backward_through_python_switch_on_and_off(dev, monkeypatch):
    """_Conv3x3Direct.backward on the 192-channel BasicBlock shape: the fused entry when the switch is on, today's two launches when
    it is off"""
    from mscs_amd import _lib_convbwd as cb
    from mscs_amd.models import ops, ops_conv
    n, c, h, w = 12, 192, 32, 64
    assert cb.supported(n, c, c, h, w)
    torch.manual_seed(5)
    conv = torch.nn.Conv2d(c, c, 3, padding=1, bias=False).to(dev)
    ops.use_direct_conv3x3(conv)
    assert isinstance(conv, ops_conv.DirectConv2d)
    x0 = torch.randn(n, c, h, w, device=dev).relu_() * 2.5
    gy = torch.randn(n, c, h, w, device=dev) * 3e-5
    dres = torch.randn(n, c, h, w, device=dev) * 1e-4
    res = {}
    for on in (True, False):
        monkeypatch.setattr(ops_conv, "FUSE_CONV_BWD", on)
        conv.weight.grad = None
        x = x0.clone().requires_grad_(True)
        tok = ops_conv.GradToken()
        before = cb.calls["bwd"]
        y = conv(x, grad_token=tok)
        tok.dres = dres.clone()
        y.backward(gy)
        assert tok.dres is None, "GradToken addend not consumed"
        assert cb.calls["bwd"] - before == (1 if on else 0)
        res[on] = (x.grad.clone(), conv.weight.grad.clone())
    assert torch.equal(res[True][0], res[False][0])
    dw64 = wgrad64(x0, gy)
    for on in (True, False):
        err = ((res[on][1].double() - dw64).abs().max() / dw64.abs().max()).item()
        print(f"switch {'on' if on else 'off'}: |gw - gw64| / max = {err:.3e}")
        assert err < BAR
