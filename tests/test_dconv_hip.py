"""The dilated 3x3 convolution kernels (csrc/dcl_dconv.hip) through their autograd Function against the float64 convolution of the same
fp32 inputs; run-to-run equality; the reference's recorded ASPP values (fixtures G16) on the device; one dilated Bottleneck and the
ASPP three ways (kernels, eager, float64); training steps of the whole DeepLabv3.

Tiles of the kernels (include/dcl_dconv.h): a workgroup owns DDC_TILE_CO = 64 output channels of DDC_TILE_P = 128 pixels (a wave: 32
pixels), input channels go in chunks of DDC_CHUNK_CI = 16; the weight gradient works on DDC_WG_TILE = 32 square channel tiles over
units of DDC_WG_CHUNK_P = 16 pixels, cut into slabs.  The shapes below cover the smallest one, odd sizes, Co that is no multiple of
32, every kind of live-tap mask, a 1 x 1 map, and one shape built from the constants with several (partial) tiles and slabs.

Tolerance of the operator tests: the project's bar for its 3x3 kernels (tests/test_model_ops_parity.py),
    max|HIP - fp64| <= 3e-6 max|fp64|        for y, dx and dW.
Every comparison prints its distances."""
import copy

import pytest
import torch
import torch.nn.functional as F

import _aspp_golden as ag

pytestmark = pytest.mark.gpu

BAR = 3e-6
FLOOR = 8 * 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib, _lib_dconv
    _lib.lib()
    _lib_dconv.lib()
    return torch.device("cuda:0")


class _switch:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from mscs_amd.debug import cfg as dbg
        self.keep, dbg.dconv_hip = dbg.dconv_hip, self.on

    def __exit__(self, *a):
        from mscs_amd.debug import cfg as dbg
        dbg.dconv_hip = self.keep


def _multi_tile():
    """More than one tile along pixels, output channels and input-channel chunks, the last of each partial, and several slabs."""
    from mscs_amd import _lib_dconv as ld
    co = ld.TILE_CO + 16                        # one full tile + a quarter: the second tile's upper row tile does not exist
    ci = 3 * ld.CHUNK_CI                        # three chunks; 48 = one weight-gradient tile + half of one
    h, w = 23, 29                               # 667 pixels = 5 tiles of 128 + 27, = 41 units of 16 + 11
    assert h * w > 2 * ld.TILE_P and (h * w) % ld.TILE_P and (h * w) % ld.WG_CHUNK_P and ci % ld.WG_TILE and co % ld.WG_TILE
    return (2, ci, co, h, w, 4)


def _inputs(shape, seed, bias=False, xs=1.0, ws=1.0):
    n, ci, co, h, w, d = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, ci, h, w, generator=g) * xs
    wt = torch.randn(co, ci, 3, 3, generator=g) * ws / (3.0 * ci ** 0.5)
    b = torch.randn(co, generator=g) * xs * ws if bias else None
    cot = torch.randn(n, co, h, w, generator=g)
    return x, wt, b, cot


def _fp64(x, wt, b, cot, d):
    x, wt, cot = x.double().requires_grad_(True), wt.double().requires_grad_(True), cot.double()
    y = F.conv2d(x, wt, None if b is None else b.double(), stride=1, padding=d, dilation=d)
    y.backward(cot)
    return {"y": y.detach(), "dx": x.grad, "dw": wt.grad}


def _hip(dev, x, wt, b, cot, d):
    from mscs_amd.models.ops_dconv import DilatedConv2d, _DilatedConv3x3
    co, ci = wt.shape[:2]
    mod = DilatedConv2d(ci, co, 3, padding=d, dilation=d, bias=b is not None).to(dev)
    with torch.no_grad():
        mod.weight.copy_(wt)
        if b is not None:
            mod.bias.copy_(b)
    xd = x.to(dev).requires_grad_(True)
    y = _DilatedConv3x3.apply(xd, mod.weight, mod.bias, mod)        # (the Function itself: d = 1 is the library's, not the module's)
    y.backward(cot.to(dev))
    torch.cuda.synchronize()
    out = {"y": y.detach().cpu(), "dx": xd.grad.cpu(), "dw": mod.weight.grad.cpu()}
    if b is not None:
        out["db"] = mod.bias.grad.cpu()
    return out


def _check(what, got, ref):
    bad = []
    for k, r in ref.items():
        assert bool(torch.isfinite(got[k]).all()), (what, k, "not finite")
        den = float(r.abs().max())
        e = float((got[k].double() - r).abs().max()) / den
        print(f"{what} {k}: {e:.3e} of max (bar {BAR:.1e})")
        if not e <= BAR:
            bad.append((k, e))
    assert not bad, (what, bad)


def _twice(dev, shape, seed, **kw):
    from mscs_amd import _lib_dconv as ld
    x, wt, b, cot = _inputs(shape, seed, **kw)
    assert ld.supported(*shape)
    before = dict(ld.calls)
    one = _hip(dev, x, wt, b, cot, shape[5])
    two = _hip(dev, x, wt, b, cot, shape[5])
    assert {k: ld.calls[k] - before[k] for k in before} == {"fwd": 2, "dgrad": 2, "wgrad": 2}
    for k in one:
        assert torch.equal(one[k], two[k]), (shape, k, "differs from run to run")
    return one, _fp64(x, wt, b, cot, shape[5]), (x, wt, b, cot)


SHAPES = [(2, 16, 16, 5, 7, 1), (1, 32, 48, 9, 13, 2), (2, 48, 16, 13, 17, 6), (1, 16, 32, 13, 17, 12), (1, 16, 16, 1, 1, 3)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_matches_fp64_and_is_reproducible(dev, shape):
    got, ref, _ = _twice(dev, shape, 100 + sum(shape))
    _check(shape, got, ref)


def test_centre_tap_only_is_a_1x1_convolution(dev):
    from mscs_amd import _lib_dconv as ld
    shape = (1, 16, 16, 8, 8, 12)
    assert ld.live_taps(8, 8, 12) == 1 << 4
    got, ref, (x, wt, b, cot) = _twice(dev, shape, 7)
    _check(shape, got, ref)
    y1 = F.conv2d(x.double(), wt.double()[:, :, 1:2, 1:2])
    e = float((got["y"].double() - y1).abs().max() / y1.abs().max())
    print(f"{shape} y against the 1x1 convolution: {e:.3e}")
    assert e <= BAR
    dead = torch.ones(3, 3, dtype=torch.bool)
    dead[1, 1] = False
    assert bool((got["dw"][:, :, dead] == 0.0).all()), "a dead tap's weight gradient is not exactly zero"
    assert float(got["dw"][:, :, 1, 1].abs().max()) > 0


def test_several_tiles_chunks_and_slabs(dev):
    from mscs_amd import _lib_dconv as ld
    shape = _multi_tile()
    assert ld.wgrad_slabs(*shape) > 1, "the weight gradient of this shape was meant to use more than one slab"
    got, ref, _ = _twice(dev, shape, 11)
    _check(shape, got, ref)


def test_slab_cut_inside_an_image(dev):
    """One image of 33 x 33: 69 units in 2 slabs of 35, so the first slab ends, and the second starts, in the middle of the image (in
    the several-tiles shape above the cut falls between the two images)."""
    from mscs_amd import _lib_dconv as ld
    shape = (1, 16, 32, 33, 33, 3)
    units = -(-33 * 33 // ld.WG_CHUNK_P)
    slabs = ld.wgrad_slabs(*shape)
    assert slabs == 2 and -(-units // slabs) % units != 0
    got, ref, _ = _twice(dev, shape, 19)
    _check(shape, got, ref)
    shape = (3, 16, 16, 21, 21, 2)              # 3 x 28 units in 2 slabs of 42: the cut halves the middle image
    assert ld.wgrad_slabs(*shape) == 2 and (3 * -(-21 * 21 // ld.WG_CHUNK_P) // 2) % -(-21 * 21 // ld.WG_CHUNK_P) != 0
    got, ref, _ = _twice(dev, shape, 23)
    _check(shape, got, ref)


def test_contiguous_view_at_an_odd_offset_is_taken(dev):
    """x[:, 1:17] of one image with H W = 35: contiguous, 4-byte but not 16-byte aligned; the module takes it (the kernels read
    one float at a time) and gives what it gives for an aligned copy, bitwise."""
    from mscs_amd import _lib_dconv as ld
    from mscs_amd.models.ops_dconv import DilatedConv2d
    g = torch.Generator().manual_seed(29)
    big = torch.randn(1, 18, 5, 7, generator=g).to(dev)
    view = big[:, 1:17]
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    mod = DilatedConv2d(16, 16, 3, padding=2, dilation=2).to(dev)
    assert mod.eligible(view)
    before = dict(ld.calls)
    outs = []
    for x in (view, view.clone()):
        x = x.detach().requires_grad_(True) if x is not view else view.detach().requires_grad_(True)
        mod.zero_grad(set_to_none=True)
        y = mod(x)
        y.backward(torch.ones_like(y))
        outs.append((y.detach().clone(), x.grad.clone(), mod.weight.grad.clone()))
    assert ld.calls["fwd"] == before["fwd"] + 2 and ld.calls["wgrad"] == before["wgrad"] + 2
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    ref = F.conv2d(view.double(), mod.weight.detach().double(), mod.bias.detach().double(), 1, 2, 2)
    assert float((outs[0][0].double() - ref).abs().max() / ref.abs().max()) <= BAR


def test_bias(dev):
    shape = (1, 32, 48, 9, 13, 2)
    got, ref, (x, wt, b, cot) = _twice(dev, shape, 13, bias=True)
    _check(shape, got, ref)
    assert torch.allclose(got["db"].double(), cot.double().sum((0, 2, 3)), rtol=1e-5, atol=1e-5)


def test_operands_2_to_the_20_apart_keep_their_scales(dev):
    shape = (2, 48, 16, 13, 17, 6)
    got, ref, _ = _twice(dev, shape, 17, xs=2.0 ** 10, ws=2.0 ** -10)
    _check(shape, got, ref)


# ---- module level: the reference's recorded values -----------------------------------------------------------------------------

@pytest.mark.parametrize("case", ag.CASES)
def test_aspp_fixtures_on_device_match_the_reference(dev, case):
    """G16 on the device with the switch on; the ``calls`` counters prove that the library ran.  The bars are those
    tests/test_ocr_hip.py holds G15 to: the float64 modules on the device must reproduce the record to 1e-4 or to the noise the eager
    path shows, and behind the batch norms (few samples: the pooled branch's sees B = 2 values per channel)
        max|HIP - fp64| / max|fp64| <= 3 * max over all tensors of max(e_eager, e_record),   at least 8 * 2^-23."""
    from mscs_amd import _lib_dconv as ld
    g = ag.load(case)
    before = dict(ld.calls)
    with _switch(False):
        ref = ag.run(ag.build(g, dev, torch.float64), g, dev, torch.float64)
        eager_run = ag.run(ag.build(g, dev), g, dev)
    assert before == ld.calls, "debug.cfg.dconv_hip = False still called the library"
    record, eager = ag.distances(ag.golden(g), ref), ag.distances(eager_run, ref)
    for k, v in record.items():
        assert v <= max(1e-4, 3 * max(eager.values())), ("the float64 modules on the device are off the reference's record", k, v)
    with _switch(True):
        hip_run = ag.run(ag.build(g, dev), g, dev)
    assert {k: ld.calls[k] - before[k] for k in before} == {"fwd": 3, "dgrad": 3, "wgrad": 3}, "the HIP path was not taken"
    d = ag.distances(hip_run, ref)
    bar = max(3 * max(max(eager[k], record[k]) for k in d), FLOOR)
    bad = []
    for k, v in d.items():
        print(f"G16 {case} {k}: hip {v:.3e} eager {eager[k]:.3e} record {record[k]:.3e} bar {bar:.3e}")
        if not v <= bar:
            bad.append((k, v, eager[k], bar))
    assert not bad, (case, bad)


@pytest.mark.parametrize("case", ag.CASES)
def test_aspp_fixtures_with_running_statistics_hold_the_bar_per_tensor(dev, case):
    """As tests/test_ocr_hip.py does for G15: the same module, weights and inputs with the norms on their running statistics (an
    affine map per channel, no few-sample amplification): every output and gradient, tensor by tensor, against float64 on the device,
        max|HIP - fp64| / max|fp64| <= max(3 e_eager, 8 * 2^-23)."""
    from mscs_amd import _lib_dconv as ld
    g = ag.load(case)
    with _switch(False):
        ref = ag.run(ag.build(g, dev, torch.float64, train=False), g, dev, torch.float64)
        eager = ag.distances(ag.run(ag.build(g, dev, train=False), g, dev), ref)
    before = dict(ld.calls)
    with _switch(True):
        d = ag.distances(ag.run(ag.build(g, dev, train=False), g, dev), ref)
    assert all(ld.calls[k] == before[k] + 3 for k in before), "the HIP path was not taken"
    bad = []
    for k, v in d.items():
        bar = max(3 * eager[k], FLOOR)
        print(f"G16 {case} eval {k}: hip {v:.3e} eager {eager[k]:.3e} bar {bar:.3e}")
        if not v <= bar:
            bad.append((k, v, eager[k], bar))
    assert not bad, (case, bad)


def _three_ways(dev, what, make, run):
    """kernels on, DCL_DCONV_HIP = 0 and float64: the kernels' distance from float64 may be at most twice the eager fp32 path's plus
    1e-6 (of the tensor's maximum), for the output and every gradient -- a different summation order of the same fp32-equivalent
    products can cost that much, no more."""
    from mscs_amd import _lib_dconv as ld
    with _switch(False):
        ref = run(make(torch.float64), torch.float64)
        before = dict(ld.calls)
        off = run(make(torch.float32), torch.float32)
        assert before == ld.calls
    with _switch(True):
        on = run(make(torch.float32), torch.float32)
    assert all(ld.calls[k] > before[k] for k in before), "the HIP path was not taken"
    bad = []
    for k, r in ref.items():
        den = float(r.abs().max()) or 1.0
        e_on = float((on[k].double() - r).abs().max()) / den
        e_off = float((off[k].double() - r).abs().max()) / den
        print(f"{what} {k}: kernels {e_on:.3e} eager {e_off:.3e} bar {2 * e_off + 1e-6:.3e}")
        if not e_on <= 2 * e_off + 1e-6:
            bad.append((k, e_on, e_off))
    assert not bad, (what, bad)


def test_dilated_layer4_bottleneck_three_ways(dev):
    """The gradient of a ReLU is discontinuous at 0: two evaluations that differ by one rounding in a ReLU input next to 0 differ by
    a whole cotangent element there (seen on the card with the default norm biases of 0: one of 600 k ReLU inputs changed sign and
    moved dx by 0.22 of its maximum, on an output that agreed to 1e-6).  A comparison of gradients between arithmetics measures the
    arithmetic only where all of them take the same mask, so the block is evaluated with norm biases of 3, 3 and 5 (weights 1;
    bn3's output meets the residual, a unit normal, before its ReLU): about one ReLU input in a thousand is negative, so the masks
    still cut, and the density of inputs next to 0 is that of a normal variable 3 to 3.5 deviations out, which over 6e5 inputs
    leaves an expectation below 0.03 of finding one within tau.  That is asserted, not assumed, on the float64 evaluation: every
    ReLU input is farther from 0 than tau = 2 * 3e-6 * max|input|, twice the operator bar of this file (float64 on the CPU gives a
    nearest input of 1.8e-3, 3.1e-4 and 9.7e-3 behind the three norms, against tau of 4.2e-5, 4.0e-5 and 6.8e-5)."""
    from mscs_amd.models.ResNet import Bottleneck
    from mscs_amd.models.ops import use_direct_conv1x1
    from mscs_amd.models.ops_dconv import DilatedConv2d, use_dilated_conv3x3
    torch.manual_seed(3)
    proto = Bottleneck(2048, 512, dilation=2)
    with torch.no_grad():
        for bn, shift in ((proto.bn1, 3.0), (proto.bn2, 3.0), (proto.bn3, 5.0)):
            bn.bias.fill_(shift)
    state = copy.deepcopy(proto.state_dict())
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(2, 2048, 9, 11, generator=g)
    cot = torch.randn(2, 2048, 9, 11, generator=g)

    def make(dtype):
        m = Bottleneck(2048, 512, dilation=2)
        m.load_state_dict(state, strict=True)
        use_direct_conv1x1(use_dilated_conv3x3(m))
        assert type(m.conv2) is DilatedConv2d
        return m.to(dev).to(dtype).train()

    def run(m, dtype):
        x = x0.to(dev).to(dtype).requires_grad_(True)
        pre = {}
        if dtype == torch.float64:          # the ReLU inputs: the norms' outputs before the in-place ReLU (bn3's: plus the residual)
            for name in ("bn1", "bn2", "bn3"):
                getattr(m, name).register_forward_hook(lambda mod, inp, out, name=name: pre.__setitem__(name, out.detach().clone()))
        y = m(x)
        y.backward(cot.to(dev).to(dtype))
        if pre:
            pre["bn3"] = pre["bn3"] + x.detach()
            for name, v in pre.items():
                nearest, tau = float(v.abs().min()), 2 * BAR * float(v.abs().max())
                print(f"layer4 bottleneck ReLU behind {name}: nearest input to 0 {nearest:.3e}, tau {tau:.3e}, "
                      f"{float((v < 0).double().mean()):.2e} of the inputs negative")
                assert nearest > tau, (name, nearest, tau, "a ReLU input of the float64 evaluation lies at the kink")
                assert bool((v < 0).any()), (name, "the mask cuts nothing")
        res = {"out": y.detach().cpu(), "dx": x.grad.cpu()}
        res.update({"g:" + k: p.grad.cpu() for k, p in m.named_parameters()})
        return res
    _three_ways(dev, "layer4 bottleneck", make, run)


def test_dilated_layer4_bottleneck_on_the_common_mask(dev):
    """The same block at its default norm biases (half of the ReLU inputs negative, as in training), with the kink taken out the
    other way: the float64 evaluation records the mask of each of the three ReLUs, and the two fp32 evaluations multiply by THAT mask
    instead of taking their own (for float64 the product is its ReLU).  Every arithmetic then differentiates the same function, a
    sign that flips next to 0 moves the output by the rounding that flipped it and no gradient by more, and the bound measures the
    arithmetic on the fully masked path."""
    from mscs_amd.models.ResNet import Bottleneck
    from mscs_amd.models.ops import use_direct_conv1x1
    from mscs_amd.models.ops_dconv import DilatedConv2d, use_dilated_conv3x3
    torch.manual_seed(5)
    state = copy.deepcopy(Bottleneck(2048, 512, dilation=2).state_dict())
    g = torch.Generator().manual_seed(6)
    x0 = torch.randn(2, 2048, 9, 11, generator=g)
    cot = torch.randn(2, 2048, 9, 11, generator=g)
    masks = {}

    def make(dtype):
        m = Bottleneck(2048, 512, dilation=2)
        m.load_state_dict(state, strict=True)
        use_direct_conv1x1(use_dilated_conv3x3(m))
        assert type(m.conv2) is DilatedConv2d
        return m.to(dev).to(dtype).train()

    def run(m, dtype):
        def cut(name, t):
            if dtype == torch.float64:
                masks[name] = t.detach() > 0
            return t * masks[name].to(dtype)
        x = x0.to(dev).to(dtype).requires_grad_(True)
        o = cut("relu1", m.bn1(m.conv1(x)))
        o = cut("relu2", m.bn2(m.conv2(o)))
        y = cut("relu3", m.bn3(m.conv3(o)) + x)
        y.backward(cot.to(dev).to(dtype))
        if dtype == torch.float64:
            print("layer4 bottleneck, common mask: negative share", {k: round(float((~v).double().mean()), 3) for k, v in masks.items()})
            assert all(0.3 < float((~v).double().mean()) < 0.7 for v in masks.values())
        res = {"out": y.detach().cpu(), "dx": x.grad.cpu()}
        res.update({"g:" + k: p.grad.cpu() for k, p in m.named_parameters()})
        return res
    _three_ways(dev, "layer4 bottleneck, common mask", make, run)


def test_aspp_case_b_three_ways(dev):
    g = ag.load("b")

    def run(m, dtype):
        out, gx, gps = ag.run(m, g, dev, dtype)
        res = {"out": out, "gx0": gx}
        res.update({"g:" + k: v for k, v in gps.items()})
        return res
    _three_ways(dev, "ASPP b", lambda dtype: ag.build(g, dev, dtype), run)


# ---- model level -----------------------------------------------------------------------------------------------------------------

def _step(dev, out_stride, state):
    from mscs_amd.models import DeepLabv3
    graph = {"dataset": "CITYSCAPES", "backbone": "resnet50", "pretrained": False, "out_stride": out_stride}
    model = DeepLabv3(graph, 1)
    if state is not None:
        model.load_state_dict(state, strict=True)
    state = copy.deepcopy(model.state_dict())
    model = model.to(dev).train()
    g = torch.Generator().manual_seed(0)
    img = torch.randn(2, 3, 65, 97, generator=g).to(dev)
    lbl = torch.randint(0, 19, (2, 65, 97), generator=g).to(dev)
    out = model(img)
    loss = F.cross_entropy(out, lbl)
    loss.backward()
    torch.cuda.synchronize()
    res = {"logits": out.detach(), "loss": loss.detach().reshape(1)}
    res.update({"g:" + n: p.grad.detach() for n, p in model.named_parameters() if p.grad is not None})
    return res, state, model


def _vendor_weight_gradients(model, img_hw):
    """{parameter name: reason} of the weight gradients of one step that do not run on this package's kernels, from the model and
    the image size: the 7x7 stem, and the 3x3 convolutions at stride 2 whose input map is not a multiple of 8 wide (DirectConv2d
    leaves those to aten::convolution_backward: models/ops_conv.py conv3x3_wgrad_supported).  A weight gradient enters nothing
    else, so these names are the whole exception."""
    names = {"backbone.conv1.weight": "7x7 stem: the vendor library's weight gradient"}
    w = ((img_hw[1] - 1) // 2 + 1 - 1) // 2 + 1             # behind the stem and the max-pool
    for L in ("layer1", "layer2", "layer3", "layer4"):
        conv2 = getattr(model.backbone, L)[0].conv2
        if conv2.stride == (2, 2):
            if w % 8:
                names[f"backbone.{L}.0.conv2.weight"] = f"3x3 at stride 2 on a map {w} wide: aten::convolution_backward"
            w = (w - 1) // 2 + 1
    return names


@pytest.mark.parametrize("out_stride", [16, 8])
def test_whole_deeplabv3_training_step(dev, out_stride):
    """ResNet-50, 2 x 3 x 65 x 97, CE + backward, twice from the same state: the logits, the loss and every gradient are bitwise equal,
    except the weight gradients named by _vendor_weight_gradients (two at out_stride 8, three at 16), which may differ."""
    from mscs_amd import _lib_dconv as ld
    from mscs_amd.utils import set_verbosity
    set_verbosity(40)
    torch.manual_seed(0)
    before = dict(ld.calls)
    one, state, model = _step(dev, out_stride, None)
    # three ASPP branches, two blocks of layer4 (its first keeps dilation 1) and at out_stride 8 five more of layer3 + layer4's first
    dilated = 3 + 2 + (6 if out_stride == 8 else 0)
    assert {k: ld.calls[k] - before[k] for k in before} == {"fwd": dilated, "dgrad": dilated, "wgrad": dilated}
    assert list(one["logits"].shape) == [2, 19, 65, 97]
    params = dict(model.named_parameters())
    assert all("g:" + n in one for n in params), [n for n in params if "g:" + n not in one][:5]
    for k, v in one.items():
        assert bool(torch.isfinite(v).all()), (k, "not finite")
        if k.startswith("g:"):
            assert v.shape == params[k[2:]].shape
    two, _, _ = _step(dev, out_stride, state)
    excepted = _vendor_weight_gradients(model, (65, 97))
    assert set(excepted) <= set(params) and len(excepted) == (3 if out_stride == 16 else 2), excepted
    differ = [k for k in one if not torch.equal(one[k], two[k])]
    print(f"out_stride {out_stride}: {len(one)} tensors, {len(differ)} differ between two runs: {differ}; excepted: {excepted}")
    assert not [k for k in differ if k[2:] not in excepted], differ[:8]
