"""The test-time-augmentation kernels (include/dcl_tta.h, models/ops_tta.py, models/TTA.py) on the GPU.

Every entry is held against a float64 evaluation of the same composition on the CPU with the bound
    e_kernel <= max(4 * e_eager, 16 * eps32 * max|ref|)
where e_eager is the error of the fp32 torch composition on the GPU against the same float64 result (the kernel may be no worse
than four times the existing path) and the floor is 16 roundings: two levels of three lerps plus the formation of the weights.  For
the exp entry the bound is relative (errors divided by |ref|, floor 16 * eps32); logits stay within +-8, far from overflow.  The
G17 fixtures go through the fused wrappers at the same bound against a float64 run of the composition."""
import contextlib

import numpy as np
import pytest
import torch

import _tta_golden as tg

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)

MERGE = [(5, 6, 9, 22, 33, 30, 44), (1, 4, 5, 16, 18, 8, 9), (19, 8, 11, 30, 44, 30, 44), (150, 3, 3, 9, 9, 7, 5),
         (5, 22, 33, 22, 33, 30, 44)]                   # (C, h, w, Hm, Wm, H, W); the last: identity inner level
ALIGN = [(0, 0), (1, 1), (0, 1), (1, 0)]                # (inner, outer)

# fixture B's geometry (tools/gen_golden_tta.py): K = 5, image 20 x 40, base 48, crop (16, 24), strides (11, 16)
#   (canvas, crop, [(h0, w0, wh, ww), ...], flip)
WINDOWS = {
    "s0.5_whole": ((12, 24), (12, 24), [(0, 0, 12, 24)], True),
    "s1.0_2x3": ((24, 48), (16, 24), [(h0, w0, 16, 24) for h0 in (0, 8) for w0 in (0, 16, 24)], True),
    "s1.5_3x4": ((36, 72), (16, 24), [(h0, w0, 16, 24) for h0 in (0, 11, 20) for w0 in (0, 16, 32, 48)], True),
    "c_noflip_short": ((24, 48), (24, 24), [(0, 0, 24, 24), (0, 24, 24, 24)], False),       # fixture C: the window is lower than the crop
    "partial": ((24, 48), (16, 24), [(3, 5, 13, 22), (8, 24, 16, 21)], True),               # wh < ch, ww < cw, odd offsets: the scalar tail
}
K = 5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_tta
    from mscs_amd.utils import set_verbosity
    _lib_tta.lib()
    set_verbosity(40)
    return torch.device("cuda:0")


@contextlib.contextmanager
def _switch(dbg, value):
    """debug.cfg.tta_hip for the duration: the fused path (True) or the composition (False) of the wrappers"""
    old, dbg.tta_hip = dbg.tta_hip, value
    try:
        yield
    finally:
        dbg.tta_hip = old


def _logits(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * 3).clamp_(-8, 8).float()


def _bound(got, eager, ref, relative=False, what=""):
    """got / eager: fp32 results of the kernel and of the torch composition; ref: float64"""
    got, eager, ref = got.detach().double().cpu(), eager.detach().double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    scale = ref.abs() if relative else torch.ones(())
    e_kernel = float(((got - ref).abs() / scale).max())
    e_eager = float(((eager - ref).abs() / scale).max())
    floor = 16 * EPS * (1.0 if relative else float(ref.abs().max()))
    print(f"{what}: e_kernel {e_kernel:.3e} e_eager {e_eager:.3e} floor {floor:.3e}")
    assert e_kernel <= max(4 * e_eager, floor), (what, e_kernel, e_eager, floor)


def check_merge(dev, shape, flip, align, ops):
    C, h, w, Hm, Wm, H, W = shape
    z = _logits((C, h, w), sum(shape) + flip)
    base = _logits((C, H, W), 7)
    ref = ops.merge_eager(z.double(), (Hm, Wm), align[0], flip, base.double().clone(), align[1], 0.5)
    eager = ops.merge_eager(z.to(dev), (Hm, Wm), align[0], flip, base.to(dev).clone(), align[1], 0.5)
    got = ops.merge(z.to(dev), (Hm, Wm), align[0], flip, base.to(dev).clone(), align[1], 0.5)
    _bound(got, eager, ref, what=f"merge {shape} flip {flip} align {align}")


def _windows(fn, conv, name, align, zs):
    (Hc, Wc), crop, wins, _ = WINDOWS[name]
    canvas = conv(torch.zeros(K, Hc, Wc))
    for (z, zf), win in zip(zs, wins):
        fn(conv(z), None if zf is None else conv(zf), crop, align, canvas, *win)
    return canvas


def check_windows(dev, name, align, ops):
    _, (ch, cw), wins, flip = WINDOWS[name]
    h, w = -(-ch // 4), -(-cw // 4)
    zs = [(_logits((K, h, w), 100 + i), _logits((K, h, w), 200 + i) if flip else None) for i in range(len(wins))]
    ref = _windows(ops.window_accum_eager, lambda t: t.double(), name, align, zs)
    eager = _windows(ops.window_accum_eager, lambda t: t.to(dev), name, align, zs)
    got = _windows(ops.window_accum, lambda t: t.to(dev), name, align, zs)
    touched = ref != 0
    assert bool((got.cpu()[~touched] == 0).all()), "written outside the windows"
    one = torch.ones((), dtype=torch.float64)           # outside the windows all three hold 0: compared as 1 == 1
    _bound(torch.where(touched, got.cpu().double(), one), torch.where(touched, eager.cpu().double(), one), torch.where(touched, ref, one),
           relative=True, what=f"window_accum {name} align {align}")


def check_canvas(dev, name, align, ops):
    (Hc, Wc), (ch, cw), wins, _ = WINDOWS[name]
    H, W = 20, 40
    g = torch.Generator().manual_seed(Hc)
    canvas = torch.rand(K, Hc, Wc, generator=g) * 20 + 0.01
    rowcnt = ops.counts_1d(Hc, sorted({(h0, h0 + wh) for h0, _, wh, _ in wins}))
    colcnt = ops.counts_1d(Wc, sorted({(w0, w0 + ww) for _, w0, _, ww in wins}))
    assert int(rowcnt.min()) >= 1 and int(colcnt.min()) >= 1
    base = _logits((K, H, W), 9)
    ref = ops.canvas_merge_eager(canvas.double(), rowcnt, colcnt, base.double().clone(), align)
    eager = ops.canvas_merge_eager(canvas.to(dev), rowcnt.to(dev), colcnt.to(dev), base.to(dev).clone(), align)
    got = ops.canvas_merge(canvas.to(dev), rowcnt.to(dev), colcnt.to(dev), base.to(dev).clone(), align)
    _bound(got, eager, ref, what=f"canvas_merge {name} align {align}")


@pytest.mark.parametrize("align", ALIGN, ids=lambda a: f"align{a[0]}{a[1]}")
@pytest.mark.parametrize("flip", (0, 1))
@pytest.mark.parametrize("shape", MERGE, ids=lambda s: "x".join(str(v) for v in s))
def test_merge_against_float64(dev, shape, flip, align):
    from mscs_amd.models import ops_tta
    check_merge(dev, shape, flip, align, ops_tta)


@pytest.mark.parametrize("align", (0, 1))
@pytest.mark.parametrize("name", list(WINDOWS))
def test_window_accum_against_float64(dev, name, align):
    from mscs_amd.models import ops_tta
    check_windows(dev, name, align, ops_tta)


@pytest.mark.parametrize("align", (0, 1))
@pytest.mark.parametrize("name", ["s0.5_whole", "s1.0_2x3", "s1.5_3x4", "c_noflip_short"])
def test_canvas_merge_against_float64(dev, name, align):
    from mscs_amd.models import ops_tta
    check_canvas(dev, name, align, ops_tta)


def check_fixture(dev, case, lazy, dbg, calls):
    """the fused wrapper on ``dev`` against the composition in float64 on the CPU and in fp32 on ``dev``"""
    g = tg.load(case)
    x = torch.from_numpy(g["x"])
    with torch.no_grad():
        ref = tg.wrapper(g, tg.toy(g, dtype=torch.float64))(x.double())
        before = dict(calls)
        with _switch(dbg, True):
            got = tg.wrapper(g, tg.toy(g, dev, lazy=lazy))(x.to(dev))
        used = {k: calls[k] - before[k] for k in calls}
        before = dict(calls)
        with _switch(dbg, False):
            eager = tg.wrapper(g, tg.toy(g, dev, lazy=lazy))(x.to(dev))
        assert calls == before, "the composition path called the kernels"
    if g["config"]["wrapper"] == "plain":
        assert used["merge"] == 2 * len(g["config"]["scales_after"]) and used["window_accum"] == 0, used
    else:
        assert used["canvas_merge"] == len(g["config"]["scales_after"]) and used["window_accum"] > 0 and used["merge"] == 0, used
    _bound(got, eager, ref, what=f"fixture {case} lazy {lazy}")
    # and the reference's own numbers: the float64 composition reproduces the fixture to fp32 round-off
    np.testing.assert_allclose(ref.float().numpy(), g["out"], rtol=1e-4, atol=1e-5 * float(np.abs(g["out"]).max()))


@pytest.mark.parametrize("lazy", (False, True), ids=("full", "lazy"))
@pytest.mark.parametrize("case", tg.CASES)
def test_fixtures_through_the_fused_wrappers(dev, case, lazy):
    from mscs_amd import _lib_tta as lt
    from mscs_amd.debug import cfg as dbg
    check_fixture(dev, case, lazy, dbg, lt.calls)


def test_accumulators_are_added_to_and_runs_are_bitwise_equal(dev):
    from mscs_amd.models import ops_tta
    C, h, w, Hm, Wm, H, W = 19, 8, 11, 30, 44, 30, 44
    z = _logits((C, h, w), 1).to(dev)
    pattern = (torch.arange(C * H * W, dtype=torch.float32).reshape(C, H, W) % 251 - 125).to(dev)
    zero = ops_tta.merge(z, (Hm, Wm), 0, 1, torch.zeros_like(pattern), 1)
    a = ops_tta.merge(z, (Hm, Wm), 0, 1, pattern.clone(), 1)
    b = ops_tta.merge(z, (Hm, Wm), 0, 1, pattern.clone(), 1)
    assert torch.equal(a, b)
    assert torch.equal(a, pattern + zero)           # one rounding of pattern + value, the value that of a zero accumulator
    (Hc, Wc), crop, wins, _ = WINDOWS["partial"]
    zc, zf = _logits((K, 4, 6), 2).to(dev), _logits((K, 4, 6), 3).to(dev)
    pat = (torch.arange(K * Hc * Wc, dtype=torch.float32).reshape(K, Hc, Wc) % 251 - 125).to(dev)
    outs = []
    for start in (torch.zeros_like(pat), pat, pat):
        canvas = start.clone()
        for win in wins:
            ops_tta.window_accum(zc, zf, crop, 1, canvas, *win)
        outs.append(canvas)
    assert torch.equal(outs[1], outs[2]) and bool((outs[0] != 0).any()) and bool((outs[0] == 0).any())
    assert torch.equal(outs[1][outs[0] == 0], pat[outs[0] == 0])       # only the window region changes
    once = outs[0] != 0
    once[:, 8:16, 24:27] = False                                        # the two windows overlap there: two additions
    assert torch.equal(outs[1][once], (pat + outs[0])[once])
    rowcnt = torch.ones(Hc, dtype=torch.int32, device=dev)
    colcnt = torch.full((Wc,), 2, dtype=torch.int32, device=dev)
    small = pattern[:K, :20, :40].contiguous()
    acc0 = ops_tta.canvas_merge(pat.abs() + 1, rowcnt, colcnt, torch.zeros_like(small), 0)
    acc1 = ops_tta.canvas_merge(pat.abs() + 1, rowcnt, colcnt, small.clone(), 0)
    acc2 = ops_tta.canvas_merge(pat.abs() + 1, rowcnt, colcnt, small.clone(), 0)
    assert torch.equal(acc1, acc2) and torch.equal(acc1, small + acc0)


def test_wrapper_runs_are_bitwise_equal(dev):
    g = tg.load("b_ac1")
    x = torch.from_numpy(g["x"]).to(dev)
    w = tg.wrapper(g, tg.toy(g, dev, lazy=True))
    with torch.no_grad():
        assert torch.equal(w(x), w(x))


def test_unsupported_shapes_are_refused_before_a_launch(dev):
    from mscs_amd import _lib_tta as lt
    L = lt.lib()
    z = torch.zeros(4, 4, 4, device=dev)
    acc = torch.zeros(4, 8, 8, device=dev)
    st = lt.stream_ptr(dev)
    assert L.dtt_merge(z.data_ptr(), 0, 4, 4, 8, 8, 0, 0, acc.data_ptr(), 8, 8, 0, 1.0, st) != 0
    assert b"dtt_supported" in L.dtt_last_error()
    assert L.dtt_merge(z.data_ptr(), 1025, 4, 4, 8, 8, 0, 0, acc.data_ptr(), 8, 8, 0, 1.0, st) != 0
    assert L.dtt_window_accum(z.data_ptr(), None, 4, 4, 4, 8, 8, 0, acc.data_ptr(), 8, 8, 1, 0, 8, 8, st) != 0       # below the canvas
    assert b"outside" in L.dtt_last_error()
    assert L.dtt_window_accum(z.data_ptr(), None, 4, 4, 4, 6, 6, 0, acc.data_ptr(), 8, 8, 0, 0, 7, 6, st) != 0       # larger than the crop
    assert L.dtt_canvas_merge(acc.data_ptr(), None, None, 4, 8, 8, acc.data_ptr(), 8, 8, 0, st) != 0
    torch.cuda.synchronize()
    assert float(acc.abs().max()) == 0.0


def test_hrnet_fused_and_composition_agree(dev):
    """HRNet (hrnet18) at 64 x 128, scales [0.5] (+ the appended 1.0): the fused path reads the quarter-resolution logits, the
    composition the model's up-sampled ones.  Both evaluate the same two-level bilinear map of the same logits in fp32 with at most
    16 roundings per view each (two levels of three lerps plus the weights), so the plain wrapper's two paths agree within
    32 * eps32 * max|logits| (the mean over the views does not grow it).  The Cityscapes wrapper takes exp, which turns that
    absolute error of the averaged logits into a relative one, and adds at most 16 relative roundings per path (expf, the division
    by the count, the three lerps and the weights of the final resize): 32 * eps32 * max|logits| + 32 * eps32, relative."""
    from mscs_amd import _lib_tta as lt
    from mscs_amd.debug import cfg as dbg
    from mscs_amd.models import HRNet, TTAWrapper, TTAWrapperCTS
    from mscs_amd.models.ops_logits import UpsampledLogits
    torch.manual_seed(0)
    graph = {"dataset": "CITYSCAPES", "backbone": "hrnet18", "pretrained": False, "align_corners": True}
    model = HRNet(config=graph, experiment=1).to(dev).eval()
    x = torch.randn(1, 3, 64, 128, generator=torch.Generator().manual_seed(5)).to(dev)
    seen = []
    model.register_forward_hook(lambda m, i, o: seen.append(float((o.lowres if hasattr(o, "lowres") else o).abs().max())))
    with torch.no_grad():
        before = lt.calls["merge"]
        with _switch(dbg, True):
            fused = TTAWrapper(model, [0.5])(x)
        assert lt.calls["merge"] == before + 4 and model.lazy_eval_logits is False
        model.lazy_eval_logits = True
        assert isinstance(model(x), UpsampledLogits)
        model.lazy_eval_logits = False
        with _switch(dbg, False):
            comp = TTAWrapper(model, [0.5])(x)
        assert lt.calls["merge"] == before + 4
        err, zmax = float((fused - comp).abs().max()), max(seen)
        print(f"hrnet18 TTAWrapper: |fused - composition| {err:.3e}, max|logits| {zmax:.3e}")
        assert fused.shape == (1, 19, 64, 128) and err <= 32 * EPS * zmax
        # the Cityscapes wrapper on the same model: whole image at 0.5, 1 x 2 windows of 64 x 64 at 1.0
        cts = lambda: TTAWrapperCTS(model, [0.5], True, None, [64, 64], base_size=128)
        del seen[:]
        before = lt.calls["window_accum"]
        with _switch(dbg, True):
            fused = cts()(x)
        assert lt.calls["window_accum"] == before + 3
        with _switch(dbg, False):
            comp = cts()(x)
        rel, zmax = float(((fused - comp).abs() / comp.abs()).max()), max(seen)
        print(f"hrnet18 TTAWrapperCTS: relative |fused - composition| {rel:.3e}, max|logits| {zmax:.3e}")
        assert fused.shape == (1, 19, 64, 128) and rel <= 32 * EPS * zmax + 32 * EPS
