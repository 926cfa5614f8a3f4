"""The sliding-window kernels with equal-size windows (include/dcl_slide.h, models/ops_slide.py, TTAWrapperPC / TTAWrapperSlide of
models/TTA.py) on the GPU.

Every entry is held against a float64 evaluation of the same composition on the CPU with the bound of tests/test_tta_hip.py
    e_kernel <= max(4 * e_eager, 16 * eps32 * max|ref|)
where e_eager is the error of the fp32 torch composition on the GPU against the same float64 result.  For the exp entry the bound
is relative (errors divided by |ref|, floor 16 * eps32); logits stay within +-8, far from overflow.  The G19 fixtures go through
the fused wrappers at the same bound against a float64 run of the composition.  With DCL_SLIDE_ACCURACY_JSON set, the errors seen
are written there (profiles/slide_accuracy.json is such a file)."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

import _slide_cases as sc
import _tta_golden as tg

pytestmark = pytest.mark.gpu

EPS = sc.EPS
K = 5
RECORD = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_slide, _lib_tta
    from mscs_amd.utils import set_verbosity
    _lib_slide.lib()
    _lib_tta.lib()
    set_verbosity(40)
    yield torch.device("cuda:0")
    path = os.environ.get("DCL_SLIDE_ACCURACY_JSON")
    if path:
        with open(path, "w") as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)


@contextlib.contextmanager
def _switch(dbg, value):
    """debug.cfg.slide_hip for the duration: the fused path (True) or the composition (False) of the wrappers"""
    old, dbg.slide_hip = dbg.slide_hip, value
    try:
        yield
    finally:
        dbg.slide_hip = old


# ---- dsw_crops -----------------------------------------------------------------------------------------------------------------------
#   grid of sc.GRIDS, image (H, W) it is cut from
CROPS = [("pa_1.5", (22, 30)), ("pb_0.5", (30, 22)), ("sa_0.5", (20, 40)), ("sa_1.5", (20, 40)), ("odd", (17, 29))]


@pytest.mark.parametrize("mirror", (1, 0), ids=("mirror", "plain"))
@pytest.mark.parametrize("name,image", CROPS, ids=[c[0] for c in CROPS])
def test_crops_against_float64(dev, name, image, mirror):
    from mscs_amd.models import ops_slide
    size, win, rows_lo, cols_lo = sc.GRIDS[name]
    x = torch.randn((3,) + image, generator=torch.Generator().manual_seed(sum(size)))
    args = (size, rows_lo, cols_lo, win, sc.PAD, mirror)
    ref = ops_slide.crops_eager(x.double(), *args)
    eager = ops_slide.crops_eager(x.to(dev), *args)
    got = ops_slide.crops(x.to(dev), *args)
    N = len(rows_lo) * len(cols_lo)
    assert got.shape == (N * (1 + mirror), 3, win[0], win[1])
    sc.bound(got, eager, ref, what=f"crops {name} mirror {mirror}", record=RECORD)
    # every padded element is exactly pad[c]
    padded = torch.zeros((N, 1) + tuple(win), dtype=torch.bool)
    for r, lo_r in enumerate(rows_lo):
        for q, lo_q in enumerate(cols_lo):
            padded[r * len(cols_lo) + q, 0, max(size[0] - lo_r, 0):, :] = True
            padded[r * len(cols_lo) + q, 0, :, max(size[1] - lo_q, 0):] = True
    if name.startswith("p"):
        assert bool(padded.any()), "the case was meant to hold padding"
    pad32 = torch.tensor(sc.PAD, dtype=torch.float32).view(1, 3, 1, 1).expand(N, 3, *win)
    plain = got[:N].cpu()
    assert torch.equal(plain[padded.expand_as(plain)], pad32[padded.expand_as(plain)])
    if mirror:
        assert torch.equal(got[N:], torch.flip(got[:N], dims=[3])), "the mirrored block is not the mirror of the plain block"
    assert torch.equal(got, ops_slide.crops(x.to(dev), *args)), "two runs differ"


# ---- dsw_gather ----------------------------------------------------------------------------------------------------------------------
#   name: (grid of sc.GRIDS or a literal one, classes)
GATHER = {
    "pa_1.0": (sc.GRIDS["pa_1.0"], K),
    "pa_1.5": (sc.GRIDS["pa_1.5"], K),
    "sa_1.5": (sc.GRIDS["sa_1.5"], K),
    "single_short": (((11, 21), (16, 24), [0], [0]), K),                      # one window, Hc < wh and Wc < ww: clipped
    "c150": (((13, 18), (8, 12), [0, 5], [0, 6]), 150),                       # classes split over grid y
    "odd": (sc.GRIDS["odd"], 19),                                             # Wc % 4 != 0: the scalar tail; a chunk of 19 classes
}


def _gather_inputs(name, flip):
    (size, win, rows_lo, cols_lo), C = GATHER[name]
    N = len(rows_lo) * len(cols_lo)
    h, w = -(-win[0] // 4), -(-win[1] // 4)
    z = sc.logits((N, C, h, w), 100 + N)
    zf = sc.logits((N, C, h, w), 200 + N) if flip else None
    return size, win, rows_lo, cols_lo, C, z, zf


@pytest.mark.parametrize("align", (0, 1))
@pytest.mark.parametrize("flip", (1, 0), ids=("zf", "nozf"))
@pytest.mark.parametrize("name", list(GATHER))
def test_gather_against_float64(dev, name, flip, align):
    from mscs_amd.models import ops_slide
    size, win, rows_lo, cols_lo, C, z, zf = _gather_inputs(name, flip)
    conv = {"ref": lambda t: None if t is None else t.double(), "dev": lambda t: None if t is None else t.to(dev)}
    ref = ops_slide.gather_eager(conv["ref"](z), conv["ref"](zf), win, align, rows_lo, cols_lo, torch.zeros((C,) + size, dtype=torch.float64))
    eager = ops_slide.gather_eager(conv["dev"](z), conv["dev"](zf), win, align, rows_lo, cols_lo, torch.zeros((C,) + size, device=dev))
    # a canvas pre-filled with NaN comes back finite: it is stored, not added to
    canvas = torch.full((C,) + size, float("nan"), device=dev)
    got = ops_slide.gather(conv["dev"](z), conv["dev"](zf), win, align, rows_lo, cols_lo, canvas)
    assert got.data_ptr() == canvas.data_ptr() and bool(torch.isfinite(canvas).all())
    sc.bound(got, eager, ref, relative=True, what=f"gather {name} zf {flip} align {align}", record=RECORD)
    again = ops_slide.gather(conv["dev"](z), conv["dev"](zf), win, align, rows_lo, cols_lo, torch.zeros((C,) + size, device=dev))
    assert torch.equal(got, again), "two runs differ, or the result depends on what the canvas held"


def test_gather_with_full_resolution_logits(dev):
    """a model without lazy_eval_logits: h == wh, the inner level is the identity"""
    from mscs_amd.models import ops_slide
    size, win, rows_lo, cols_lo = sc.GRIDS["pa_1.0"]
    N = len(rows_lo) * len(cols_lo)
    z, zf = sc.logits((N, K) + win, 7), sc.logits((N, K) + win, 8)
    ref = ops_slide.gather_eager(z.double(), zf.double(), win, 1, rows_lo, cols_lo, torch.zeros((K,) + size, dtype=torch.float64))
    eager = ops_slide.gather_eager(z.to(dev), zf.to(dev), win, 1, rows_lo, cols_lo, torch.zeros((K,) + size, device=dev))
    got = ops_slide.gather(z.to(dev), zf.to(dev), win, 1, rows_lo, cols_lo, torch.empty((K,) + size, device=dev))
    sc.bound(got, eager, ref, relative=True, what="gather pa_1.0 full-resolution logits", record=RECORD)


# ---- the wrappers --------------------------------------------------------------------------------------------------------------------
def _fixture_reference(g):
    """the float64 composition on the CPU, once per fixture"""
    key = g["config_json"].item()
    if key not in _fixture_reference.cache:
        with torch.no_grad():
            _fixture_reference.cache[key] = sc.wrapper(g, tg.toy(g, dtype=torch.float64))(torch.from_numpy(g["x"]).double())
    return _fixture_reference.cache[key]


_fixture_reference.cache = {}


@pytest.mark.parametrize("lazy", (False, True), ids=("full", "lazy"))
@pytest.mark.parametrize("case", sc.CASES)
def test_fixtures_through_the_fused_wrappers(dev, case, lazy):
    from mscs_amd import _lib_slide as ls
    from mscs_amd import _lib_tta as lt
    from mscs_amd.debug import cfg as dbg
    g = sc.load(case)
    x = torch.from_numpy(g["x"])
    ref = _fixture_reference(g)
    with torch.no_grad():
        before, merges = dict(ls.calls), lt.calls["merge"]
        with _switch(dbg, True):
            got = sc.wrapper(g, tg.toy(g, dev, lazy=lazy))(x.to(dev))
        used = {k: ls.calls[k] - before[k] for k in ls.calls}
        assert used == {"crops": sc.views(g), "gather": sc.views(g)} and lt.calls["merge"] - merges == sc.views(g), used
        before = dict(ls.calls)
        with _switch(dbg, False):
            eager = sc.wrapper(g, tg.toy(g, dev, lazy=lazy))(x.to(dev))
        assert ls.calls == before, "the composition path called the kernels"
        sc.bound(got, eager, ref, what=f"fixture {case} lazy {lazy}", record=RECORD)
        # tta_window_batch only changes how the windows are batched through the model
        for wb in (1, 3, 64):
            with _switch(dbg, True):
                other = sc.wrapper(g, tg.toy(g, dev, lazy=lazy), window_batch=wb)(x.to(dev))
            sc.bound(other, eager, ref, what=f"fixture {case} lazy {lazy} tta_window_batch {wb}")
    # and the reference's own numbers: the float64 composition reproduces the fixture to fp32 round-off
    np.testing.assert_allclose(ref.float().numpy(), g["out"], rtol=1e-4, atol=1e-5 * float(np.abs(g["out"]).max()))


@pytest.mark.parametrize("case", ("pa_ac1", "sa_ac0"))
def test_wrapper_runs_are_bitwise_equal(dev, case):
    g = sc.load(case)
    x = torch.from_numpy(g["x"]).to(dev)
    w = sc.wrapper(g, tg.toy(g, dev, lazy=True))
    with torch.no_grad():
        assert torch.equal(w(x), w(x))


def test_refused_shapes_return_before_a_launch(dev):
    from mscs_amd import _lib_slide as ls
    L = ls.lib()
    st = ls.stream_ptr(dev)
    z = torch.zeros(1, 4, 4, 6, device=dev)
    canvas = torch.full((4, 16, 24), 3.0, device=dev)
    out = torch.full((2, 3, 16, 24), 3.0, device=dev)
    x = torch.zeros(3, 8, 8, device=dev)
    lo0, lo65 = ls.ints([0]), ls.ints(range(65))
    assert L.dsw_gather(z.data_ptr(), None, 1025, 4, 6, 16, 24, 0, lo0, 1, lo0, 1, canvas.data_ptr(), 16, 24, st) != 0
    assert b"dsw_supported" in L.dsw_last_error()
    assert L.dsw_gather(z.data_ptr(), None, 4, 4, 6, 16, 24, 0, lo65, 65, lo0, 1, canvas.data_ptr(), 16, 24, st) != 0
    assert b"DSW_MAX_WIN" in L.dsw_last_error()
    assert L.dsw_gather(z.data_ptr(), None, 4, 4, 6, 12, 24, 0, lo0, 1, lo0, 1, canvas.data_ptr(), 16, 24, st) != 0      # rows 12 .. 15 uncovered
    assert b"under no" in L.dsw_last_error()
    assert L.dsw_gather(z.data_ptr(), None, 4, 4, 6, 16, 24, 0, ls.ints([16]), 1, lo0, 1, canvas.data_ptr(), 16, 24, st) != 0
    assert b"outside" in L.dsw_last_error()
    assert L.dsw_gather(None, None, 4, 4, 6, 16, 24, 0, lo0, 1, lo0, 1, canvas.data_ptr(), 16, 24, st) != 0
    assert L.dsw_crops(x.data_ptr(), 9, 8, 8, 16, 24, lo0, 1, lo0, 1, 16, 24, ls.floats([0] * 9), 1, out.data_ptr(), st) != 0
    assert L.dsw_crops(x.data_ptr(), 3, 8, 8, 16, 24, lo0, 1, lo65, 65, 16, 24, ls.floats([0] * 3), 1, out.data_ptr(), st) != 0
    assert L.dsw_crops(x.data_ptr(), 3, 8, 8, 16, 24, ls.ints([-1]), 1, lo0, 1, 16, 24, ls.floats([0] * 3), 1, out.data_ptr(), st) != 0
    assert b"below 0" in L.dsw_last_error()
    torch.cuda.synchronize()
    assert bool((canvas == 3.0).all()) and bool((out == 3.0).all())
    with pytest.raises(RuntimeError, match="under no"):
        from mscs_amd.models import ops_slide
        ops_slide.gather(z, None, (12, 24), 0, [0], [0], canvas)


def test_hrnet_fused_and_composition_agree(dev):
    """HRNet (hrnet18), TTAWrapperPC, image 96 x 128, crop (64, 64), base 128, scales [0.5] (+ the appended 1.0): the fused path
    reads the quarter-resolution logits of a window batch, the composition the model's up-sampled ones window by window.  The bar is
    that of tests/test_tta_hip.py::test_hrnet_fused_and_composition_agree for the Cityscapes wrapper: both evaluate the same bilinear
    map of the same logits in fp32 with at most 16 roundings each, exp turns that absolute error of the averaged logits into a
    relative one and adds at most 16 relative roundings per path: 32 * eps32 * max|logits| + 32 * eps32, relative."""
    from mscs_amd import _lib_slide as ls
    from mscs_amd.debug import cfg as dbg
    from mscs_amd.models import HRNet, TTAWrapperPC
    torch.manual_seed(0)
    graph = {"dataset": "PASCALC", "backbone": "hrnet18", "pretrained": False, "align_corners": True}
    model = HRNet(config=graph, experiment=1).to(dev).eval()
    x = torch.randn(1, 3, 96, 128, generator=torch.Generator().manual_seed(5)).to(dev)
    seen = []
    model.register_forward_hook(lambda m, i, o: seen.append(float((o.lowres if hasattr(o, "lowres") else o).abs().max())))
    pc = lambda: TTAWrapperPC(model, [0.5], num_classes=model.num_classes, crop_size=(64, 64), base_size=128)
    with torch.no_grad():
        before = dict(ls.calls)
        with _switch(dbg, True):
            fused = pc()(x)
        assert {k: ls.calls[k] - before[k] for k in before} == {"crops": 2, "gather": 2} and model.lazy_eval_logits is False
        with _switch(dbg, False):
            comp = pc()(x)
        rel, zmax = float(((fused - comp).abs() / comp.abs()).max()), max(seen)
        print(f"hrnet18 TTAWrapperPC: relative |fused - composition| {rel:.3e}, max|logits| {zmax:.3e}")
        RECORD["hrnet18 TTAWrapperPC fused vs composition"] = {"relative": rel, "max_logits": zmax, "bar": 32 * EPS * zmax + 32 * EPS}
        assert fused.shape == (1, model.num_classes, 96, 128) and rel <= 32 * EPS * zmax + 32 * EPS
