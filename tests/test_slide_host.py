"""Host half of the sliding-window test-time augmentation with equal-size windows (include/dcl_slide.h, models/ops_slide.py,
TTAWrapperPC / TTAWrapperSlide of models/TTA.py): the eleventh library is built next to the main one, exports and binds exactly what
its header declares; the plan in C agrees with the plan in Python and with the reference's loops restated; every pixel of the
fixture geometries is under a window; too many windows and empty grids are refused with a message; the wrappers reproduce the
reference's outputs on the CPU (fixtures G19), restore the model's attributes when a call raises, and the manager dispatches to
them."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import mscs_amd  # noqa: F401
from mscs_amd import _lib
from mscs_amd.models import TTAWrapper, TTAWrapperCTS, TTAWrapperPC, TTAWrapperSlide      # (the feature: this import fails without it)
from mscs_amd.utils import set_verbosity

import _slide_cases as sc
import _tta_golden as tg

ENTRIES = {"dsw_version", "dsw_last_error", "dsw_supported", "dsw_crops", "dsw_gather", "dsw_plan_pc_windows", "dsw_plan_cover"}


def _header():
    return open(os.path.join(ROOT, "include", "dcl_slide.h")).read()


def test_eleventh_library_is_built_by_the_same_target():
    from mscs_amd import _lib_slide as ls
    _lib.build()
    assert os.path.exists(ls.LIB_PATH) and os.path.basename(ls.LIB_PATH) == "libdcl_slide.so"
    assert os.path.dirname(ls.LIB_PATH) == os.path.dirname(_lib.LIB_PATH)
    mk = open(os.path.join(_lib.CSRC_DIR, "Makefile")).read()
    assert "SW.slide" in re.search(r"^SATELLITES = (.*)$", mk, re.M).group(1)
    assert "dcl_slide" not in re.search(r"^PACKED = (.*)$", mk, re.M).group(1)         # the generic rule: built with NOPK
    assert "dsw_" not in open(os.path.join(ROOT, "include", "dcl_tta.h")).read()


def test_header_exports_and_bindings_agree():
    from mscs_amd import _lib_slide as ls
    _lib.build()
    hdr = _header()
    names = sorted(set(re.findall(r"\b(dsw_[a-z0-9_]+)\s*\(", hdr)))
    assert set(names) == ENTRIES
    assert not re.findall(r"\b(dcl|dat|dco|ddc|dtt)_[a-z0-9_]+\s*\(", hdr), "another library's prefix in this library's header"
    raw = ctypes.CDLL(ls.LIB_PATH)
    for name in names:
        assert hasattr(raw, name), f"{name} declared in include/dcl_slide.h but not exported"
    assert set(ls.SIGNATURES) | {"dsw_last_error"} == set(names)
    assert not any(n.startswith("dsw_") for n in _lib.SIGNATURES)
    L = ls.lib()
    assert L.dsw_version() >= 1
    for name, sig in ls.SIGNATURES.items():
        decl = re.search(rf"\b{name}\s*\(([^;]*)\);", hdr).group(1).strip()
        assert len(sig) == (0 if decl == "void" else decl.count(",") + 1), name
    for macro, value in (("DSW_MAX_C", ls.MAX_C), ("DSW_MAX_CIN", ls.MAX_CIN), ("DSW_MAX_WIN", ls.MAX_WIN), ("DSW_RUN", ls.RUN)):
        assert int(re.search(rf"#define {macro} (\d+)", hdr).group(1)) == value
    from mscs_amd.models import ops_slide
    assert ops_slide.MAX_WIN == ls.MAX_WIN == 64


def test_switch_is_registered():
    from mscs_amd.debug import DebugConfig, cfg as dbg
    assert "slide_hip" in DebugConfig.__dataclass_fields__ and isinstance(dbg.slide_hip, bool)


def test_supported_is_host_arithmetic():
    from mscs_amd import _lib_slide as ls
    assert ls.supported(3, 375, 500, 59, 128, 128, 512, 512, 3, 3, 750, 1000)          # PASCAL-Context at 2.0
    assert ls.supported(3, 512, 683, 150, 128, 128, 512, 512, 9, 3, 3072, 768)         # ADE20K slide at 1.5
    good = [3, 20, 40, 5, 4, 6, 16, 24, 2, 3, 24, 48]
    assert ls.supported(*good)
    for i in range(12):
        for bad in (0, -3):
            args = list(good)
            args[i] = bad
            assert not ls.supported(*args), args
    for i, v in ((0, 9), (3, 1025), (8, 65), (9, 65), (4, 17), (5, 25)):              # Cin, C, R, Q, h > wh, w > ww
        args = list(good)
        args[i] = v
        assert not ls.supported(*args), args
    assert ls.supported(1, 1, 1, 1, 1, 1, 1, 1, 1, 1, (1 << 16) - 1, 1 << 15) and not ls.supported(1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1 << 16, 1 << 15)


# ---- the plan ----------------------------------------------------------------------------------------------------------------------
def _reference_pc_windows(n, crop, stride):
    """the reference's window loop along one padded axis (models/TTA_wrapper_PC.py forward), restated"""
    rows = int(np.ceil(1.0 * (n - crop) / stride)) + 1
    return rows, [(r * stride, min(r * stride + crop, n)) for r in range(rows)]


def test_pc_plan_in_c_equals_the_plan_in_python():
    from mscs_amd import _lib_slide as ls
    from mscs_amd.models import ops_slide
    kinds = set()
    for n in (1, 7, 16, 23, 24, 29, 36, 44, 48, 60, 75):
        for crop in (1, 16, 24, 32):
            for stride in (1, 10, 11, 16, 24, 40):
                rows, want = _reference_pc_windows(n, crop, stride)
                count, spans = ls.plan_pc_windows(n, crop, stride)
                mine = ops_slide.pc_windows_1d(n, crop, stride)
                assert count == rows, (n, crop, stride)
                if rows < 1:
                    kinds.add("degenerate")
                    assert spans == [] and mine == []
                    continue
                assert spans == want and mine == want, (n, crop, stride)
                kinds.add("partial" if want[-1][1] - want[-1][0] < crop else "exact")
                if want[-1][0] < n and len(want) <= ls.MAX_WIN:
                    least, cnt = ls.plan_cover(n, crop, [lo for lo, _ in want])
                    assert cnt == ops_slide.cover_1d(n, crop, [lo for lo, _ in want]) and least == min(cnt)
                    assert least >= 1 or stride > crop
    assert kinds == {"degenerate", "partial", "exact"}
    assert ops_slide.pc_strides((512, 512)) == (341, 341) and ops_slide.pc_strides((16, 24)) == (10, 16)


def _wrapper_grid(name):
    """the grid this package's wrappers plan for a fixture geometry of sc.GRIDS"""
    case, scale = name.split("_")
    g = sc.load(case + "_ac0")
    w = sc.wrapper(g, tg.toy(g))
    H, W = g["x"].shape[-2:]
    if case.startswith("p"):
        nh, nw, rows, cols = w._plan(float(scale), H, W)
        win = tuple(w.crop_size)
    else:
        nh, nw = int(w.img_scale[0] * float(scale)), int(w.img_scale[1] * float(scale))
        rows, cols = w._plan((nh, nw), float(scale))
        win = (rows[0][1] - rows[0][0], cols[0][1] - cols[0][0])
    return (nh, nw), win, [r[0] for r in rows], [c[0] for c in cols]


def test_fixture_geometries_are_planned_as_stated_and_fully_covered(quiet):
    from mscs_amd import _lib_slide as ls
    for name, grid in sc.GRIDS.items():
        (nh, nw), (wh, ww), rows_lo, cols_lo = grid
        if name != "odd":
            assert _wrapper_grid(name) == grid, name
        for n, wlen, los in ((nh, wh, rows_lo), (nw, ww, cols_lo)):
            least, cnt = ls.plan_cover(n, wlen, los)
            assert least >= 1 and len(cnt) == n and min(cnt) == least, (name, cnt)
    assert max(ls.plan_cover(22, 16, [0, 5, 6])[1]) == 3                               # sa at 0.5: cover up to 3
    assert max(ls.plan_cover(66, 16, sc.GRIDS["sa_1.5"][2])[1]) == 4 and max(ls.plan_cover(42, 24, [0, 11, 18])[1]) == 3
    # every scale of every fixture, as the wrappers plan it
    for case in ("pa", "pb", "sa", "sb"):
        for scale in sc.load(case + "_ac0")["config"]["scales_after"]:
            (nh, nw), (wh, ww), rows_lo, cols_lo = _wrapper_grid(f"{case}_{scale}")
            assert ls.plan_cover(nh, wh, rows_lo)[0] >= 1 and ls.plan_cover(nw, ww, cols_lo)[0] >= 1, (case, scale)
    # pa at 0.25 and 0.5: the whole image inside one padded window
    assert _wrapper_grid("pa_0.25") == ((7, 10), (16, 24), [0], [0]) and _wrapper_grid("pa_0.5") == ((15, 20), (16, 24), [0], [0])


def test_too_many_windows_and_empty_grids_are_refused_with_a_message(quiet):
    from mscs_amd import _lib_slide as ls
    L = ls.lib()
    lo65, lo1 = ls.ints(range(65)), ls.ints([0])
    # host checks only: both return before anything touches a device
    assert L.dsw_gather(None, None, 5, 4, 6, 16, 24, 0, lo65, 65, lo1, 1, None, 80, 24, None) == 1
    assert b"DSW_MAX_WIN" in L.dsw_last_error()
    assert L.dsw_crops(None, 3, 20, 40, 80, 24, lo1, 1, lo65, 65, 16, 24, ls.floats([0, 0, 0]), 1, None, None) == 1
    assert b"DSW_MAX_WIN" in L.dsw_last_error()
    assert ls.plan_cover(80, 16, list(range(65)))[0] == -1 and ls.plan_cover(80, 16, list(range(64)))[0] >= 0
    assert ls.plan_cover(12, 4, [0, 9]) == (0, [1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1])
    assert ls.plan_pc_windows(10, 100, 32)[0] < 1
    with pytest.raises(RuntimeError, match="DSW_MAX_WIN"):
        ls.check(L.dsw_gather(None, None, 5, 4, 6, 16, 24, 0, lo1, 1, lo65, 65, None, 16, 90, None), "dsw_gather")
    g = sc.load("sa_ac0")
    w = TTAWrapperSlide(tg.toy(g), [1.25], True, (8, 8), (200, 24), num_classes=5, img_scale=(44, 28))
    with pytest.raises(ValueError, match=r"scale 1\.25.*would be zero"):
        with torch.no_grad():
            w(torch.from_numpy(g["x"]))
    with pytest.raises(ValueError, match="strides"):
        with torch.no_grad():
            TTAWrapperPC(tg.toy(g), [1.0], num_classes=5, crop_size=(1, 1), base_size=40)(torch.from_numpy(g["x"]))


def test_standalone_plan_program_under_sanitizers(tmp_path):
    gxx = shutil.which("g++") or shutil.which("c++")
    cxx = gxx or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    # the sanitizer runtimes inside the program (clang's default): it runs as it is, whatever else the loader brings along
    static = ["-static-libasan", "-static-libubsan"] if gxx else []
    exe = str(tmp_path / "slide_plan_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static +
                       ["-I", _lib.CSRC_DIR, os.path.join(ROOT, "tests", "slide_plan_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "plan ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


# ---- the wrappers on the CPU -------------------------------------------------------------------------------------------------------
@pytest.fixture()
def quiet():
    set_verbosity(40)
    threads = torch.get_num_threads()
    torch.set_num_threads(4)            # as tools/gen_golden_slide.py
    yield
    torch.set_num_threads(threads)


@pytest.mark.parametrize("lazy", (False, True), ids=("full", "lazy"))
@pytest.mark.parametrize("case", sc.CASES)
def test_cpu_wrappers_reproduce_the_reference(case, lazy, quiet, monkeypatch):
    from mscs_amd import _lib_slide as ls
    monkeypatch.setattr(ls, "lib", lambda: (_ for _ in ()).throw(AssertionError("the HIP library was asked for a CPU tensor")))
    g = sc.load(case)
    assert os.path.getsize(os.path.join(GOLDEN, f"G19_slide_{case}.npz")) < 64 * 1024
    scales = list(g["config"]["scales"])
    model = tg.toy(g, lazy=lazy)
    w = sc.wrapper(g, model, scales)
    assert scales == g["config"]["scales_after"] and w.scales is scales and scales[-1] == 1.0      # mutated as the reference mutates it
    assert w.align_corners == g["config"]["align_corners"]
    with torch.no_grad():
        out = w(torch.from_numpy(g["x"]))
    ref = g["out"]
    print(case, "max|out - ref|", float(np.abs(out.numpy() - ref).max()), "max|ref|", float(np.abs(ref).max()))
    assert out.dtype == torch.float32 and tuple(out.shape) == ref.shape
    np.testing.assert_allclose(out.numpy(), ref, rtol=1e-4, atol=1e-5 * float(np.abs(ref).max()))
    if lazy:
        assert model.lazy_eval_logits is False


def test_constructor_surface_and_views(quiet):
    g = sc.load("sa_ac0")
    model = tg.toy(g)
    w = TTAWrapperPC(model, [0.5])
    assert (w.num_classes, tuple(w.crop_size), w.base_size, w.scales, w.flip) == (59, (512, 512), 520, [0.5, 1.0], True)
    np.testing.assert_allclose(w.padvalue, sc.PAD, rtol=0, atol=0)
    with pytest.raises(TypeError):
        TTAWrapperPC(model, [1.0], 59)                                                       # keyword-only
    w = TTAWrapperSlide(model, [0.5])
    assert (w.num_classes, w.crop_size, w.strides, w.base_size, w.flip) == (150, [512, 512], [512, 512], 512, True)
    assert w.image_scales == [((1024, 256), 0.5), ((1024, 256), 0.5), ((2048, 512), 1.0), ((2048, 512), 1.0)]
    assert w.image_flips == [True, False, True, False]                                       # each scale twice: mirrored mean, plain
    w = TTAWrapperSlide(model, [1.0], False, (5, 11), (16, 24), num_classes=5, img_scale=(44, 28))
    assert w.image_scales == [((44, 28), 1.0)] and w.image_flips == [False] and w.strides == (5, 11)
    assert w.tta_window_batch == 8 and TTAWrapperPC(model, [1.0]).tta_window_batch == 8
    assert isinstance(w, TTAWrapper) and not isinstance(w, TTAWrapperCTS)


@pytest.mark.parametrize("case", ("pa_ac0", "sa_ac1"))
def test_model_attributes_are_restored_when_the_call_raises(case, quiet):
    g = sc.load(case)

    class Raising(tg.Toy):
        def forward(self, x):
            self.seen = (self.lazy_eval_logits, self.return_features, self.get_intermediate)
            raise RuntimeError("the model refuses")
    model = Raising(5, False, lazy=True).eval()
    model.return_features, model.get_intermediate = True, "kept"
    w = sc.wrapper(g, model)
    with pytest.raises(RuntimeError, match="refuses"):
        with torch.no_grad():
            w(torch.from_numpy(g["x"]))
    assert model.seen == (False, False, False)                                               # the composition on the CPU
    assert model.lazy_eval_logits is False and model.return_features is True and model.get_intermediate == "kept"


# ---- the manager -------------------------------------------------------------------------------------------------------------------
def _bare_manager(dataset, **cfg):
    from mscs_amd.managers import HRNetManager
    g = tg.load("a_ac0")
    m = object.__new__(HRNetManager)                # dispatch only: no log directory, no dataset, no process group
    m.config = {"tta": True, "data": {"transform_values": {"crop_shape": [16, 24]}}}
    m.config.update(cfg)
    m.dataset, m.debugging, m.model = dataset, False, tg.toy(g)
    return m


def test_dispatch_through_tta_wrapper(quiet):
    from mscs_amd.managers import BaseManager
    assert BaseManager.ORIGINAL_SIZE_DATASETS == ('ADE20K', 'PASCALC')
    w = _bare_manager("PASCALC", tta_scales=[0.5])._tta_wrapper()
    assert type(w) is TTAWrapperPC and w.scales == [0.5, 1.0] and w.num_classes == 5 and w.tta_window_batch == 8
    assert (tuple(w.crop_size), w.base_size) == ((512, 512), 520)
    w = _bare_manager("PASCALC")._tta_wrapper()
    assert type(w) is TTAWrapperPC and w.scales == [0.75, 1.25, 1.5, 1.75, 2, 1.0]
    w = _bare_manager("ADE20K", strides=[341, 341], flip=False, tta_scales=[0.5, 1.5], tta_window_batch=4)._tta_wrapper()
    assert type(w) is TTAWrapperSlide
    assert (w.strides, w.flip, w.crop_size, w.scales, w.tta_window_batch, w.num_classes) == ([341, 341], False, [16, 24], [0.5, 1.5, 1.0], 4, 150)
    assert _bare_manager("ADE20K", strides=[11, 16])._tta_wrapper().flip is True
    # everything else: what _tta_model() gives
    for dataset, cfg in (("CITYSCAPES", {}), ("CITYSCAPES", {"strides": [11, 16], "flip": False, "tta_scales": [0.5]}),
                         ("ADE20K", {"tta_scales": [0.5, 1.5]}), ("CADIS", {})):
        a, b = _bare_manager(dataset, **cfg)._tta_wrapper(), _bare_manager(dataset, **cfg)._tta_model()
        assert type(a) is type(b) and type(a) in (TTAWrapper, TTAWrapperCTS) and a.scales == b.scales
        assert getattr(a, "strides", None) == getattr(b, "strides", None) and a.flip == b.flip
    m = _bare_manager("PASCALC", tta_scales=[0.5])
    m.debugging = True
    assert m._tta_wrapper().scales == [1.0]
    # _tta_model() itself is as it was
    with pytest.raises(NotImplementedError, match="TTAWrapperPC"):
        _bare_manager("PASCALC")._tta_model()
    with pytest.raises(NotImplementedError, match="TTAWrapperSlide"):
        _bare_manager("ADE20K", strides=[341, 341])._tta_model()
