"""Host half of test-time-augmentation inference: the sixth library is built next to the main one, exports and binds exactly what
its header declares and answers the shape test without touching a device; the plan (image-size rule, window grid, separable
counts, source index) agrees with a direct restatement of the reference's loops, in Python and in a stand-alone sanitized host
program; the wrappers reproduce the reference's outputs on the CPU (fixtures G17 a-d); ``lazy_eval_logits`` and the manager's
``infer()`` behave as documented."""
import ctypes
import math
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
from mscs_amd.models import TTAWrapper, TTAWrapperCTS          # (the feature: this import fails without it)
from mscs_amd.utils import set_verbosity

import _tta_golden as tg

ENTRIES = {"dtt_version", "dtt_last_error", "dtt_supported", "dtt_merge", "dtt_window_accum", "dtt_canvas_merge",
           "dtt_plan_cts_size", "dtt_plan_windows", "dtt_plan_src_index"}


def _header():
    return open(os.path.join(ROOT, "include", "dcl_tta.h")).read()


def test_sixth_library_is_built_by_the_same_target():
    from mscs_amd import _lib_tta as lt
    _lib.build()
    assert os.path.exists(lt.LIB_PATH) and os.path.basename(lt.LIB_PATH) == "libdcl_tta.so"
    assert os.path.dirname(lt.LIB_PATH) == os.path.dirname(_lib.LIB_PATH)
    flags = subprocess.run(["make", "-s", "-C", _lib.CSRC_DIR, "print-cxxflags"], capture_output=True, text=True).stdout
    assert "--offload-arch=gfx950" in flags and "-packed-fp32-ops" in flags
    mk = open(os.path.join(_lib.CSRC_DIR, "Makefile")).read()
    assert "dcl_tta" not in re.search(r"^PACKED = (.*)$", mk, re.M).group(1)           # the generic rule: built with NOPK


def test_header_exports_and_bindings_agree():
    from mscs_amd import _lib_tta as lt
    _lib.build()
    hdr = _header()
    names = sorted(set(re.findall(r"\b(dtt_[a-z0-9_]+)\s*\(", hdr)))
    assert set(names) == ENTRIES
    assert not re.findall(r"\b(dcl|dat|dco|ddc)_[a-z0-9_]+\s*\(", hdr), "another library's prefix in this library's header"
    raw = ctypes.CDLL(lt.LIB_PATH)
    for name in names:
        assert hasattr(raw, name), f"{name} declared in include/dcl_tta.h but not exported"
    assert set(lt.SIGNATURES) | {"dtt_last_error"} == set(names)
    assert not any(n.startswith("dtt_") for n in _lib.SIGNATURES)
    L = lt.lib()
    assert L.dtt_version() >= 1
    for name, sig in lt.SIGNATURES.items():
        decl = re.search(rf"\b{name}\s*\(([^;]*)\);", hdr).group(1).strip()
        assert len(sig) == (0 if decl == "void" else decl.count(",") + 1), name
    for macro, value in (("DTT_MAX_C", lt.MAX_C), ("DTT_RUN", lt.RUN)):
        assert int(re.search(rf"#define {macro} (\d+)", hdr).group(1)) == value


def test_missing_library_error_names_the_build(monkeypatch):
    from mscs_amd import _lib_tta as lt
    monkeypatch.setattr(lt, "_lib", None)
    monkeypatch.setattr(lt, "LIB_PATH", os.path.join(ROOT, "no_such_dir", "libdcl_tta.so"))
    with pytest.raises(RuntimeError) as e:
        lt.lib()
    assert "not found" in str(e.value) and "build" in str(e.value)


def test_switch_is_registered_and_defaults_on():
    from mscs_amd.debug import DebugConfig, cfg as dbg
    assert "tta_hip" in DebugConfig.__dataclass_fields__
    assert dbg.tta_hip is True or os.environ.get("DCL_TTA_HIP") == "0"


def test_supported_is_host_arithmetic():
    from mscs_amd import _lib_tta as lt
    assert lt.supported(19, 256, 512, 1024, 2048, 1024, 2048)             # Cityscapes at scale 1.0
    assert lt.supported(19, 512, 1024, 2048, 4096, 1024, 2048)            # ... at 2.0: 19 x 2048 x 4096 < 2^31
    assert lt.supported(150, 128, 128, 512, 512, 512, 512)                # ADE20K
    for c in (1, 19, 150, 1024):
        assert lt.supported(c, 1, 1, 1, 1, 1, 1), c
    for c in (0, -1, 1025):
        assert not lt.supported(c, 4, 4, 8, 8, 8, 8), c
    for i in range(1, 7):
        for bad in (0, -3):
            args = [5, 4, 4, 8, 8, 8, 8]
            args[i] = bad
            assert not lt.supported(*args), args
    # every tensor below 2^31 elements: z, the map it is resized to, the accumulator
    assert lt.supported(1, 1, 1, 1, 1, (1 << 16) - 1, 1 << 15) and not lt.supported(1, 1, 1, 1, 1, 1 << 16, 1 << 15)
    assert lt.supported(1, 1, 1, (1 << 16) - 1, 1 << 15, 1, 1) and not lt.supported(1, 1, 1, 1 << 16, 1 << 15, 1, 1)
    assert lt.supported(1, (1 << 16) - 1, 1 << 15, 1, 1, 1, 1) and not lt.supported(1, 1 << 16, 1 << 15, 1, 1, 1, 1)
    assert not lt.supported(1024, 1 << 11, 1 << 10, 1, 1, 1, 1) and lt.supported(1024, (1 << 11) - 1, 1 << 10, 1, 1, 1, 1)
    assert lt.supported(19, 2048, 4096, 2048, 4096, 8, 8) and not lt.supported(32, 8192, 8192, 8, 8, 8, 8)


# ---- the plan ----------------------------------------------------------------------------------------------------------------------
def _reference_windows(new_len, crop, stride):
    """the reference's window loop along one axis (models/TTA_wrapper_CTS.py forward), restated"""
    rows = int(np.ceil(1.0 * (new_len - crop) / stride)) + 1
    out = []
    for r in range(rows):
        h0 = r * stride
        h1 = min(h0 + crop, new_len)
        h0 = max(int(h1 - crop), 0)
        out.append((h0, h1))
    return rows, out


GRID = [(n, crop, stride) for n in (1, 7, 16, 23, 24, 36, 48, 72, 75) for crop in (1, 16, 24, 32) for stride in (1, 11, 16, 24, 40)]


def test_window_plan_agrees_with_the_references_loop():
    from mscs_amd import _lib_tta as lt
    from mscs_amd.models import ops_tta
    kinds = set()
    for n, crop, stride in GRID:
        rows, want = _reference_windows(n, crop, stride)
        count, spans, cnt = lt.plan_windows(n, crop, stride)
        mine = ops_tta.windows_1d(n, crop, stride)
        assert count == rows, (n, crop, stride)
        if rows < 1:
            kinds.add("degenerate")
            assert spans == [] and mine == []
            continue
        assert spans == want and mine == want, (n, crop, stride)
        ones = np.zeros(n, dtype=np.int64)
        for lo, hi in want:
            ones[lo:hi] += 1
        assert cnt == ones.tolist() and ops_tta.counts_1d(n, mine).tolist() == ones.tolist()
        kinds.add("shorter" if n < crop else "equal" if n == crop else "shifted" if (n - crop) % stride else "exact")
    assert kinds == {"degenerate", "shorter", "equal", "shifted", "exact"}
    # fixture B's columns at scale 1.0: the last of three windows is shifted back to 24
    assert lt.plan_windows(48, 24, 16)[1] == [(0, 24), (16, 40), (24, 48)]
    assert lt.plan_windows(24, 32, 32)[1] == [(0, 24)]                      # fixture C: the window is lower than the crop


def test_separable_counts_equal_the_count_map():
    from mscs_amd.models import ops_tta
    for (nh, ch, sh), (nw, cw, sw) in (((24, 16, 11), (48, 24, 16)), ((36, 16, 11), (72, 24, 16)), ((24, 32, 32), (48, 24, 24)),
                                       ((23, 7, 5), (31, 9, 9)), ((40, 16, 24), (16, 16, 3))):
        rows, cols = ops_tta.windows_1d(nh, ch, sh), ops_tta.windows_1d(nw, cw, sw)
        count = torch.zeros(nh, nw, dtype=torch.int32)
        for h0, h1 in rows:
            for w0, w1 in cols:
                count[h0:h1, w0:w1] += 1
        assert torch.equal(ops_tta.counts_1d(nh, rows)[:, None] * ops_tta.counts_1d(nw, cols)[None, :], count)


def test_image_size_rule_and_source_index():
    from mscs_amd import _lib_tta as lt
    from mscs_amd.models import ops_tta
    for H, W in ((1024, 2048), (20, 40), (40, 20), (30, 30), (33, 47), (511, 1023)):
        for base in (48, 2048, 513):
            for s in (0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2, 2.0, 0.33):
                long_size = int(base * s + 0.5)                           # the reference's multi_scale_aug, restated
                want = (long_size, int(W * long_size / H + 0.5)) if H > W else (int(H * long_size / W + 0.5), long_size)
                assert lt.plan_cts_size(H, W, base, s) == want == ops_tta.cts_size(H, W, base, s), (H, W, base, s)
    # the source index against torch's own resize of a ramp and of one-hot rows
    for n_in, n_out in ((6, 22), (22, 30), (9, 33), (33, 44), (5, 5), (4, 1), (1, 3), (24, 20), (72, 40)):
        for align in (False, True):
            eye = torch.eye(n_in, dtype=torch.float64)[None, None]        # [1, 1, in (value), in (position)]
            wts = torch.nn.functional.interpolate(eye, size=(n_in, n_out), mode="bilinear", align_corners=align)[0, 0]
            for dst in range(n_out):
                i0, i1, l0, l1 = lt.plan_src_index(n_in, n_out, align, dst)
                mine = np.zeros(n_in)
                mine[i0] += l0
                mine[i1] += l1
                # the fp32 source coordinate is below n_in: the scale's rounding and the product's, 2 * eps32 * n_in on the weights
                np.testing.assert_allclose(mine, wts[:, dst].numpy(), rtol=0, atol=2 * float(np.finfo(np.float32).eps) * n_in,
                                           err_msg=str((n_in, n_out, align, dst)))


def test_standalone_plan_program_under_sanitizers(tmp_path):
    gxx = shutil.which("g++") or shutil.which("c++")
    cxx = gxx or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    # the sanitizer runtimes inside the program (clang's default): it runs as it is, whatever else the loader brings along
    static = ["-static-libasan", "-static-libubsan"] if gxx else []
    exe = str(tmp_path / "tta_plan_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static +
                       ["-I", _lib.CSRC_DIR, os.path.join(ROOT, "tests", "tta_plan_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "plan ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


# ---- the wrappers on the CPU -------------------------------------------------------------------------------------------------------
@pytest.fixture()
def quiet():
    set_verbosity(40)
    threads = torch.get_num_threads()
    torch.set_num_threads(4)            # as tools/gen_golden_tta.py
    yield
    torch.set_num_threads(threads)


@pytest.mark.parametrize("lazy", (False, True), ids=("full", "lazy"))
@pytest.mark.parametrize("case", tg.CASES)
def test_cpu_wrappers_reproduce_the_reference(case, lazy, quiet, monkeypatch):
    from mscs_amd import _lib_tta as lt
    monkeypatch.setattr(lt, "lib", lambda: (_ for _ in ()).throw(AssertionError("the HIP library was asked for a CPU tensor")))
    g = tg.load(case)
    assert os.path.getsize(os.path.join(GOLDEN, f"G17_tta_{case}.npz")) < 256 * 1024
    scales = list(g["config"]["scales"])
    model = tg.toy(g, lazy=lazy)
    w = tg.wrapper(g, model, scales)
    assert scales == g["config"]["scales_after"] and w.scales is scales          # mutated as the reference mutates it
    assert w.align_corners == g["config"]["align_corners"]
    with torch.no_grad():
        out = w(torch.from_numpy(g["x"]))
    ref = g["out"]
    print(case, "max|out - ref|", float(np.abs(out.numpy() - ref).max()), "max|ref|", float(np.abs(ref).max()))
    assert out.dtype == torch.float32 and tuple(out.shape) == ref.shape
    np.testing.assert_allclose(out.numpy(), ref, rtol=1e-5, atol=1e-6 * float(np.abs(ref).max()))
    if lazy:
        assert model.lazy_eval_logits is False


def test_scale_list_and_constructor_surface(quiet):
    g = tg.load("a_ac0")
    model = tg.toy(g)
    scales = [0.5, 1.0, 2.0]
    assert TTAWrapper(model, scales).scales is scales and scales == [0.5, 1.0, 2.0]           # 1.0 present: untouched
    scales = [2.0]
    w = TTAWrapperCTS(model, scales)
    assert scales == [2.0, 1.0]                                                              # appended at the end, in place
    assert (w.crop_size, w.strides, w.base_size, w.num_classes, w.flip) == ([512, 1024], [512, 1024], 2048, 19, True)
    w = TTAWrapperCTS(model, [1.0], False, None, (32, 24), base_size=48, num_classes=5)
    assert (w.crop_size, w.strides, w.base_size, w.num_classes, w.flip) == ((32, 24), (32, 24), 48, 5, False)
    with pytest.raises(TypeError):
        TTAWrapperCTS(model, [1.0], True, None, None, 48)                                    # keyword-only
    assert not hasattr(w, "debug")
    assert TTAWrapper(torch.nn.Conv2d(3, 2, 1), [1.0]).align_corners is True                 # a model without the attribute
    assert w.flip is False and TTAWrapper(model, [1.0], flip=False).flip is False            # stored; both orientations run anyway
    a, b = TTAWrapper(model, [1.0], flip=False), TTAWrapper(model, [1.0], flip=True)
    x = torch.from_numpy(g["x"])
    with torch.no_grad():
        assert torch.equal(a(x), b(x))


def test_degenerate_window_grid_raises_naming_the_scale(quiet):
    g = tg.load("b_ac0")
    w = TTAWrapperCTS(tg.toy(g), [1.25], True, (8, 8), (100, 24), base_size=48, num_classes=5)
    with pytest.raises(ValueError, match=r"scale 1\.25"):
        with torch.no_grad():
            w(torch.from_numpy(g["x"]))


def test_ddp_wrapped_model_is_unwrapped(quiet, monkeypatch):
    from mscs_amd.models import TTA
    g = tg.load("d_ac0")
    model = tg.toy(g)

    class FakeDDP(torch.nn.Module):
        def __init__(self, module):
            super().__init__()
            self.module = module
    monkeypatch.setattr(TTA, "ddp", FakeDDP)
    assert TTAWrapper(FakeDDP(model), [1.0]).model is model


def _hrnet18(**extra):
    from mscs_amd.models import HRNet
    graph = {"dataset": "CITYSCAPES", "backbone": "hrnet18", "pretrained": False, "align_corners": True}
    graph.update(extra)
    return HRNet(config=graph, experiment=1).eval()


def test_lazy_eval_logits_on_hrnet_and_its_restoration(quiet):
    from mscs_amd.models.ops_logits import UpsampledLogits
    torch.manual_seed(0)
    model = _hrnet18()
    x = torch.randn(1, 3, 64, 64)
    with torch.no_grad():
        assert model.lazy_eval_logits is False
        full = model(x)
        assert torch.is_tensor(full) and list(full.shape) == [1, 19, 64, 64]                  # unset: nothing changes
        model.lazy_eval_logits = True
        lazy = model(x)
        assert isinstance(lazy, UpsampledLogits) and list(lazy.lowres.shape) == [1, 19, 16, 16] and lazy.size == (64, 64)
        assert lazy.align_corners is True and torch.allclose(lazy.materialize(), full, atol=1e-6)
        model.lazy_eval_logits = False

        # a wrapper call that raises restores all three attributes
        model.return_features, model.get_intermediate = True, "kept"
        w = TTAWrapper(model, [1.0])
        with pytest.raises(RuntimeError):
            w._call_model(torch.randn(1, 5, 64, 64), True)                                    # 5 input channels: the stem refuses
        assert model.lazy_eval_logits is False and model.return_features is True and model.get_intermediate == "kept"
        seen = {}
        hook = model.register_forward_pre_hook(lambda m, a: seen.update(lazy=m.lazy_eval_logits, feats=m.return_features,
                                                                        interm=m.get_intermediate))
        out = w._call_model(x, True)
        hook.remove()
        assert seen == {"lazy": True, "feats": False, "interm": False} and isinstance(out, UpsampledLogits)
        assert model.lazy_eval_logits is False and model.return_features is True and model.get_intermediate == "kept"
        # on the CPU the wrapper takes the composition and never asks for the low-resolution logits
        model.return_features = False
        hook = model.register_forward_pre_hook(lambda m, a: seen.update(lazy=m.lazy_eval_logits))
        out = w(x)
        hook.remove()
        assert seen["lazy"] is False and list(out.shape) == [1, 19, 64, 64]
        assert torch.allclose(out, 0.5 * (full + torch.flip(model(torch.flip(x, dims=[3])), dims=[3])), atol=1e-5)
    # a module without the attribute does not get one
    g = tg.load("d_ac0")
    toy = tg.toy(g)
    with torch.no_grad():
        TTAWrapper(toy, [1.0])._call_model(torch.from_numpy(g["x"]), True)
    assert not hasattr(toy, "lazy_eval_logits") and not hasattr(toy, "return_features")


# ---- the manager -------------------------------------------------------------------------------------------------------------------
def _bare_manager(dataset, **cfg):
    from mscs_amd.managers import HRNetManager
    g = tg.load("a_ac0")
    m = object.__new__(HRNetManager)                # dispatch only: no log directory, no dataset, no process group
    m.config = {"tta": True, "data": {"transform_values": {"crop_shape": [16, 24]}}}
    m.config.update(cfg)
    m.dataset, m.debugging, m.model = dataset, False, tg.toy(g)
    return m


def test_infer_dispatch_per_dataset(quiet):
    w = _bare_manager("CITYSCAPES")._tta_model()
    assert type(w) is TTAWrapperCTS and w.scales == [0.75, 1.25, 1.5, 1.75, 2, 1.0]
    assert (w.crop_size, w.strides, w.flip, w.base_size, w.num_classes) == ([16, 24], [16, 24], True, 2048, 19)
    w = _bare_manager("CITYSCAPES", strides=[11, 16], flip=False, tta_scales=[0.5])._tta_model()
    assert type(w) is TTAWrapperCTS and (w.strides, w.flip, w.scales) == ([11, 16], False, [0.5, 1.0])
    for dataset in ("ADE20K", "CADIS"):
        w = _bare_manager(dataset, tta_scales=[0.5, 1.5])._tta_model()
        assert type(w) is TTAWrapper and w.scales == [0.5, 1.5, 1.0]
    with pytest.raises(NotImplementedError, match="TTAWrapperPC"):
        _bare_manager("PASCALC")._tta_model()
    with pytest.raises(NotImplementedError, match="TTAWrapperSlide"):
        _bare_manager("ADE20K", strides=[341, 341])._tta_model()
    m = _bare_manager("CITYSCAPES")
    m.debugging = True
    assert m._tta_model().scales == [1.0]


def _cfg(tmp, **extra):
    cfg = {"name": "tta", "mode": "training", "manager": "HRNet", "cuda": False, "parallel": False,
           "gpu_device": [0], "seed": 3, "log_every_n_steps": 1000, "log_path": str(tmp), "run_id": "run0",
           "graph": {"model": "HRNet", "backbone": "hrnet18", "sync_bn": False, "pretrained": False, "align_corners": True},
           "data": {"dataset": "ADE20K", "experiment": 1, "batch_size": 2, "synthetic": True,
                    "synthetic_length": 2, "synthetic_valid_length": 2, "synthetic_mode": "blocky",
                    "transform_values": {"crop_shape": [32, 32]}},
           "loss": {"name": "LossWrapper", "losses": {"CrossEntropyLoss": 1}},
           "train": {"learning_rate": 0.01, "lr_fct": "polynomial", "optim": "SGD", "lr_batchwise": True, "epochs": 1}}
    cfg.update(extra)
    return cfg


@pytest.mark.timeout(600)
def test_infer_on_the_synthetic_dataset(tmp_path, quiet):
    from mscs_amd.managers import HRNetManager
    m = HRNetManager(_cfg(tmp_path), autostart=False)
    m.setup()
    with pytest.raises(AssertionError, match="load_checkpoint"):
        m.infer()
    path = m.save_checkpoint(path=str(tmp_path / "chk.pt"))
    outs = {}
    for tta in (True, False):
        m2 = HRNetManager(_cfg(tmp_path, mode="inference", load_checkpoint=path, tta=tta, tta_scales=[0.5]), autostart=False)
        m2.setup()
        mious = m2.infer()
        assert set(mious) == {"mean_iou", "per_class_iou", "categories"}
        assert math.isfinite(float(mious["mean_iou"])) and 0.0 <= float(mious["mean_iou"]) <= 1.0
        assert list(mious["per_class_iou"].shape) == [150] and not m2.model.training
        assert m2.model.return_features is False and m2.model.lazy_eval_logits is False
        outs[tta] = float(mious["mean_iou"])
    print(outs)
