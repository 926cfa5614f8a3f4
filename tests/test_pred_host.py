"""Host half of the saved predictions: the eighth library is built next to the main one, exports and binds exactly what its header
declares and answers the shape test without touching a device; the index arithmetic of csrc/dcl_pred_plan.h agrees with a direct
restatement in a stand-alone sanitized host program; the tables restate the reference's (fixture G18); ``predict_maps`` on the CPU;
the writer; the manager's ``save_outputs`` and ``save_valid_images``."""
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
from mscs_amd import _lib_pred as lp                                       # (the feature: this import fails without it)
from mscs_amd.models.ops_logits import UpsampledLogits
from mscs_amd.utils import (DATASETS_INFO, PredictionWriter, class_palette, panel_image, predict_maps, set_verbosity, submission_lut)

import _pred_cases as cases

ENTRIES = {"dpr_version", "dpr_last_error", "dpr_supported", "dpr_predict", "dpr_panel_supported", "dpr_panel", "dpr_plan_src_index",
           "dpr_plan_runs"}


# ---- library surface ---------------------------------------------------------------------------------------------------------------
def test_eighth_library_is_built_by_the_same_target():
    _lib.build()
    assert os.path.exists(lp.LIB_PATH) and os.path.basename(lp.LIB_PATH) == "libdcl_pred.so"
    assert os.path.dirname(lp.LIB_PATH) == os.path.dirname(_lib.LIB_PATH)
    mk = open(os.path.join(_lib.CSRC_DIR, "Makefile")).read()
    assert "dcl_pred" not in re.search(r"^PACKED = (.*)$", mk, re.M).group(1)          # the generic rule: built with NOPK
    assert re.search(r"^all:.*\$\(OUT_PR\)", mk, re.M)


def test_header_exports_and_bindings_agree():
    _lib.build()
    hdr = open(os.path.join(ROOT, "include", "dcl_pred.h")).read()
    names = sorted(set(re.findall(r"\b(dpr_[a-z0-9_]+)\s*\(", hdr)))
    assert set(names) == ENTRIES
    assert not re.findall(r"\b(dcl|dat|dco|ddc|dtt|dlv|dau)_[a-z0-9_]+\s*\(", hdr), "another library's prefix in this library's header"
    rawlib = ctypes.CDLL(lp.LIB_PATH)
    for name in names:
        assert hasattr(rawlib, name), f"{name} declared in include/dcl_pred.h but not exported"
    assert set(lp.SIGNATURES) | {"dpr_last_error"} == set(names)
    assert not any(n.startswith("dpr_") for n in _lib.SIGNATURES)
    assert lp.lib().dpr_version() >= 1
    for name, sig in lp.SIGNATURES.items():
        decl = re.search(rf"\b{name}\s*\(([^;]*)\);", hdr).group(1).strip()
        assert len(sig) == (0 if decl == "void" else decl.count(",") + 1), name
    for macro, value in (("DPR_MAX_C", lp.MAX_C), ("DPR_MAX_N", lp.MAX_N), ("DPR_RUN", lp.RUN)):
        assert int(re.search(rf"#define {macro} (\d+)", hdr).group(1)) == value


def test_missing_library_error_names_the_build(monkeypatch):
    monkeypatch.setattr(lp, "_lib", None)
    monkeypatch.setattr(lp, "LIB_PATH", os.path.join(ROOT, "no_such_dir", "libdcl_pred.so"))
    with pytest.raises(RuntimeError) as e:
        lp.lib()
    assert "not found" in str(e.value) and "build" in str(e.value)


def test_switch_is_registered_and_defaults_on():
    from mscs_amd.debug import DebugConfig, cfg as dbg
    assert "pred_hip" in DebugConfig.__dataclass_fields__
    assert dbg.pred_hip is True or os.environ.get("DCL_PRED_HIP") == "0"


def test_supported_is_host_arithmetic():
    for C, h, w, H, W in cases.SHAPES:
        assert lp.supported(1, C, h, w, H, W) and lp.supported(3, C, h, w, H, W)
    assert lp.supported(1, 19, 256, 512, 1024, 2048) and lp.supported(1, 150, 128, 128, 512, 512)
    assert not lp.supported(1, 0, 4, 4, 8, 8) and not lp.supported(1, 257, 4, 4, 8, 8) and lp.supported(1, 256, 4, 4, 8, 8)
    assert not lp.supported(0, 19, 4, 4, 8, 8) and not lp.supported(65536, 19, 4, 4, 8, 8)
    assert not lp.supported(1, 19, 4, 4, 32768, 65536, with_rgb=False)                # an output of 2^31 elements
    assert lp.supported(1, 19, 4, 4, 32768, 65535, with_rgb=False) and not lp.supported(1, 19, 4, 4, 32768, 65535, with_rgb=True)
    assert not lp.supported(1, 256, 2048, 4096, 8, 8)                                 # logits of 2^31 elements
    assert lp.panel_supported(18, 22, 8) and not lp.panel_supported(18, 22, 2) and not lp.panel_supported(15447, 15447, 1)


def _index_table():
    rows = []
    for C, h, w, H, W in cases.SHAPES + [(1, 1, 1, 7, 5), (1, 6, 9, 1, 1), (1, 256, 512, 1024, 2048)]:
        for n_in, n_out in ((h, H), (w, W)):
            for align in (0, 1):
                for dst in range(n_out):
                    rows.append((n_in, n_out, align, dst) + cases.src_index(n_in, n_out, align, dst))
    return rows


def test_plan_exports_agree_with_the_restated_rule():
    for n_in, n_out, align, dst, i0, i1, l0, l1 in _index_table()[::3]:
        g0, g1, m0, m1 = lp.plan_src_index(n_in, n_out, bool(align), dst)
        assert (g0, g1) == (i0, i1) and np.float32(m0) == l0 and np.float32(m1) == l1, (n_in, n_out, align, dst)
    assert lp.lib().dpr_plan_src_index(4, 4, 0, 4, None, None, None, None) != 0
    assert lp.plan_runs(23) == (6, False) and lp.plan_runs(24) == (6, True) and lp.plan_runs(24, 2) == (6, False)
    assert lp.plan_runs(24, 8, 3) == (6, True) and lp.plan_runs(0) == (0, False) and lp.plan_runs(8, 0, 2) == (0, False)


def test_standalone_plan_program_under_sanitizers(tmp_path):
    table = tmp_path / "index.txt"
    with open(table, "w") as f:
        for n_in, n_out, align, dst, i0, i1, l0, l1 in _index_table():
            f.write("%d %d %d %d %d %d %08x %08x\n" % (n_in, n_out, align, dst, i0, i1, int(np.float32(l0).view(np.uint32)),
                                                       int(np.float32(l1).view(np.uint32))))
    gxx = shutil.which("g++") or shutil.which("c++")
    cxx = gxx or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    # the sanitizer runtimes inside the program (clang's default): it runs as it is, whatever else the loader brings along
    static = ["-static-libasan", "-static-libubsan"] if gxx else []
    exe = str(tmp_path / "pred_plan_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static +
                       ["-I", _lib.CSRC_DIR, os.path.join(ROOT, "tests", "pred_plan_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(table)], capture_output=True, text=True)
    assert r.returncode == 0 and "plan ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


# ---- the tables --------------------------------------------------------------------------------------------------------------------
def test_submission_lut_against_the_reference_fixture():
    z = np.load(os.path.join(GOLDEN, "G18_submission_lut.npz"), allow_pickle=False)
    assert set(z.files) == {"CITYSCAPES_1", "ADE20K_0", "ADE20K_1"}        # (CITYSCAPES_0: the reference's own code raises on it)
    for key in z.files:
        dataset, experiment = key.rsplit("_", 1)
        lut = submission_lut(dataset, int(experiment))
        assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256,)
        want = z[key]
        assert want.shape == (len(DATASETS_INFO[dataset].CLASS_INFO[int(experiment)][1]),)
        assert np.array_equal(lut.numpy()[:len(want)], want), key
        assert bool((lut[len(want):] == 255).all())
    assert submission_lut("CITYSCAPES", 1)[:6].tolist() == [7, 8, 11, 12, 13, 17]
    # the experiment without a fixture, by the rule: identity on its 34 classes, the class id -1 as the byte 255
    lut0 = submission_lut("CITYSCAPES", 0)
    remap = DATASETS_INFO["CITYSCAPES"].CLASS_INFO[0][0]
    for k, ids in remap.items():
        if k != 255:
            assert int(lut0[k]) == ids[-1] % 256


def test_class_palette():
    for dataset, experiment in (("CITYSCAPES", 1), ("ADE20K", 1), ("CITYSCAPES", 0)):
        names = DATASETS_INFO[dataset].CLASS_INFO[experiment][1]
        classes = len(names) - 1 if 255 in names else len(names)
        pal = class_palette(dataset, experiment)
        assert pal.dtype == torch.uint8 and tuple(pal.shape) == (256, 3)
        assert bool((pal[classes:] == 0).all())                                         # the ignore id and every unused id: black
        used = {tuple(c) for c in pal[:classes].tolist()}
        assert len(used) == classes and (0, 0, 0) not in used                          # distinct, and none of them black
    assert class_palette("CITYSCAPES", 1)[:3].tolist() == [[128, 0, 0], [0, 128, 0], [128, 128, 0]]     # VOC colours 1, 2, 3
    override = [[i, 2 * i, 255 - i] for i in range(19)]
    pal = class_palette("CITYSCAPES", 1, override)
    assert pal[:19].tolist() == override and bool((pal[19:] == 0).all())
    assert bool((class_palette("CITYSCAPES", 1, override[:4])[4:] == 0).all())


# ---- predict_maps on the CPU -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_predict_maps_cpu_against_numpy(shape):
    C, h, w, H, W = shape
    lut, pal = cases.tables()
    z = cases.logits(C, h, w, n=2)
    # dense: numpy's arg-max (the first maximal index, as torch's), exactly
    ids, mapped, rgb = predict_maps(z, lut, pal)
    want = np.argmax(z.numpy(), axis=1)
    assert ids.dtype == torch.uint8 and np.array_equal(ids.numpy(), want)
    assert np.array_equal(mapped.numpy(), lut.numpy()[want]) and np.array_equal(rgb.numpy(), pal.numpy()[want])
    assert predict_maps(z)[1:] == (None, None)
    # low-resolution logits: the float64 restatement, near-ties left out
    for align in (False, True):
        out = UpsampledLogits(z, (H, W), align)
        ids, mapped, rgb = predict_maps(out, lut, None)
        assert rgb is None and tuple(ids.shape) == (2, H, W) and out.pred is ids
        ref, ok = cases.decided(cases.resize_np(z.numpy(), H, W, align), float(z.abs().max()))
        assert float((~ok).float().mean()) <= cases.MAX_LEFT_OUT
        assert torch.equal(ids.long()[ok], ref[ok])
        assert torch.equal(mapped, lut[ids.long()])


def test_predict_maps_refuses_what_does_not_fit():
    with pytest.raises(ValueError, match="uint8"):
        predict_maps(torch.zeros(1, 257, 2, 2))
    with pytest.raises(AssertionError):
        predict_maps(torch.zeros(1, 3, 2, 2), lut=torch.zeros(255, dtype=torch.uint8))


def test_panel_image_cpu():
    g = torch.Generator().manual_seed(8)
    H, W = 18, 22
    img = torch.randn(3, H, W, generator=g) * 1.5
    lbl = torch.randint(0, 20, (H, W), generator=g)
    ids = torch.randint(0, 19, (H, W), generator=g, dtype=torch.uint8)
    pal = class_palette("CITYSCAPES", 1)
    panel = panel_image(img, lbl, ids, pal, label_ignore=19, ids_ignore=19)
    assert panel.dtype == torch.uint8 and tuple(panel.shape) == (H, 3 * W, 3)
    mean, std = np.float32([0.485, 0.456, 0.406]), np.float32([0.229, 0.224, 0.225])
    left = np.rint(np.clip(img.numpy() * std[:, None, None] + mean[:, None, None], 0, 1) * np.float32(255)).astype(np.uint8)
    assert np.array_equal(panel[:, :W].numpy(), left.transpose(1, 2, 0))
    assert np.array_equal(panel[:, W:2 * W].numpy(), pal.numpy()[lbl.numpy()])          # (the palette's entry 19 is black already)
    assert bool((panel[:, W:2 * W][lbl == 19] == 0).all()) and bool((lbl == 19).any())
    assert np.array_equal(panel[:, 2 * W:].numpy(), pal.numpy()[ids.numpy()])
    # explicit ignore ids win over the palette
    white = torch.full((256, 3), 255, dtype=torch.uint8)
    panel = panel_image(img, lbl, ids, white, label_ignore=19, ids_ignore=int(ids[0, 0]))
    assert bool((panel[:, W:2 * W][lbl == 19] == 0).all()) and bool((panel[:, W:2 * W][lbl != 19] == 255).all())
    assert bool((panel[:, 2 * W:][ids == ids[0, 0]] == 0).all())


# ---- the writer --------------------------------------------------------------------------------------------------------------------
def test_writer_round_trip_and_error(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    g = torch.Generator().manual_seed(2)
    grey = torch.randint(0, 256, (17, 23), generator=g, dtype=torch.uint8)
    colour = torch.randint(0, 256, (17, 23, 3), generator=g, dtype=torch.uint8)
    with PredictionWriter(tmp_path / "out", depth=2) as wr:
        p1 = wr.write(os.path.join("submit", "a.png"), grey)
        assert os.path.exists(p1)                                                       # a CPU tensor: written when write() returns
        p2 = wr.write(os.path.join("debug", "a.png"), colour)
        p3 = wr.write("b.png", colour.permute(1, 0, 2))                                 # not contiguous
    a, b = Image.open(p1), Image.open(p2)
    assert a.mode == "L" and b.mode == "RGB"
    assert np.array_equal(np.asarray(a), grey.numpy()) and np.array_equal(np.asarray(b), colour.numpy())
    assert np.array_equal(np.asarray(Image.open(p3)), colour.permute(1, 0, 2).numpy())
    assert wr.written == 3 and not wr._thread.is_alive()
    wr.close()                                                                          # a second close is a no-op
    # an error in the worker surfaces at close(), and the files after it are still written
    blocker = tmp_path / "file"
    blocker.write_text("not a directory")
    wr = PredictionWriter(tmp_path / "out2")
    wr.write(os.path.join("..", "file", "x.png"), grey)                                 # its directory cannot be made
    ok = wr.write("fine.png", grey)
    with pytest.raises(OSError):
        wr.close()
    assert os.path.exists(ok) and not wr._thread.is_alive()
    with pytest.raises(AssertionError):
        wr.write("late.png", grey)


# ---- the manager -------------------------------------------------------------------------------------------------------------------
def _cfg(tmp, **extra):
    cfg = {"name": "pred", "mode": "training", "manager": "HRNet", "cuda": False, "parallel": False,
           "gpu_device": [0], "seed": 3, "log_every_n_steps": 1000, "log_path": str(tmp), "run_id": "run0", "save_checkpoints": False,
           "graph": {"model": "HRNet", "backbone": "hrnet18", "sync_bn": False, "pretrained": False, "align_corners": True},
           "data": {"dataset": "CITYSCAPES", "experiment": 1, "batch_size": 2, "num_workers": 0, "synthetic": True,
                    "synthetic_length": 2, "synthetic_valid_length": 2, "synthetic_mode": "blocky",
                    "transform_values": {"crop_shape": [32, 64]}},
           "loss": {"name": "LossWrapper", "losses": {"CrossEntropyLoss": 1}},
           "train": {"learning_rate": 0.01, "lr_fct": "polynomial", "optim": "SGD", "lr_batchwise": True, "epochs": 1}}
    cfg.update(extra)
    return cfg


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """A manager on the synthetic config and its checkpoint; the global random streams are left as they were found."""
    from mscs_amd.managers import HRNetManager
    state = (torch.get_rng_state(), np.random.get_state())
    import random
    pystate = random.getstate()
    set_verbosity(40)
    threads = torch.get_num_threads()
    torch.set_num_threads(4)
    tmp = tmp_path_factory.mktemp("pred")
    m = HRNetManager(_cfg(tmp), autostart=False)
    m.setup()
    path = m.save_checkpoint(path=str(tmp / "chk.pt"))
    yield m, path, tmp
    torch.set_num_threads(threads)
    torch.set_rng_state(state[0])
    np.random.set_state(state[1])
    random.setstate(pystate)


@pytest.mark.timeout(600)
def test_infer_save_outputs(trained, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from mscs_amd.managers import HRNetManager
    _, path, _ = trained
    runs = {}
    for name, extra in (("off", {}), ("on", {"save_outputs": True})):
        m = HRNetManager(_cfg(tmp_path / name, mode="inference", load_checkpoint=path, tta=False, **extra), autostart=False)
        m.setup()
        runs[name] = (m, m.infer())
        assert m.model.lazy_eval_logits is False
    assert not os.path.exists(tmp_path / "off" / "run0" / "outputs") and not os.path.exists(tmp_path / "off" / "run0")
    assert float(runs["off"][1]["mean_iou"]) == float(runs["on"][1]["mean_iou"])
    assert torch.equal(runs["off"][1]["per_class_iou"], runs["on"][1]["per_class_iou"])
    m = runs["on"][0]
    base = tmp_path / "on" / "run0" / "outputs" / "val"
    assert sorted(os.listdir(base)) == ["debug", "submit"]
    assert sorted(os.listdir(base / "debug")) == sorted(os.listdir(base / "submit")) == ["record_000000.png", "record_000001.png"]
    lut, pal = submission_lut("CITYSCAPES", 1), class_palette("CITYSCAPES", 1)
    with torch.no_grad():
        for i, batch in enumerate(m.data_loaders["valid_loader"]):
            want = m.model(batch[0].float()).argmax(1)[0]
            submit = Image.open(base / "submit" / f"record_{i:06d}.png")
            debug = Image.open(base / "debug" / f"record_{i:06d}.png")
            assert submit.mode == "L" and debug.mode == "RGB"
            assert np.array_equal(np.asarray(submit), lut[want].numpy())
            assert np.array_equal(np.asarray(debug), pal[want].numpy())
    # with a wrapper its dense output goes through the same step (the plain wrapper: the Cityscapes protocol works on 2048-pixel
    # images); the split's name comes from data.split
    from mscs_amd.models import TTAWrapper
    cfg = _cfg(tmp_path / "tta", mode="inference", load_checkpoint=path, tta=True, save_outputs=True)
    cfg["data"]["split"] = ["train", "test"]
    m = HRNetManager(cfg, autostart=False)
    m.setup()
    m._tta_model = lambda: TTAWrapper(m.model, [0.5])
    m.infer()
    base = tmp_path / "tta" / "run0" / "outputs" / "test" / "submit"
    assert sorted(os.listdir(base)) == ["record_000000.png", "record_000001.png"]
    with torch.no_grad():
        want = TTAWrapper(m.model, [0.5])(list(m.data_loaders["valid_loader"])[1][0].float()).argmax(1)[0]
    assert np.array_equal(np.asarray(Image.open(base / "record_000001.png")), lut[want].numpy())


def test_record_stem():
    from mscs_amd.managers import HRNetManager
    stem = HRNetManager._record_stem
    assert stem((None, None, [{"target_filename": "/a/b/x_gtFine_labelIds.png", "img_filename": "/a/y.png"}]), 0, 7) == "x_gtFine_labelIds"
    assert stem((None, None, [{"index": 1}, {"img_filename": "/a/y.jpg", "index": 2}]), 1, 7) == "y"
    assert stem((None, None, {"target_filename": ["p/one.png", "p/two.png"]}), 1, 7) == "two"
    assert stem((None, None, {"index": torch.tensor([4])}), 0, 7) == "record_000007" and stem((None, None), 0, 12) == "record_000012"


@pytest.mark.timeout(600)
def test_validate_save_valid_images(trained, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from mscs_amd.managers import HRNetManager
    _, path, _ = trained
    got = {}
    for name, extra in (("off", {}), ("on", {"save_valid_images": True})):
        m = HRNetManager(_cfg(tmp_path / name, load_checkpoint=path, **extra), autostart=False)
        m.setup()
        m.global_step = 5
        got[name] = m.validate()
        assert m.model.training
    assert got["off"] == got["on"] and not os.path.exists(tmp_path / "off" / "run0")
    base = tmp_path / "on" / "run0" / "valid_images"
    assert sorted(os.listdir(base)) == ["record_00_step5.png", "record_01_step5.png"]
    pal = class_palette("CITYSCAPES", 1)
    m.model.eval()
    with torch.no_grad():
        for i, batch in enumerate(m.data_loaders["valid_loader"]):
            panel = np.asarray(Image.open(base / f"record_{i:02d}_step5.png"))
            assert panel.shape == (32, 3 * 64, 3)
            want = panel_image(batch[0][0], batch[1][0], m.model(batch[0].float()).argmax(1)[0], pal, label_ignore=19, ids_ignore=19)
            assert np.array_equal(panel, want.numpy())
            assert np.array_equal(panel[:, 64:128], pal.numpy()[batch[1][0].numpy()])
