"""Host half of the evaluation at the original label size: the ninth library is built next to the main one, exports and binds
exactly what its header declares, answers the shape test and refuses bad argument combinations without touching a device; the
two-stage taps of csrc/dcl_eval_plan.h agree with a direct restatement, in Python and in a stand-alone sanitized host program;
``evaluate_at_original`` on the CPU equals the torch composition written out here; the manager validates, saves panels and
predictions at the original size on an ADE20K ``resize_val`` config, and still raises on a CITYSCAPES one."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

import mscs_amd  # noqa: F401
from mscs_amd import _lib
from mscs_amd import _lib_eval as le                                       # (the feature: this import fails without it)
from mscs_amd.utils import evaluate_at_original, set_verbosity

import _eval_cases as cases

ENTRIES = {"dve_version", "dve_last_error", "dve_supported", "dve_evaluate", "dve_plan_taps", "dve_plan_hist_in_lds", "dve_plan_runs",
           "dve_plan_class_split"}


# ---- library surface ---------------------------------------------------------------------------------------------------------------
def test_ninth_library_is_built_by_the_same_target():
    _lib.build()
    assert os.path.exists(le.LIB_PATH) and os.path.basename(le.LIB_PATH) == "libdcl_eval.so"
    assert os.path.dirname(le.LIB_PATH) == os.path.dirname(_lib.LIB_PATH)
    mk = open(os.path.join(_lib.CSRC_DIR, "Makefile")).read()
    assert "dcl_eval" not in re.search(r"^PACKED = (.*)$", mk, re.M).group(1)          # the generic rule: built with NOPK
    assert re.search(r"^all:.*\$\(OUT_EV\)", mk, re.M) and re.search(r"^\trm -rf.*\$\(OUT_EV\)", mk, re.M)
    assert "EV.eval" in re.search(r"^SATELLITES = (.*)$", mk, re.M).group(1)
    assert re.search(r"^\$\(OBJS_EV\): dcl_bilinear\.h", mk, re.M)


def test_header_exports_and_bindings_agree():
    _lib.build()
    hdr = open(os.path.join(ROOT, "include", "dcl_eval.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(dve_[a-z0-9_]+)\s*\(", code)))
    assert set(names) == ENTRIES
    assert not re.findall(r"\b(dcl|dat|dco|ddc|dtt|dlv|dau|dpr)_[a-z0-9_]+\s*\(", hdr), "another library's prefix in this library's header"
    rawlib = ctypes.CDLL(le.LIB_PATH)
    for name in names:
        assert hasattr(rawlib, name), f"{name} declared in include/dcl_eval.h but not exported"
    assert set(le.SIGNATURES) | {"dve_last_error"} == set(names)
    assert not any(n.startswith("dve_") for n in _lib.SIGNATURES)
    assert le.lib().dve_version() >= 1
    for name, sig in le.SIGNATURES.items():
        decl = re.search(rf"\b{name}\s*\(([^;]*)\);", code).group(1).strip()
        assert len(sig) == (0 if decl == "void" else decl.count(",") + 1), name
    for macro, value in (("DVE_MAX_C", le.MAX_C), ("DVE_RUN", le.RUN), ("DVE_LDS_CELLS", le.LDS_CELLS)):
        assert int(re.search(rf"#define {macro} (\d+)", hdr).group(1)) == value


def test_missing_library_error_names_the_build(monkeypatch):
    monkeypatch.setattr(le, "_lib", None)
    monkeypatch.setattr(le, "LIB_PATH", os.path.join(ROOT, "no_such_dir", "libdcl_eval.so"))
    with pytest.raises(RuntimeError) as e:
        le.lib()
    assert "not found" in str(e.value) and "build" in str(e.value)


def test_switch_is_registered():
    from mscs_amd.debug import DebugConfig, cfg as dbg
    assert "eval_hip" in DebugConfig.__dataclass_fields__ and isinstance(dbg.eval_hip, bool)
    assert "DCL_EVAL_HIP" in open(os.path.join(os.path.dirname(_lib.CSRC_DIR), "debug.py")).read()


def test_supported_at_and_beyond_each_limit():
    for case in cases.CASES:
        C, h, w, _, Hp, Wp, rh, rw, H0, W0, _ = case
        assert le.supported(C, h or Hp, w or Wp, Hp, Wp, rh, rw, H0, W0, C) and le.supported(C, h or Hp, w or Wp, Hp, Wp, rh, rw, H0, W0, C + 1)
    ok = (19, 4, 4, 8, 8, 8, 8, 9, 9, 19)
    assert le.supported(*ok)
    assert le.supported(150, 128, 176, 512, 704, 512, 683, 1536, 2048, 151)            # the ADE20K shapes of tools/eval_time.py
    assert not le.supported(0, *ok[1:9], 0) and not le.supported(257, *ok[1:9], 257) and le.supported(256, *ok[1:9], 257)
    assert not le.supported(*ok[:9], 18) and not le.supported(*ok[:9], 21) and le.supported(*ok[:9], 20)
    for k in range(1, 9):                                                               # every size >= 1
        bad = list(ok)
        bad[k] = 0
        assert not le.supported(*bad), k
    assert not le.supported(1, 4, 4, 8, 8, 8, 8, 32768, 65536, 1) and le.supported(1, 4, 4, 8, 8, 8, 8, 32768, 65535, 1)   # H0 W0 = 2^31
    assert not le.supported(2, 4, 4, 8, 8, 8, 8, 32768, 32768, 2) and le.supported(2, 4, 4, 8, 8, 8, 8, 32768, 32767, 2)   # C H0 W0
    assert not le.supported(256, 2048, 4096, 8, 8, 8, 8, 9, 9, 256) and le.supported(255, 2048, 4096, 8, 8, 8, 8, 9, 9, 255)   # C h w
    assert not le.supported(256, 4, 4, 2048, 4096, 8, 8, 9, 9, 256) and le.supported(255, 4, 4, 2048, 4096, 8, 8, 9, 9, 255)   # C Hp Wp


def test_refused_argument_combinations_need_no_device():
    """Every refusal comes before any launch: host pointers that are never dereferenced stand in for the tensors."""
    L = le.lib()
    z = np.zeros(19 * 4 * 4, dtype=np.float32)
    lab = np.zeros(81, dtype=np.uint8)
    lut = np.zeros(256, dtype=np.uint8)
    cm = np.zeros(19 * 19, dtype=np.int32)
    oob = np.zeros(1, dtype=np.int32)
    ids = np.zeros(81, dtype=np.uint8)
    p = lambda a: a.ctypes.data                                                         # noqa: E731
    shape = (19, 4, 4, 8, 8, 0, 8, 8, 9, 9, 0)

    def call(shape=shape, label=p(lab), lbytes=1, lut_=None, cols=19, cm_=p(cm), oob_=p(oob), ids_=p(ids)):
        return L.dve_evaluate(p(z), *shape, label, lbytes, lut_, cols, cm_, oob_, ids_, None)
    for what, rc in (("label without cm", call(cm_=None)), ("label without oob", call(oob_=None)),
                     ("cm without label", call(label=None)), ("neither cm nor ids", call(label=None, cm_=None, oob_=None, ids_=None)),
                     ("lut with int64 labels", call(lbytes=8, lut_=p(lut))), ("label_bytes 2", call(lbytes=2)),
                     ("lut without a label", call(label=None, cm_=None, oob_=None, lut_=p(lut))),
                     ("rh > Hp", call(shape=(19, 4, 4, 8, 8, 0, 9, 8, 9, 9, 0))), ("rw > Wp", call(shape=(19, 4, 4, 8, 8, 0, 8, 9, 9, 9, 0))),
                     ("C = 257", call(shape=(257,) + shape[1:], cols=257)), ("cols = C + 2", call(cols=21)),
                     ("H0 = 0", call(shape=shape[:8] + (0, 9, 0)))):
        assert rc != 0, what
        assert L.dve_last_error().startswith(b"dve_evaluate"), what
    with pytest.raises(RuntimeError, match="dve_evaluate failed.*crop"):
        le.check(call(shape=(19, 4, 4, 8, 8, 0, 9, 8, 9, 9, 0)), "dve_evaluate")
    assert not cm.any() and not oob.any() and not ids.any()


# ---- the plan ----------------------------------------------------------------------------------------------------------------------
def _taps_table():
    rows = []
    for C, h, w, _, Hp, Wp, rh, rw, H0, W0, _ in cases.CASES:
        for n_in, mid, crop, out in ((h or Hp, Hp, rh, H0), (w or Wp, Wp, rw, W0)):
            for a1 in (0, 1):
                for a2 in (0, 1):
                    for dst in range(out):
                        rows.append((n_in, mid, crop, out, a1, a2, dst) + cases.taps_np(n_in, mid, crop, out, a1, a2, dst))
    return rows


def test_plan_taps_agree_with_the_restated_rule():
    for n_in, mid, crop, out, a1, a2, dst, j, m, i, l in _taps_table():
        gj, gm, gi, gl = le.plan_taps(n_in, mid, crop, out, bool(a1), bool(a2), dst)
        what = (n_in, mid, crop, out, a1, a2, dst)
        assert gj == tuple(j) and gi == tuple(i), what
        assert all(np.float32(a) == b for a, b in zip(gm, m)) and all(np.float32(a) == b for a, b in zip(gl, l)), what
        assert 0 <= gj[0] <= gj[1] <= crop - 1, what                                   # stage 2 never leaves the crop
        assert all(0 <= v <= n_in - 1 for v in gi), what                               # stage 1 never leaves the input
        assert abs(gm[0] + gm[1] - 1) <= 1.2e-7 and abs(gl[0] + gl[1] - 1) <= 1.2e-7 and abs(gl[2] + gl[3] - 1) <= 1.2e-7, what
    # the crop matters: the last output column of a cropped axis reads crop - 1, not what a resize of the whole map would read
    assert le.plan_taps(12, 48, 43, 55, False, False, 54)[0] == (42, 42)
    assert le.lib().dve_plan_taps(4, 16, 8, 8, 0, 0, 0, None, None, None, None) != 0
    with pytest.raises(RuntimeError, match="dve_plan_taps"):
        le.plan_taps(4, 16, 17, 8, False, False, 0)                                     # a crop larger than the map
    assert le.plan_runs(55) == (14, False) and le.plan_runs(96) == (24, True) and le.plan_runs(96, 2) == (24, False)
    assert le.plan_runs(0) == (0, False)
    assert le.plan_hist_in_lds(19, 20) and le.plan_hist_in_lds(64, 64) and not le.plan_hist_in_lds(150, 151) and not le.plan_hist_in_lds(256, 256)
    assert le.plan_class_split(375 * 125, 150) == 8 and le.plan_class_split(1536 * 512, 150) == 1 and le.plan_class_split(99, 15) == 1


def test_standalone_plan_program_under_sanitizers(tmp_path):
    table = tmp_path / "taps.txt"
    bits = lambda v: int(np.float32(v).view(np.uint32))                                # noqa: E731
    with open(table, "w") as f:
        for n_in, mid, crop, out, a1, a2, dst, j, m, i, l in _taps_table():
            f.write("%d %d %d %d %d %d %d %d %d %08x %08x %d %d %d %d %08x %08x %08x %08x\n" %
                    ((n_in, mid, crop, out, a1, a2, dst) + tuple(j) + tuple(bits(v) for v in m) + tuple(i) + tuple(bits(v) for v in l)))
    gxx = shutil.which("g++") or shutil.which("c++")
    cxx = gxx or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    # the sanitizer runtimes inside the program (clang's default): it runs as it is, whatever else the loader brings along
    static = ["-static-libasan", "-static-libubsan"] if gxx else []
    exe = str(tmp_path / "eval_plan_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static +
                       ["-I", _lib.CSRC_DIR, os.path.join(ROOT, "tests", "eval_plan_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(table)], capture_output=True, text=True)
    assert r.returncode == 0 and "plan ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


# ---- evaluate_at_original on the CPU -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_evaluate_cpu_equals_the_composition(case):
    C, h, w, a1, Hp, Wp, rh, rw, H0, W0, a2 = case
    z, ref, ok = cases.reference(case)
    # the three lines
    full = F.interpolate(z, size=(Hp, Wp), mode="bilinear", align_corners=bool(a1)) if h else z
    x = full[:, :, :rh, :rw]
    want = (F.interpolate(x, size=(H0, W0), mode="bilinear", align_corners=bool(a2)) if (rh, rw) != (H0, W0) else x).argmax(1)
    assert torch.equal(want[ok], ref[ok])                                              # ... agree with float64 where it decides
    from mscs_amd.utils.metrics import _cols
    dataset = "ADE20K" if C == 150 else "CITYSCAPES"
    cols = _cols(C, dataset, True)                                                      # C + 1 where the dataset has an ignore id
    assert cols == (C + 1 if C in (19, 150) else C)
    t = cases.target(case, hi=cols)
    cm, ids = evaluate_at_original(cases.wrap(z, case), t, (rh, rw), (H0, W0), bool(a2), dataset, return_ids=True)
    assert ids.dtype == torch.uint8 and tuple(ids.shape) == (1, H0, W0) and torch.equal(ids.long(), want)
    ref_cm, _ = cases.bincount_cm(want, t, C, cols)
    assert cm.dtype == torch.int32 and tuple(cm.shape) == (C, C) and torch.equal(cm.long(), ref_cm[:, :C])
    # [1, H0, W0] labels, no ids, an existing matrix
    again = evaluate_at_original(cases.wrap(z, case), t[None], (rh, rw), (H0, W0), bool(a2), dataset, existing_matrix=cm)
    assert torch.is_tensor(again) and torch.equal(again, 2 * cm)
    # through a table: raw bytes whose table entries are the targets (every target here is below 256)
    perm = torch.randperm(256, generator=torch.Generator().manual_seed(3))
    table = torch.empty(256, dtype=torch.uint8)
    table[perm] = torch.arange(256, dtype=torch.int64).to(torch.uint8)                # table[perm[v]] = v
    got = evaluate_at_original(cases.wrap(z, case), perm[t].to(torch.uint8), (rh, rw), (H0, W0), bool(a2), dataset, label_lut=table)
    assert torch.equal(got, cm)


def test_evaluate_cpu_bad_target_and_bad_crop():
    case = cases.CASES[1]
    C, h, w, a1, Hp, Wp, rh, rw, H0, W0, a2 = case
    z = cases.logits(case)
    t = cases.target(case)
    t[3, 4] = C + 1
    with pytest.raises(RuntimeError, match="Class values must be smaller than num_classes"):
        evaluate_at_original(cases.wrap(z, case), t, (rh, rw), (H0, W0), True, "CITYSCAPES")
    t[3, 4] = -1
    with pytest.raises(RuntimeError, match="Class values must be smaller than num_classes"):
        evaluate_at_original(cases.wrap(z, case), t, (rh, rw), (H0, W0), True, "CITYSCAPES")
    with pytest.raises(ValueError, match="crop"):
        evaluate_at_original(cases.wrap(z, case), cases.target(case), (Hp + 1, rw), (H0, W0), True, "CITYSCAPES")
    lazy = cases.wrap(z, case)
    evaluate_at_original(lazy, cases.target(case), (rh, rw), (H0, W0), True, "CITYSCAPES")
    assert lazy._full is not None                                                       # the composition does materialise


def test_importing_the_module_needs_no_pil():
    r = subprocess.run([os.sys.executable, "-c",
                        "import sys; sys.path.insert(0, %r); import mscs_amd; from mscs_amd.utils import evaluate; "
                        "assert not any(m == 'PIL' or m.startswith('PIL.') for m in sys.modules)" % ROOT],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


# ---- the manager -------------------------------------------------------------------------------------------------------------------
def composition_matrix(m):
    """The confusion matrix of the manager's validation set, built from the model's dense output by the composition against
    lut[raw label] at the original size; and the number of ignored pixels."""
    from mscs_amd.datasets import network_lut
    lut = network_lut(m.dataset, m.experiment)
    C = 150
    total = torch.zeros(C, C + 1, dtype=torch.int64)
    m.model.eval()
    with torch.no_grad():
        for batch in m.data_loaders["valid_loader"]:
            plan = batch[2][0]["plan"]
            assert (plan.H, plan.W, plan.rh, plan.rw, plan.Hc, plan.Wc) == (45, 70, 64, 100, 64, 128)
            img, _, _ = m._upload(*batch[:3])
            out = m._bare_model()(img.float())
            assert torch.is_tensor(out) and tuple(out.shape) == (1, C, 64, 128)
            x = F.interpolate(out[:, :, :64, :100], size=(45, 70), mode="bilinear", align_corners=True)
            t = lut[batch[1][0].to(m.device).long().cpu()].long()
            total += torch.bincount(x.argmax(1).reshape(-1).cpu() * (C + 1) + t.reshape(-1), minlength=C * (C + 1)).view(C, C + 1)
    m.model.train()
    return total[:, :C], int(total[:, C].sum())


@pytest.fixture()
def quiet():
    import random
    state = (torch.get_rng_state(), np.random.get_state(), random.getstate())
    threads = torch.get_num_threads()
    torch.set_num_threads(4)
    set_verbosity(40)
    yield
    torch.set_num_threads(threads)
    torch.set_rng_state(state[0])
    np.random.set_state(state[1])
    random.setstate(state[2])


@pytest.mark.timeout(600)
def test_manager_validates_at_the_original_size(tmp_path, quiet, monkeypatch):
    """(raises NotImplementedError without the feature)"""
    from mscs_amd.managers import HRNetManager
    from mscs_amd.utils import evaluate as ev
    m = HRNetManager(cases.manager_cfg(tmp_path), autostart=False)
    m.setup()
    seen = []
    real = ev.evaluate_at_original

    def spy(*a, **k):
        r = real(*a, **k)
        seen.append((a, k, r))
        return r
    monkeypatch.setattr(ev, "evaluate_at_original", spy)
    miou = m.validate()
    assert 0.0 <= miou <= 1.0 and m.metrics["final_miou"] == miou and m.model.training
    assert len(seen) == 2
    for a, k, _ in seen:
        assert tuple(a[2]) == (64, 100) and tuple(a[3]) == (45, 70) and a[4] is True and a[5] == "ADE20K"
        assert a[1].dtype == torch.uint8 and tuple(a[1].shape) == (45, 70) and k["label_lut"].dtype == torch.uint8
    cm = seen[-1][2]
    want, ignored = composition_matrix(m)
    assert torch.equal(cm.long(), want)
    assert int(cm.sum()) == 2 * 45 * 70 - ignored
    from mscs_amd.utils import t_get_mean_iou
    assert miou == float(t_get_mean_iou(cm))
    # max_valid_imgs still ends the loop
    m.config["max_valid_imgs"] = 1
    del seen[:]
    m.validate()
    assert len(seen) == 1


def test_cityscapes_on_resize_val_still_raises(tmp_path, quiet):
    """The reference applies the step to ADE20K and PASCAL-Context only: the same config on CITYSCAPES raises as before."""
    from mscs_amd.managers import HRNetManager
    m = HRNetManager(cases.manager_cfg(tmp_path, dataset="CITYSCAPES"), autostart=False)
    m.setup()
    with pytest.raises(NotImplementedError, match="original-label"):
        m.validate()
    m2 = HRNetManager(cases.manager_cfg(tmp_path), autostart=False)
    m2.setup()
    assert m2.validate() is not None


@pytest.mark.timeout(600)
def test_manager_saves_at_the_original_size(tmp_path, quiet):
    Image = pytest.importorskip("PIL.Image")
    from mscs_amd.datasets import network_lut
    from mscs_amd.managers import HRNetManager
    from mscs_amd.utils import class_palette, submission_lut
    m = HRNetManager(cases.manager_cfg(tmp_path / "train", save_valid_images=True), autostart=False)
    m.setup()
    path = m.save_checkpoint(path=str(tmp_path / "chk.pt"))
    m.global_step = 5
    miou = m.validate()
    base = tmp_path / "train" / "run0" / "valid_images"
    assert sorted(os.listdir(base)) == ["record_00_step5.png", "record_01_step5.png"]
    pal, lut = class_palette("ADE20K", 1), network_lut("ADE20K", 1)
    m.model.eval()
    preds = []
    with torch.no_grad():
        for i, batch in enumerate(m.data_loaders["valid_loader"]):
            panel = np.asarray(Image.open(base / f"record_{i:02d}_step5.png"))
            assert panel.shape == (45, 3 * 70, 3)
            img, _, _ = m._upload(*batch[:3])
            x = F.interpolate(m.model(img.float())[:, :, :64, :100], size=(45, 70), mode="bilinear", align_corners=True)
            preds.append(x.argmax(1)[0])
            label_colours = pal[lut[batch[1][0].long()].long()]
            assert np.array_equal(panel[:, 70:140], label_colours.numpy())             # the label panel: lut[raw], never resized
            assert np.array_equal(panel[:, 140:], pal[preds[-1]].numpy())
    # the same model and images without panels: the same mIoU
    m2 = HRNetManager(cases.manager_cfg(tmp_path / "plain", load_checkpoint=path), autostart=False)
    m2.setup()
    assert m2.validate() == miou and not os.path.exists(tmp_path / "plain" / "run0")
    # infer(): files at the original size
    runs = {}
    for name, extra in (("off", {}), ("on", {"save_outputs": True})):
        mi = HRNetManager(cases.manager_cfg(tmp_path / name, mode="inference", load_checkpoint=path, tta=False, **extra), autostart=False)
        mi.setup()
        runs[name] = mi.infer()
    assert float(runs["off"]["mean_iou"]) == float(runs["on"]["mean_iou"]) and not os.path.exists(tmp_path / "off" / "run0")
    assert torch.equal(runs["off"]["per_class_iou"], runs["on"]["per_class_iou"])
    base = tmp_path / "on" / "run0" / "outputs" / "val"
    assert sorted(os.listdir(base)) == ["debug", "submit"]
    sub = submission_lut("ADE20K", 1)
    for i in range(2):
        submit, debug = Image.open(base / "submit" / f"record_{i:06d}.png"), Image.open(base / "debug" / f"record_{i:06d}.png")
        assert submit.mode == "L" and debug.mode == "RGB" and submit.size == debug.size == (70, 45)
        assert np.array_equal(np.asarray(submit), sub[preds[i]].numpy()) and np.array_equal(np.asarray(debug), pal[preds[i]].numpy())
    # with a wrapper its dense output takes the stage-1-identity form
    from mscs_amd.models import TTAWrapper
    mt = HRNetManager(cases.manager_cfg(tmp_path / "tta", mode="inference", load_checkpoint=path, tta=True, save_outputs=True), autostart=False)
    mt.setup()
    mt._tta_model = lambda: TTAWrapper(mt.model, [0.5])
    mt.infer()
    with torch.no_grad():
        batch = list(mt.data_loaders["valid_loader"])[1]
        img, _, _ = mt._upload(*batch[:3])
        dense = TTAWrapper(mt.model, [0.5])(img.float())
        want = F.interpolate(dense[:, :, :64, :100], size=(45, 70), mode="bilinear", align_corners=True).argmax(1)[0]
    got = np.asarray(Image.open(tmp_path / "tta" / "run0" / "outputs" / "val" / "submit" / "record_000001.png"))
    assert got.shape == (45, 70) and np.array_equal(got, sub[want].numpy())
