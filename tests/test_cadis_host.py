"""Host half of the CaDIS input path: the twelfth library is built next to the main one and exports and binds exactly what its header
declares; its host arithmetic in a stand-alone sanitized program; the torch composition's blur against PIL's GaussianBlur and the
chain against fixtures of the reference's Resize, PadNP and BlurPIL; ``planner_for`` and the extended planner; the CaDIS reader on a
tiny tree built from an excerpt of the reference's frame table; the repeat-factor sampler against fixtures of the reference's; the
manager on the CPU with the real reader and the repeat-factor schedule."""
import csv
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import mscs_amd  # noqa: F401
from mscs_amd import _lib
from mscs_amd import _lib_blur as lb                                       # (the feature: this import fails without it)
from mscs_amd.datasets import augment as A
from mscs_amd.datasets import raw as R
from mscs_amd.utils import DATASETS_INFO, set_verbosity
from mscs_amd.utils.repeat_factor_sampling import RepeatFactorSampler

import _cadis_cases as cases

GOLDEN = os.path.join(ROOT, "tests", "golden")
TABLE = os.path.join(GOLDEN, "cadis_frames_v1_v5.csv")
ENTRIES = {"dbl_version", "dbl_last_error", "dbl_supported", "dbl_box", "dbl_blur", "dbl_pad_rows", "dbl_gray_mean", "dbl_colour",
           "dbl_from_unit", "dbl_normalise"}
# PIL rounds to uint8 after each of its six passes (<= 0.5 each, and its weights are 24-bit fixed point); every pass is a convex
# combination, so these errors add and do not grow: 6 x 0.5 + 0.1
PIL_BLUR_BOUND = 3.1


@pytest.fixture(scope="module", autouse=True)
def leave_no_state():
    """The modules that run after this one find the global random streams as this one found them (a manager's setup() seeds them)."""
    state = cases.save_state()
    yield
    cases.restore_state(state)


# ---- library surface ---------------------------------------------------------------------------------------------------------------
def test_twelfth_library_is_built_by_the_same_target():
    _lib.build()
    assert os.path.exists(lb.LIB_PATH) and os.path.basename(lb.LIB_PATH) == "libdcl_blur.so"
    assert os.path.dirname(lb.LIB_PATH) == os.path.dirname(_lib.LIB_PATH)
    mk = open(os.path.join(_lib.CSRC_DIR, "Makefile")).read()
    assert "BL.blur" in re.search(r"^SATELLITES = (.*)$", mk, re.M).group(1)
    assert "dcl_blur" not in re.search(r"^PACKED = (.*)$", mk, re.M).group(1)          # the generic rule: built with NOPK
    assert re.search(r"^all:.*\$\(OUT_BL\)", mk, re.M)
    # one copy of the colour operations: both libraries include the header, neither source defines them
    for name in ("dcl_aug.hip", "dcl_blur.hip"):
        src = open(os.path.join(_lib.CSRC_DIR, name)).read()
        assert '#include "dcl_colour.h"' in src and not re.search(r"Rgb\s+(colour_ops|hue_shift)\s*\(", src), name


def test_header_exports_and_bindings_agree():
    _lib.build()
    hdr = open(os.path.join(ROOT, "include", "dcl_blur.h")).read()
    names = sorted(set(re.findall(r"\b(dbl_[a-z0-9_]+)\s*\(", hdr)))
    assert set(names) == ENTRIES
    assert not re.findall(r"\b(dcl|dau|dat|dco|ddc|dtt|dlv)_[a-z0-9_]+\s*\(", hdr), "another library's prefix in this library's header"
    rawlib = ctypes.CDLL(lb.LIB_PATH)
    for name in names:
        assert hasattr(rawlib, name), f"{name} declared in include/dcl_blur.h but not exported"
    assert set(lb.SIGNATURES) | {"dbl_last_error"} == set(names)
    assert not any(n.startswith("dbl_") for n in _lib.SIGNATURES)
    assert lb.lib().dbl_version() >= 1
    for name, sig in lb.SIGNATURES.items():
        decl = re.search(rf"\b{name}\s*\(([^;]*)\);", hdr).group(1).strip()
        assert len(sig) == (0 if decl == "void" else decl.count(",") + 1), name
    for macro, value in (("DBL_MAX_RADIUS", lb.MAX_RADIUS), ("DBL_MAX_CHANNELS", lb.MAX_CHANNELS), ("DBL_ROW_TILE_H", lb.ROW_TILE_H),
                         ("DBL_ROW_TILE_W", lb.ROW_TILE_W), ("DBL_COL_TILE_H", lb.COL_TILE_H), ("DBL_COL_TILE_W", lb.COL_TILE_W),
                         ("DBL_WS_INTS", lb.WS_INTS), ("DBL_WS_TICKET", lb.WS_TICKET), ("DBL_WS_MEAN", lb.WS_MEAN),
                         ("DBL_WS_PART", lb.WS_PART), ("DBL_MAX_BLOCKS", lb.MAX_BLOCKS)):
        assert int(re.search(rf"#define {macro} (\d+)", hdr).group(1)) == value
    assert lb.WS_PART + 2 * lb.MAX_BLOCKS <= lb.WS_INTS and lb.WS_TICKET < lb.WS_MEAN < lb.WS_PART
    from mscs_amd import _lib_aug as la                                   # one workspace row serves both libraries
    assert (lb.WS_INTS, lb.WS_TICKET, lb.WS_MEAN, lb.WS_PART) == (la.WS_INTS, la.WS_TICKET, la.WS_MEAN, la.WS_PART)
    body = re.search(r"typedef struct dbl_colour_plan \{(.*?)\} dbl_colour_plan;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"\[.*", "", f.strip()) for d in body.split(";") if d.strip() for f in d.split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in lb.CColourPlan._fields_] and ctypes.sizeof(lb.CColourPlan) == 44
    # a column tile with its halo at the largest radius, twice, stays under 64 KB of LDS
    assert 2 * (lb.COL_TILE_H + 6 * lb.MAX_RADIUS) * lb.COL_TILE_W * 4 < 64 * 1024


def test_missing_library_error_names_the_build(monkeypatch):
    monkeypatch.setattr(lb, "_lib", None)
    monkeypatch.setattr(lb, "LIB_PATH", os.path.join(ROOT, "no_such_dir", "libdcl_blur.so"))
    with pytest.raises(RuntimeError) as e:
        lb.lib()
    assert "not found" in str(e.value) and "build" in str(e.value)


def test_switch_is_registered_and_defaults_on():
    from mscs_amd.debug import DebugConfig, cfg as dbg
    assert "blur_hip" in DebugConfig.__dataclass_fields__
    assert dbg.blur_hip is True or os.environ.get("DCL_BLUR_HIP") == "0"


def _box_restated(R):
    """the rule of the header, written directly"""
    s2 = R * R / 3
    l = int(np.floor((np.sqrt(12 * s2 + 1) - 1) / 2))
    a = (2 * l + 1) * (l * (l + 1) - 3 * s2) / (6 * (s2 - (l + 1) ** 2))
    ww = 1 / (2 * (l + a) + 1)
    return l, np.float32(ww), np.float32((1 - (2 * l + 1) * ww) / 2)


def test_box_and_limits_are_host_arithmetic():
    for R in range(1, lb.MAX_RADIUS + 1):
        l, ww, fw = _box_restated(R)
        assert lb.box(R) == (l, float(ww), float(fw)) == A.box_of(R) and 2 * l + 3 <= 17
        assert abs((2 * l + 1) * float(ww) + 2 * float(fw) - 1) < 1e-6                 # the weights of a pass sum to 1
    assert [A.box_of(R)[0] for R in (3, 4, 5, 6, 8)] == [2, 3, 4, 5, 7]
    assert lb.supported(3, 540, 960, 3) and lb.supported(1, 1, 1, 8) and lb.supported(4, 5, 7, 1)
    assert not lb.supported(3, 540, 960, 0) and not lb.supported(3, 540, 960, 9) and not lb.supported(3, 540, 960, 3.5)
    assert not lb.supported(5, 8, 8, 3) and not lb.supported(0, 8, 8, 3) and not lb.supported(3, 0, 8, 3)
    assert lb.supported(1, 46340, 46340, 3) and not lb.supported(1, 46341, 46341, 3)                       # below 2^31 elements
    rc = lb.lib().dbl_box(9, ctypes.byref(ctypes.c_int()), ctypes.byref(ctypes.c_float()), ctypes.byref(ctypes.c_float()))
    assert rc != 0


def test_standalone_plan_program_under_sanitizers(tmp_path):
    table = tmp_path / "boxes.txt"
    with open(table, "w") as f:
        for R in range(1, lb.MAX_RADIUS + 1):
            l, ww, fw = _box_restated(R)
            f.write("%d %d %08x %08x\n" % (R, l, int(ww.view(np.uint32)), int(fw.view(np.uint32))))
    gxx = shutil.which("g++") or shutil.which("c++")
    cxx = gxx or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    # the sanitizer runtimes inside the program (clang's default): it runs as it is, whatever else the loader brings along
    static = ["-static-libasan", "-static-libubsan"] if gxx else []
    exe = str(tmp_path / "blur_plan_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined"] + static +
                       ["-I", _lib.CSRC_DIR, os.path.join(ROOT, "tests", "blur_plan_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(table)], capture_output=True, text=True)
    assert r.returncode == 0 and "blur plan ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


# ---- the composition against PIL and the reference's transforms ---------------------------------------------------------------------
@pytest.mark.parametrize("size", ((5, 7), (33, 65), (96, 160)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_blur_against_pil(size):
    """max |float64 composition - PIL| <= 3.1 grey levels (PIL_BLUR_BOUND; measured <= 2.1), and the bound tells radii apart: for
    R = 3 .. 6 the composition at R - 1 and at R + 1 is MORE than 3.1 away from PIL at R (measured >= 5.7 on these images)."""
    Image = pytest.importorskip("PIL.Image")
    ImageFilter = pytest.importorskip("PIL.ImageFilter")
    src = cases.structured(*size, seed=1)
    x = torch.from_numpy(src).double()
    for radius in (1, 3, 4, 5, 6):
        ref = np.asarray(Image.fromarray(src).filter(ImageFilter.GaussianBlur(radius))).astype(np.float64)
        err = float(np.abs(A.gaussian_blur(x, radius).numpy() - ref).max())
        others = [float(np.abs(A.gaussian_blur(x, r).numpy() - ref).max()) for r in (radius - 1, radius + 1) if radius >= 3]
        print(size, "R", radius, "max |composition - PIL|:", err, " at R - 1, R + 1:", others)
        assert err <= PIL_BLUR_BOUND, radius
        assert all(o > PIL_BLUR_BOUND for o in others), radius


def test_reference_transform_fixtures():
    g = np.load(os.path.join(GOLDEN, "cadis_transforms.npz"))
    img, lbl = cases.source(37, 53, 7)
    assert np.array_equal(g["img"], img.numpy()) and np.array_equal(g["lbl"], lbl.numpy())
    lut = cases.identity_lut()
    # Resize(target_size=[64, 96], fit_stride=32): labels and geometry exact (no output index of 37 -> 64 or 53 -> 96 lies on PIL's
    # accumulated-double boundary: (2 o + 1) S is odd), image within test_aug_host.test_image_resize_against_pil's 1.01 levels
    for target, stride, shape in (([64, 96], 32, (64, 96)), ([40, 61], 32, (64, 64))):
        p = A.planner_for(["resize"], {"target_size": target, "fit_stride": stride}, "CADIS", 2, 0).plan(37, 53, 0, 0)
        assert (p.rh, p.rw) == tuple(target) and (p.Hc, p.Wc, p.h, p.w) == shape * 2 and (p.pt, p.pl) == (0, 0) and p.ignore == 17
    p = A.planner_for(["resize"], {"target_size": [64, 96], "fit_stride": 32}, "CADIS", 2, 0).plan(37, 53, 0, 0)
    x, y, _ = A.apply_plan_torch(img, lbl, p, lut, torch.float64)
    assert not p.normalise and np.array_equal(y.numpy(), g["resize_lbl"])
    got = (x * 255).permute(1, 2, 0).numpy()
    assert got.shape == g["resize_img"].shape and float(np.abs(np.floor(got + 0.5) - g["resize_img"]).max()) <= 1.01
    # PadNP(ver=(2, 2), hor=(0, 0), 'reflect')
    p = A.planner_for(["pad"], {}, "CADIS", 2, 0).plan(37, 53, 0, 0)
    assert p.chain == (("pad", 2, 2),) and (p.out_h, p.out_w) == (41, 53)
    x, y, _ = A.apply_plan_torch(img, lbl, p, lut, torch.float64)
    assert np.array_equal(y.numpy(), g["pad_lbl"]) and np.array_equal(np.floor((x * 255).permute(1, 2, 0).numpy() + 0.5), g["pad_img"])
    # BlurPIL(probability=1, kernel_limits=(3, 7)) at the radii it drew
    assert set(g["blur_radii"].tolist()) >= {3, 4, 6}
    for seed, radius in enumerate(g["blur_radii"].tolist()):
        err = float(np.abs(A.gaussian_blur(img.double(), radius).numpy() - g[f"blur{seed}"]).max())
        print("BlurPIL seed", seed, "R", radius, "max |composition - reference|:", err)
        assert err <= PIL_BLUR_BOUND


# ---- the planner -------------------------------------------------------------------------------------------------------------------
TRAIN = ["flip", "random_scale", "RandomCropImgLbl", "colorjitter", "torchvision_normalise"]
VALUES = {"crop_shape": [512, 1024], "crop_class_max_ratio": 0.75, "scale_range": [0.5, 2]}
PAIRS = [(e, i) for e in range(5) for i in (0, 1, 7, 16, 17, 100, 1001, 5000, 12345, 99999)]


def test_planner_for_gives_the_earlier_plans():
    assert len(PAIRS) == 50
    lists = [(TRAIN, VALUES, "CITYSCAPES", 1)]
    for name in sorted(os.listdir(os.path.join(GOLDEN, "reference_configs"))):
        d = json.load(open(os.path.join(GOLDEN, "reference_configs", name)))["data"]
        lists.append((d["transforms"], d["transform_values"], d["dataset"], d["experiment"]))
        lists.append((d["transforms_val"], d["transform_values_val"], d["dataset"], d["experiment"]))
    assert len(lists) == 7
    for transforms, values, dataset, experiment in lists:
        new, old = A.planner_for(transforms, values, dataset, experiment, 5), A.AugmentPlanner(transforms, values, dataset, experiment, 5)
        assert type(new) is A.AugmentPlanner
        # and the extended planner itself draws the same plans: its own draws come after every earlier one
        ext = A.ChainPlanner(transforms, values, dataset, experiment, 5)
        ext_blur = A.ChainPlanner(list(transforms) + ["blur"], dict(values, blur_p=0), dataset, experiment, 5)
        for epoch, index in PAIRS:
            want = old.plan(600, 800, epoch, index)
            assert new.plan(600, 800, epoch, index) == want and want.chain == ()
            assert ext.plan(600, 800, epoch, index) == want and ext_blur.plan(600, 800, epoch, index) == want


def test_blur_draws():
    from dataclasses import replace
    pl = A.planner_for(TRAIN[:3] + ["blur"] + TRAIN[3:], VALUES, "CITYSCAPES", 1, 2)
    assert type(pl) is A.ChainPlanner and (pl.blur_p, pl.blur_limits) == (0.05, (3, 7))
    base = A.AugmentPlanner(TRAIN, VALUES, "CITYSCAPES", 1, 2)
    blurred = 0
    for i in range(4000):
        p = pl.plan(1024, 2048, 0, i)
        if p.chain:
            blurred += 1
            assert p.chain[0][0] == "blur" and p.chain[1:] == (("colour",),) and 3 <= p.chain[0][1] <= 6      # in the list's order
        assert replace(p, chain=()) == base.plan(1024, 2048, 0, i)
    print("blurred", blurred, "of 4000")
    assert abs(blurred / 4000 - 0.05) <= 0.015                               # 4 sigma of the binomial: 4 sqrt(.05 .95 / 4000) = 0.0138
    always = A.planner_for(["blur", "torchvision_normalise"], {"blur_p": 1}, "CITYSCAPES", 1, 2)
    radii = [always.plan(64, 64, 0, i).chain for i in range(400)]
    assert all(len(c) == 1 and c[0][0] == "blur" for c in radii) and {c[0][1] for c in radii} == {3, 4, 5, 6}
    wide = A.planner_for(["blur"], {"blur_p": 1, "blur_kernel_limits": [1, 3]}, "CITYSCAPES", 1, 2)
    assert {wide.plan(64, 64, 0, i).chain[0][1] for i in range(100)} == {1, 2}
    # the order of the list is the order of the chain
    first = A.planner_for(["colorjitter", "blur"], {"blur_p": 1}, "CITYSCAPES", 1, 2).plan(64, 64, 0, 0)
    assert [c[0] for c in first.chain] == ["colour", "blur"] and sorted(first.perm) == [0, 1, 2, 3]


def test_key_rules_and_errors_name_their_key():
    with pytest.raises(ValueError, match="pad"):
        A.planner_for(["flip", "pad"], {}, "CITYSCAPES", 1, 0)
    with pytest.raises(ValueError, match="resize"):
        A.planner_for(["resize"], {"fit_stride": 32}, "CADIS", 2, 0)
    with pytest.raises(ValueError, match="no_such_transform"):
        A.planner_for(["pad", "no_such_transform"], {}, "CADIS", 2, 0)
    with pytest.raises(ValueError, match="blur"):
        A.planner_for(["blur"], {"blur_kernel_limits": [4, 4]}, "CADIS", 2, 0)
    # pad: 2 + 2 rows, on the training and on the validation list alike
    p = A.planner_for(["pad", "flip", "blur", "colorjitter", "torchvision_normalise"], {"blur_p": 1}, "CADIS", 2, 0).plan(540, 960, 0, 0)
    assert [c[0] for c in p.chain] == ["pad", "blur", "colour"] and p.chain[0] == ("pad", 2, 2) and (p.out_h, p.out_w) == (544, 960)
    assert (p.h, p.w, p.ignore) == (540, 960, 17) and p.normalise
    # min_side_length is read under its own name (the reference looks it up under 'min_size_length' and never finds it)
    p = A.planner_for(["resize"], {"min_side_length": 64}, "CADIS", 2, 0).plan(100, 70, 0, 0)
    assert (p.rw, p.rh, p.Hc, p.Wc, p.h, p.w) == (64, int(round(100 * 64 / 70)), 91, 64, 91, 64)
    # Resize(target_size=[64, 96], fit_stride=32) on 37 x 53 and 100 x 70: the target, then bottom and right to the stride
    for target, stride, canvas in (([64, 96], 32, (64, 96)), ([50, 70], 32, (64, 96)), ([64, 96], None, (64, 96)), ([50, 70], None, (50, 70))):
        for H, W in ((37, 53), (100, 70)):
            p = A.planner_for(["resize"], {"target_size": target, "fit_stride": stride}, "CADIS", 2, 0).plan(H, W, 0, 0)
            assert (p.rh, p.rw) == tuple(target) and (p.Hc, p.Wc) == canvas == (p.h, p.w) and (p.pt, p.pl) == (0, 0) and p.corners == [(0, 0)]
            assert p.chain == () and la_supported(p)


def la_supported(plan):
    from mscs_amd import _lib_aug as la
    return la.supported(la.c_plan(plan))


def test_experiment_without_an_ignore_class():
    assert A.ignore_id("CADIS", 1) == -1 and A.ignore_id("CADIS", 2) == 17
    with pytest.raises(ValueError, match="ignore"):
        A.AugmentPlanner(["flip"], {}, "CADIS", 1, 0)
    pl = A.planner_for(["pad", "flip", "blur", "colorjitter"], {"blur_p": 1}, "CADIS", 1, 0)
    p = pl.plan(12, 16, 0, 0)
    assert p.ignore == A.NO_IGNORE == 255 and int(A.network_lut("CADIS", 1).max()) == 7 and la_supported(p)
    crop = A.planner_for(["RandomCropImgLbl"], {"crop_shape": [8, 8], "crop_class_max_ratio": 0.75}, "CADIS", 1, 0).plan(12, 16, 0, 0)
    assert len(crop.corners) == 10 and crop.ignore == 255
    # every class counts in the crop choice: a window of one class is refused, as the reference's -1 refuses it
    assert A.candidate_verdict(torch.full((4, 4), 7, dtype=torch.uint8), 255, 0.75) == (False, 16, 16)
    for key, values in (("random_scale", {"crop_shape": [8, 8], "scale_range": [0.5, 2]}),
                        ("resize", {"target_size": [8, 8], "fit_stride": 32}), ("resize_val", {"min_side_length": 8, "fit_stride_val": 32})):
        with pytest.raises(ValueError, match=key):
            A.planner_for(["flip", key], values, "CADIS", 1, 0)
    assert A.planner_for(["resize"], {"target_size": [8, 8]}, "CADIS", 1, 0).plan(12, 16, 0, 0).h == 8        # nothing pads: accepted


def test_chain_composition_properties():
    """The chain in torch: pad before or after the blur differ, the colour item applies perm exactly once, labels follow pads only."""
    from dataclasses import replace
    img, lbl = cases.source(33, 65, 7)
    lut = cases.identity_lut()
    base = A.Plan(H=33, W=65, rh=33, rw=65, Hc=33, Wc=65, pt=0, pl=0, h=33, w=65, perm=(1, 0, 2, 3), ignore=19, normalise=False, **cases.COL)
    plain, y0, _ = A.apply_plan_torch(img, lbl, base, lut, torch.float64)
    forced, y1, _ = A.apply_plan_torch(img, lbl, replace(base, chain=(("colour",),)), lut, torch.float64)
    assert torch.equal(y0, y1) and float((plain - forced).abs().max()) < 1e-12
    none, _, _ = A.apply_plan_torch(img, lbl, replace(base, chain=(("pad", 0, 0),)), lut, torch.float64)   # no colour item: perm is not run
    assert float((none * 255 - img.permute(2, 0, 1).double()).abs().max()) < 1e-9
    a, ya, _ = A.apply_plan_torch(img, lbl, replace(base, perm=(), chain=(("pad", 2, 3), ("blur", 3))), lut, torch.float64)
    b, yb, _ = A.apply_plan_torch(img, lbl, replace(base, perm=(), chain=(("blur", 3), ("pad", 2, 3))), lut, torch.float64)
    assert tuple(a.shape) == tuple(b.shape) == (3, 38, 65) and torch.equal(ya, yb) and float((a - b).abs().max()) > 1e-3
    assert np.array_equal(ya.numpy(), np.pad(lbl.numpy(), ((2, 3), (0, 0)), mode="reflect"))
    # CPU tensors take the composition, whatever the switches say
    aug = A.DeviceAugment(lut)
    plan = replace(base, chain=(("pad", 2, 2), ("blur", 4), ("colour",)), normalise=True)
    x, y = aug([img], [lbl], [plan])
    ex, ey, _ = A.apply_plan_torch(img, lbl, plan, lut)
    assert aug.last_paths == ["torch"] and torch.equal(x[0], ex) and torch.equal(y[0], ey) and tuple(x.shape) == (1, 3, 37, 65)


# ---- the reader --------------------------------------------------------------------------------------------------------------------
def _rows():
    with open(TABLE, newline="") as f:
        return list(csv.DictReader(f))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """A CaDIS folder for the excerpt's rows: 12 x 16 PNGs, labels in the raw ids 0 .. 35, and relabeled/ copies."""
    Image = pytest.importorskip("PIL.Image")
    root = tmp_path_factory.mktemp("cadis")
    rng = np.random.default_rng(31)
    for r in _rows():
        for key, shape, hi in (("img_path", (12, 16, 3), 256), ("lbl_path", (12, 16), 36)):
            path = root.joinpath(*r[key].split("\\"))
            path.parent.mkdir(parents=True, exist_ok=True)
            Image.fromarray(rng.integers(0, hi, shape, dtype=np.uint8)).save(path)
    (root / "relabeled").mkdir()
    return root


def _table(tmp_path, rows, drop=()):
    path = tmp_path / "data.csv"
    names = [k for k in rows[0] if k not in drop]
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=names, extrasaction="ignore")
        w.writeheader()
        w.writerows(rows)
    return str(path)


def test_split_table_is_data():
    splits = DATASETS_INFO["CADIS"].DATA_SPLITS
    assert len(splits) == 6 and splits[0] == [[1], [5]] and [len(s) for s in splits] == [2, 2, 2, 2, 2, 3]
    assert splits[2][0] == list(range(1, 26)) and sorted(splits[5][1] + splits[5][2]) == sorted(splits[1][1]) and splits[5][0] == splits[1][0]
    assert all(not set(s[0]) & set(s[1]) for i, s in enumerate(splits) if i != 2)


def test_reader_filters_as_the_reference(tree, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rows = _rows()
    assert len(rows) == 355 and "propagated" not in rows[0]
    planner = A.planner_for(["pad", "flip"], {}, "CADIS", 2, 0)
    train = R.CaDIS(str(tree), TABLE, split=0, experiment=2, planner=planner, subset="train")
    valid = R.CaDIS(str(tree), rows, split=0, experiment=2, planner=None, subset="valid")          # no 'propagated' column: all kept
    assert (len(train), len(valid)) == (177, 178)
    assert [r["img_path"] for r in train.rows] == [r["img_path"] for r in rows if r["vid_num"] == "1"]
    assert all(r["vid_num"] == "5" for r in valid.rows)
    train.set_epoch(1)
    img, lbl, meta = train[3]
    assert img.dtype == torch.uint8 and tuple(img.shape) == (12, 16, 3) and lbl.dtype == torch.uint8 and tuple(lbl.shape) == (12, 16)
    assert train.images[3] == os.path.join(str(tree), *rows[3]["img_path"].split("\\"))
    assert np.array_equal(img.numpy(), np.asarray(Image.open(train.images[3]).convert("RGB")))
    assert np.array_equal(lbl.numpy(), np.asarray(Image.open(train.targets[3])))
    assert meta["index"] == 3 and meta["plan"] == planner.plan(12, 16, 1, 3) and meta["plan"].out_h == 16
    # split 5 is three-way: training validates on its second list, inference on its third; videos 1 and 5 are in lists 0 and 1
    assert len(R.CaDIS(str(tree), rows, split=5, subset="train")) == 177 and len(R.CaDIS(str(tree), rows, split=5, subset="valid")) == 178
    assert len(R.CaDIS(str(tree), rows, split=5, subset="valid", mode="inference")) == 0
    # propagated validation frames leave; training frames stay
    flagged = [dict(r, propagated="1" if n % 2 else "0") for n, r in enumerate(rows)]
    assert len(R.CaDIS(str(tree), flagged, split=0, subset="valid")) == sum(1 for n, r in enumerate(rows) if r["vid_num"] == "5" and n % 2 == 0)
    assert len(R.CaDIS(str(tree), flagged, split=0, subset="train")) == 177
    # blacklist drops, use_relabeled reads relabeled/<name> and takes the frame off the blacklist
    marked = [dict(r) for r in rows]
    for n in (2, 5, 9):
        marked[n]["blacklisted"] = "1"
    marked[5]["relabeled"] = "1"
    assert len(R.CaDIS(str(tree), _table(tmp_path, marked), split=0, subset="train", blacklist=True)) == 174
    assert len(R.CaDIS(str(tree), marked, split=0, subset="train", blacklist=False)) == 177
    name = os.path.basename(marked[5]["lbl_path"])
    with pytest.raises(FileNotFoundError, match=re.escape(os.path.join("relabeled", name))):
        R.CaDIS(str(tree), marked, split=0, subset="train", use_relabeled=True)
    shutil.copy(os.path.join(str(tree), *marked[5]["lbl_path"].split("\\")), os.path.join(str(tree), "relabeled", name))
    ds = R.CaDIS(str(tree), marked, split=0, subset="train", use_relabeled=True, blacklist=True)
    assert len(ds) == 175 and ds.targets[4] == os.path.join(str(tree), "relabeled", name) and ds.rows[4]["blacklisted"] == "0"
    # backslashes separate folders as well
    back = [dict(r, img_path=r["img_path"].replace("/", "\\"), lbl_path=r["lbl_path"].replace("/", "\\")) for r in rows]
    assert R.CaDIS(str(tree), back, split=0, subset="train").images == train.images


def test_reader_errors_name_what_is_missing(tree, tmp_path):
    rows = _rows()
    with pytest.raises(KeyError, match="img_path"):
        R.CaDIS(str(tree), _table(tmp_path, rows, drop=("img_path",)), split=0)
    with pytest.raises(FileNotFoundError, match="no_such_table.csv"):
        R.CaDIS(str(tree), str(tmp_path / "no_such_table.csv"), split=0)
    gone = [dict(r) for r in rows]
    gone[7]["img_path"] = "Video01/Images/no_such_frame.png"
    with pytest.raises(FileNotFoundError, match="no_such_frame.png"):
        R.CaDIS(str(tree), gone, split=0)


def test_import_needs_neither_pil_nor_pandas():
    code = ("import sys\n"
            "class Block:\n"
            "    def find_spec(self, name, path=None, target=None):\n"
            "        if name.split('.')[0] in ('PIL', 'pandas'):\n"
            "            raise ImportError(name + ' is hidden')\n"
            "sys.meta_path.insert(0, Block())\n"
            "for k in [k for k in sys.modules if k.split('.')[0] in ('PIL', 'pandas')]:\n"
            "    del sys.modules[k]\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            "import mscs_amd\n"
            "from mscs_amd.datasets import CaDIS, ChainPlanner, planner_for, read_frame_table\n"
            "from mscs_amd.utils.repeat_factor_sampling import RepeatFactorSampler\n"
            "from mscs_amd.managers import HRNetManager\n"
            f"rows = read_frame_table({TABLE!r})\n"
            "RepeatFactorSampler([r for r in rows if r['vid_num'] == '1'], 0.15, 2)\n"
            "assert not any(k.split('.')[0] in ('PIL', 'pandas') for k in sys.modules)\n"
            "print('imported without PIL and pandas')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0 and "imported without PIL and pandas" in r.stdout, r.stderr[-2000:]


# ---- the sampler -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("experiment", (2, 3))
def test_sampler_against_the_reference(experiment):
    g = np.load(os.path.join(GOLDEN, f"cadis_rfs_exp{experiment}.npz"))
    rows = [r for r in _rows() if r["vid_num"] == "1"]                        # split 0's training frames; none is blacklisted
    s = RepeatFactorSampler(rows, 0.15, experiment)
    assert sorted(s.class_repeat_factors) == g["class_ids"].tolist()
    got = np.asarray([s.class_repeat_factors[c] for c in g["class_ids"]], dtype=np.float64)
    assert np.allclose(got, g["class_factors"], rtol=1e-12, atol=0)
    assert s.repeat_factors.dtype == torch.float32 and np.array_equal(s.repeat_factors.numpy(), g["image_factors"])
    for epoch in (0, 1):
        s.set_epoch(epoch)
        assert list(iter(s)) == g[f"epoch{epoch}"].tolist(), epoch
    if experiment == 2:
        assert len(g["image_factors"]) == 177 and int((g["image_factors"] > 1).sum()) == 21 and len(g["epoch0"]) == 189
        assert abs(float(g["image_factors"].max()) - 5.153) < 1e-3
    # a loader asks for the length first: the list it then walks is the one the length drew
    fresh = RepeatFactorSampler(rows, 0.15, experiment)
    assert len(fresh) == len(g["epoch0"]) and list(iter(fresh)) == g["epoch0"].tolist()
    for rank in (0, 1):
        r = RepeatFactorSampler(rows, 0.15, experiment, num_replicas=2, rank=rank)
        r.set_epoch(0)
        assert list(iter(r)) == g[f"w2_rank{rank}"].tolist(), rank
    assert len(g["w2_rank0"]) == len(g["w2_rank1"])


# ---- the manager -------------------------------------------------------------------------------------------------------------------
def _cfg(tmp, tree, **data):
    d = {"dataset": "CADIS", "experiment": 2, "batch_size": 2, "num_workers": 0, "split": 0, "frame_table": TABLE, "blacklist": True,
         "use_relabeled": False, "transforms": ["pad", "flip", "blur", "colorjitter", "torchvision_normalise"], "transforms_val": ["pad"],
         "transform_values": {"blur_p": 1}, "repeat_factor": [1, 2], "repeat_factor_freq_thresh": 0.15}
    d.update(data)
    return {"name": "cadis", "mode": "training", "manager": "HRNet", "cuda": False, "parallel": False, "gpu_device": [0], "seed": 3,
            "data_path": str(tree), "log_every_n_steps": 1000, "log_path": str(tmp), "run_id": "run0", "save_checkpoints": False,
            "graph": {"model": "HRNet", "backbone": "hrnet18", "sync_bn": False, "pretrained": False, "align_corners": True},
            "data": d, "loss": {"name": "LossWrapper", "losses": {"CrossEntropyLoss": 1}},
            "train": {"learning_rate": 0.01, "lr_fct": "polynomial", "optim": "SGD", "lr_batchwise": True, "epochs": 2}}


@pytest.mark.timeout(600)
def test_manager_reads_cadis_and_follows_the_repeat_factor_schedule(tree, tmp_path):
    from mscs_amd.managers import HRNetManager
    set_verbosity(40)
    m = HRNetManager(_cfg(tmp_path, tree), autostart=False)
    m.setup()
    assert m.train_schedule == {0: "train_loader", 1: "train_repeat_factor_loader"}
    train = m.data_loaders["train_loader"].dataset
    assert isinstance(train, R.CaDIS) and len(train) == 177 and len(m.data_loaders["valid_loader"].dataset) == 178
    assert m.data_loaders["train_repeat_factor_loader"].dataset is train
    sampler = m.samplers["train_repeat_factor_loader"]
    assert isinstance(sampler, RepeatFactorSampler) and len(m.data_loaders["train_repeat_factor_loader"]) == 189 // 2
    m.model.train()
    # One training step from each loader, each from the initial weights: at 16 x 16 the coarsest HRNet branch is a 1 x 1 map, its
    # batch norms see two values a channel and the first backward's gradients reach 1e23 (measured), so ANY second step on the
    # updated weights overflows, whichever loader feeds it.  What is checked here is the loaders, not the model at that size.
    import copy
    start = copy.deepcopy(m.model.state_dict()), copy.deepcopy(m.optimiser.state_dict())
    for epoch, key in m.train_schedule.items():
        m.model.load_state_dict(start[0])
        m.optimiser.load_state_dict(start[1])
        if m.samplers.get(key) is not None:
            m.samplers[key].set_epoch(epoch)
        train.set_epoch(epoch)
        batch = next(iter(m.data_loaders[key]))
        x, y, ready = m._upload(*batch[:3])
        assert ready is None and tuple(x.shape) == (2, 3, 16, 16) and tuple(y.shape) == (2, 16, 16) and int(y.max()) <= 17
        assert all([c[0] for c in meta["plan"].chain] == ["pad", "blur", "colour"] for meta in batch[2])
        m.optimiser.zero_grad()
        ret = m.forward_step(x, y, label_ready=ready)
        ret["loss"].backward()
        m.optimiser.step()
        assert np.isfinite(float(ret["loss"].detach())), key
    # the schedule's other forms
    assert _schedule(tmp_path, tree, repeat_factor=[0, 0]) == {0: "train_loader", 1: "train_loader"}
    assert _schedule(tmp_path, tree, repeat_factor=[1]) == {0: "train_loader", 1: "train_repeat_factor_loader"}
    cfg = _cfg(tmp_path, tree)
    del cfg["data"]["repeat_factor"]
    assert _schedule(tmp_path, tree, cfg=cfg) == {0: "train_loader", 1: "train_loader"}
    with pytest.raises(NotImplementedError, match="random_split"):
        _schedule(tmp_path, tree, random_split=[0.8, 0.2])


def _schedule(tmp_path, tree, cfg=None, **data):
    from mscs_amd.managers import HRNetManager
    m = HRNetManager(cfg or _cfg(tmp_path, tree, **data), autostart=False)
    m.setup()
    assert ("train_repeat_factor_loader" in m.data_loaders) == ("train_repeat_factor_loader" in m.train_schedule.values())
    return m.train_schedule
