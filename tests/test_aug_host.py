"""Host half of the raw input path: the seventh library is built next to the main one, exports and binds exactly what its header
declares and answers the plan test without touching a device; the index rules of csrc/dcl_aug_plan.h agree with a direct Python
restatement in a stand-alone sanitized host program; the torch composition agrees with PIL within derived bounds; the planner's
streams and ranges; the crop choice on constructed labels; the readers on tiny trees; the manager on ``synthetic_raw``."""
import ctypes
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
from mscs_amd import _lib_aug as la                                        # (the feature: this import fails without it)
from mscs_amd.datasets import augment as A
from mscs_amd.datasets import raw as R
from mscs_amd.utils import DATASETS_INFO, set_verbosity

import _aug_cases as cases

@pytest.fixture(scope="module", autouse=True)
def leave_no_state():
    """The modules that run after this one find the global random streams as this one found them (a manager's setup() seeds them)."""
    state = cases.save_state()
    yield
    cases.restore_state(state)


ENTRIES = {"dau_version", "dau_last_error", "dau_supported", "dau_crop_select", "dau_gray_mean", "dau_apply", "dau_plan_taps",
           "dau_plan_nearest"}
GRID = [(1, 1), (2, 1), (1, 7), (53, 27), (33, 131), (100, 27), (37, 19), (8, 1), (5, 40), (64, 64), (65, 33), (27, 53)]


def _header():
    return open(os.path.join(ROOT, "include", "dcl_aug.h")).read()


# ---- library surface ---------------------------------------------------------------------------------------------------------------
def test_seventh_library_is_built_by_the_same_target():
    _lib.build()
    assert os.path.exists(la.LIB_PATH) and os.path.basename(la.LIB_PATH) == "libdcl_aug.so"
    assert os.path.dirname(la.LIB_PATH) == os.path.dirname(_lib.LIB_PATH)
    flags = subprocess.run(["make", "-s", "-C", _lib.CSRC_DIR, "print-cxxflags"], capture_output=True, text=True).stdout
    assert "--offload-arch=gfx950" in flags and "-packed-fp32-ops" in flags
    mk = open(os.path.join(_lib.CSRC_DIR, "Makefile")).read()
    assert "dcl_aug" not in re.search(r"^PACKED = (.*)$", mk, re.M).group(1)           # the generic rule: built with NOPK
    assert re.search(r"^all:.*\$\(OUT_AU\)", mk, re.M)


def test_header_exports_and_bindings_agree():
    _lib.build()
    hdr = _header()
    names = sorted(set(re.findall(r"\b(dau_[a-z0-9_]+)\s*\(", hdr)))
    assert set(names) == ENTRIES
    assert not re.findall(r"\b(dcl|dat|dco|ddc|dtt|dlv)_[a-z0-9_]+\s*\(", hdr), "another library's prefix in this library's header"
    rawlib = ctypes.CDLL(la.LIB_PATH)
    for name in names:
        assert hasattr(rawlib, name), f"{name} declared in include/dcl_aug.h but not exported"
    assert set(la.SIGNATURES) | {"dau_last_error"} == set(names)
    assert not any(n.startswith("dau_") for n in _lib.SIGNATURES)
    L = la.lib()
    assert L.dau_version() >= 1
    for name, sig in la.SIGNATURES.items():
        decl = re.search(rf"\b{name}\s*\(([^;]*)\);", hdr).group(1).strip()
        assert len(sig) == (0 if decl == "void" else decl.count(",") + 1), name
    for macro, value in (("DAU_MAX_CAND", la.MAX_CAND), ("DAU_MAX_TAPS", la.MAX_TAPS), ("DAU_WS_INTS", la.WS_INTS),
                         ("DAU_WS_TICKET", la.WS_TICKET), ("DAU_WS_MEAN", la.WS_MEAN), ("DAU_WS_PART", la.WS_PART),
                         ("DAU_MAX_BLOCKS", la.MAX_BLOCKS)):
        assert int(re.search(rf"#define {macro} (\d+)", hdr).group(1)) == value
    assert la.WS_PART + 2 * la.MAX_BLOCKS <= la.WS_INTS and 3 * la.MAX_CAND <= la.WS_TICKET < la.WS_MEAN < la.WS_PART
    # the struct, field for field: names in order, and the size the C compiler gives it (172 bytes of 4-byte fields, the double
    # aligned to 8)
    body = re.search(r"typedef struct dau_plan \{(.*?)\} dau_plan;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"\[.*", "", f.strip()) for d in body.split(";") if d.strip() for f in d.split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in la.CPlan._fields_]
    assert ctypes.sizeof(la.CPlan) == 184 and la.CPlan.max_ratio.offset == 176


def test_missing_library_error_names_the_build(monkeypatch):
    monkeypatch.setattr(la, "_lib", None)
    monkeypatch.setattr(la, "LIB_PATH", os.path.join(ROOT, "no_such_dir", "libdcl_aug.so"))
    with pytest.raises(RuntimeError) as e:
        la.lib()
    assert "not found" in str(e.value) and "build" in str(e.value)


def test_switch_is_registered_and_defaults_on():
    from mscs_amd.debug import DebugConfig, cfg as dbg
    assert "aug_hip" in DebugConfig.__dataclass_fields__
    assert dbg.aug_hip is True or os.environ.get("DCL_AUG_HIP") == "0"


def _ok(plan):
    return la.supported(la.c_plan(plan))


def test_supported_is_host_arithmetic():
    from dataclasses import replace
    for _, _, plan in cases.eight_plans():
        assert _ok(plan)
    for _, _, plan, _ in cases.select_cases() + cases.extra_select_cases():
        assert _ok(plan)
    cts = A.Plan(H=1024, W=2048, rh=2252, rw=4505, Hc=2252, Wc=4505, pt=0, pl=0, h=512, w=1024, corners=[(7, 9)] * 10, max_ratio=0.75,
                 perm=(0, 1, 2, 3), ignore=19)
    assert _ok(cts)
    assert _ok(replace(cts, rh=128, rw=256, Hc=512, Wc=1024, pt=384, pl=768, corners=[(0, 0)]))           # scale 1/8, padded
    assert not _ok(replace(cts, rh=127, rw=256, Hc=512, Wc=1024, corners=[(0, 0)]))                        # beyond 1/8
    assert _ok(replace(cts, H=64, W=64, rh=512, rw=512, Hc=512, Wc=1024, corners=[(0, 0)]))                # scale 8
    assert not _ok(replace(cts, H=64, W=64, rh=513, rw=512, Hc=513, Wc=1024, corners=[(0, 0)]))
    assert not _ok(replace(cts, h=2253))                                                                    # crop larger than the canvas
    assert not _ok(replace(cts, corners=[(7, 9)] * 11))                                                     # P <= 10
    assert not _ok(replace(cts, corners=[(2252 - 512 + 1, 0)]))                                             # candidate leaves the canvas
    assert not _ok(replace(cts, corners=[(0, 0), (1, 1)], max_ratio=None))                                  # candidates need a ratio
    assert not _ok(replace(cts, pt=1))                                                                      # resized image leaves it
    assert not _ok(replace(cts, perm=(1, 1)))
    assert not _ok(replace(cts, ignore=256))
    # every tensor below 2^31 elements: the source (x 3), the output (x 3), the canvas
    big = A.Plan(H=26754, W=26754, rh=26754, rw=26754, Hc=26754, Wc=26754, pt=0, pl=0, h=8, w=8, ignore=19)
    assert _ok(big) and not _ok(replace(big, H=26755, W=26755, rh=26755, rw=26755, Hc=26755, Wc=26755))      # 3 * 26755^2 > 2^31
    assert not _ok(replace(big, H=8192, W=8192, rh=46341, rw=46341, Hc=46341, Wc=46341))


# ---- the plan header ---------------------------------------------------------------------------------------------------------------
def _taps_restated(S, D, o):
    """the rule of the issue / DESIGN.md, written directly: (k0, [fp32 weights], nearest index)"""
    scale = S / D
    sup = max(scale, 1.0)
    centre = (o + 0.5) * scale
    k0, k1 = max(int(centre - sup + 0.5), 0), min(int(centre + sup + 0.5), S)
    raw = [max(0.0, 1.0 - abs(k + 0.5 - centre) / sup) for k in range(k0, k1)]
    total = 0.0
    for v in raw:
        total += v
    return k0, [np.float32(v / total) for v in raw], ((2 * o + 1) * S) // (2 * D)


def test_plan_exports_agree_with_the_restated_rules():
    for S, D in GRID:
        Wm = A.resize_weights(S, D)
        near = A.nearest_index(S, D)
        for o in range(D):
            k0, w, n = _taps_restated(S, D, o)
            got_k0, got_w = la.plan_taps(S, D, o)
            assert (got_k0, len(got_w)) == (k0, len(w)) and all(np.float32(a) == b for a, b in zip(got_w, w)), (S, D, o)
            assert la.plan_nearest(S, D, o) == n == near[o]
            row = np.zeros(S)
            row[k0:k0 + len(w)] = w
            assert np.array_equal(Wm[o].astype(np.float32), row.astype(np.float32))
            assert abs(sum(float(v) for v in w) - 1.0) < 1e-6
    assert la.lib().dau_plan_nearest(4, 4, 4) < 0 and la.lib().dau_plan_taps(0, 4, 0, 0, None, None) < 0


def test_standalone_plan_program_under_sanitizers(tmp_path):
    table = tmp_path / "taps.txt"
    with open(table, "w") as f:
        for S, D in GRID:
            for o in range(D):
                k0, w, n = _taps_restated(S, D, o)
                f.write(" ".join([str(v) for v in (S, D, o, k0, len(w), n)] + ["%08x" % int(np.float32(v).view(np.uint32)) for v in w]) + "\n")
    gxx = shutil.which("g++") or shutil.which("c++")
    cxx = gxx or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    # the sanitizer runtimes inside the program (clang's default): it runs as it is, whatever else the loader brings along
    static = ["-static-libasan", "-static-libubsan"] if gxx else []
    exe = str(tmp_path / "aug_plan_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static +
                       ["-I", _lib.CSRC_DIR, os.path.join(ROOT, "tests", "aug_plan_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(table)], capture_output=True, text=True)
    assert r.returncode == 0 and "plan ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


# ---- the composition against PIL ---------------------------------------------------------------------------------------------------
TARGETS = [(19, 27), (74, 106), (40, 61), (91, 77), (25, 50), (100, 200), (23, 131)]


def test_image_resize_against_pil():
    """Bound 1.01 grey levels.  PIL resamples the two axes one after the other and rounds to uint8 after each: the first rounding
    moves an intermediate value by at most 0.5, the second axis' weights are non-negative and sum to 1, so that error reaches the
    result as at most 0.5, and the final rounding adds at most 0.5: 1.0 between PIL and the exact value rounded to the nearest level
    -- plus PIL's coefficients, fixed point with 22 fractional bits (each off by <= 2^-23, up to 17 taps of <= 255 per axis:
    < 0.002 levels) and the fp32 rounding of this arithmetic's weights (2^-24 relative: < 0.0001 levels).  Measured maximum: 1.0."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(11)
    worst = 0.0
    for H, W in ((37, 53), (64, 128), (33, 65), (50, 100)):
        src = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        for th, tw in TARGETS + [(H, W)]:
            ref = np.asarray(Image.fromarray(src).resize((tw, th), Image.BILINEAR)).astype(np.float64)
            got = A.resize_image(torch.from_numpy(src), th, tw, torch.float64).numpy()
            worst = max(worst, float(np.abs(np.floor(got + 0.5) - ref).max()))
    print("max |round(composition) - PIL| in grey levels:", worst)
    assert worst <= 1.01


def test_label_resize_against_pil():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(12)
    for H, W in ((37, 53), (33, 65)):
        lbl = rng.integers(0, 256, (H, W), dtype=np.uint8)
        for th, tw in TARGETS:
            # PIL accumulates a double and lands one lower exactly where (2 o + 1) S is a multiple of 2 D: those rows / columns
            # would be excluded -- and there are none in this set, so nothing is
            rows = [o for o in range(th) if ((2 * o + 1) * H) % (2 * th) == 0]
            cols = [o for o in range(tw) if ((2 * o + 1) * W) % (2 * tw) == 0]
            assert rows == [] and cols == [], (H, W, th, tw)
            ref = np.asarray(Image.fromarray(lbl).resize((tw, th), Image.NEAREST))
            got = A.resize_label(torch.from_numpy(lbl), th, tw).numpy()
            assert np.array_equal(got, ref), (H, W, th, tw)
    # the stated deviation, where the set is not empty: 100 -> 27 differs at column 13 only
    lbl = rng.integers(0, 256, (53, 100), dtype=np.uint8)
    ref = np.asarray(Image.fromarray(lbl).resize((27, 27), Image.NEAREST))
    got = A.resize_label(torch.from_numpy(lbl), 27, 27).numpy()
    cols = [o for o in range(27) if ((2 * o + 1) * 100) % 54 == 0]
    assert cols == [13] and np.array_equal(np.delete(got, cols, axis=1), np.delete(ref, cols, axis=1))


@pytest.mark.parametrize("factor", (2 / 3, 0.81, 1.0, 1.27, 1.5))
def test_colour_operations_against_pil_enhancers(factor):
    """Bound 1.01 levels each, on the composition rounded to the nearest level (as for the resize).  ImageEnhance blends two uint8
    images, p = uint8(deg + factor (img - deg)), one conversion at the end that truncates: p is within 1 level of the exact value of
    that expression.  What differs from the composition is deg.  Brightness: deg = 0, nothing differs.  Saturation: deg is PIL's L
    image, integer weights (19595, 38470, 7471) / 65536 and rounded: within 0.5 + 0.002 of L; it enters with |1 - factor| <= 0.5:
    0.26.  Contrast: deg is PIL's mean, an integer (0.5) of rounded L values (0.5); times |1 - factor|: 0.5.  So the exact value x
    and PIL's p differ by less than 1.5, round(x) and p by less than 2, and both are integers: at most 1 level.  1.01 leaves room
    for nothing but float64 round-off at a rounding boundary.  The unrounded difference is printed next to it."""
    Image = pytest.importorskip("PIL.Image")
    ImageEnhance = pytest.importorskip("PIL.ImageEnhance")
    rng = np.random.default_rng(13)
    src = rng.integers(0, 256, (33, 65, 3), dtype=np.uint8)
    src[:, :20] = (src[:, :20].astype(np.int32) * 40 // 255 + 100).astype(np.uint8)          # a low-contrast part
    pil = Image.fromarray(src)
    x = torch.from_numpy(src).to(torch.float64)
    for name, enh, mine in (("brightness", ImageEnhance.Brightness, A.brightness), ("contrast", ImageEnhance.Contrast, A.contrast),
                            ("saturation", ImageEnhance.Color, A.saturation)):
        ref = np.asarray(enh(pil).enhance(factor)).astype(np.float64)
        got = mine(x, factor).numpy()
        err = float(np.abs(np.floor(got + 0.5) - ref).max())
        print(name, factor, "max |round(composition) - PIL|:", err, " unrounded:", float(np.abs(got - ref).max()))
        assert err <= 1.01, name


def test_hue_is_a_rotation():
    rng = np.random.default_rng(14)
    x = torch.from_numpy(rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)).to(torch.float64)
    x[0, 0] = 0
    x[0, 1] = 255
    x[0, 2] = torch.tensor([17.0, 17.0, 17.0])                                          # grey: no hue
    assert torch.allclose(A.hue(x, 0.0), x, atol=1e-9) and torch.allclose(A.hue(x, 1.0), x, atol=1e-9)
    assert torch.allclose(A.hue(A.hue(x, 0.05), -0.05), x, atol=1e-9)
    y = A.hue(x, 1 / 3)                                                                 # a third of a turn: R -> G -> B -> R
    assert torch.allclose(y, x[..., [2, 0, 1]], atol=1e-9)
    assert torch.equal(y.max(-1).values, x.max(-1).values)


# ---- the planner -------------------------------------------------------------------------------------------------------------------
TRAIN = ["flip", "random_scale", "RandomCropImgLbl", "colorjitter", "torchvision_normalise"]
VALUES = {"crop_shape": [512, 1024], "crop_class_max_ratio": 0.75, "scale_range": [0.5, 2]}


def test_planner_streams():
    pl = A.AugmentPlanner(TRAIN, VALUES, "CITYSCAPES", 1, seed=5)
    a = pl.plan(1024, 2048, epoch=3, index=17)
    other = [pl.plan(1024, 2048, epoch=e, index=i) for e in (0, 3) for i in (0, 16, 18)]       # calls in between
    assert pl.plan(1024, 2048, epoch=3, index=17) == a
    assert A.AugmentPlanner(TRAIN, VALUES, "CITYSCAPES", 1, seed=5).plan(1024, 2048, 3, 17) == a
    assert all(o != a for o in other) and pl.plan(1024, 2048, 4, 17) != a
    assert A.AugmentPlanner(TRAIN, VALUES, "CITYSCAPES", 1, seed=6).plan(1024, 2048, 3, 17) != a
    # the reference's three shipped configs parse
    import json
    for name in sorted(os.listdir(os.path.join(ROOT, "tests", "golden", "reference_configs"))):
        d = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_configs", name)))["data"]
        p = A.AugmentPlanner(d["transforms"], d["transform_values"], d["dataset"], d["experiment"], 0).plan(600, 800, 0, 0)
        assert (p.h, p.w) == tuple(d["transform_values"]["crop_shape"]) and p.normalise
        A.AugmentPlanner(d["transforms_val"], d["transform_values_val"], d["dataset"], d["experiment"], 0)


def test_planner_ranges_over_2000_draws():
    pl = A.AugmentPlanner(TRAIN, dict(VALUES, p_random_scale=0.8), "CITYSCAPES", 1, seed=1)
    H, W = 1024, 2048
    flips = unscaled = 0
    for i in range(2000):
        p = pl.plan(H, W, 0, i)
        flips += p.flip
        assert (p.h, p.w) == (512, 1024) and len(p.corners) in (1, 10) and p.max_ratio == 0.75 and p.ignore == 19 and p.normalise
        if (p.rh, p.rw) == (H, W):
            unscaled += 1
            assert (p.Hc, p.Wc, p.pt, p.pl) == (H, W, 0, 0)
        else:
            # w_ratio = sqrt(a) s, h_ratio = sqrt(1 / a) s with s in [0.5, 2], a in [0.9, 1.1]; int() truncates
            s2 = ((p.rw + 1) / W) * ((p.rh + 1) / H)
            assert p.rw / W * (p.rh / H) <= 4.0 and s2 >= 0.25
            assert 0.9 * 0.999 <= (p.rw / W) / ((p.rh + 1) / H) and (p.rw + 1) / W / (p.rh / H) >= 0.9 and (p.rw / W) / ((p.rh + 1) / H) <= 1.1
        assert (p.Hc, p.Wc) == (max(p.rh, 512), max(p.rw, 1024))
        assert 0 <= p.pt <= p.Hc - p.rh and 0 <= p.pl <= p.Wc - p.rw                    # pad offsets inside the slack
        for ci, cj in p.corners:
            assert 0 <= ci <= p.Hc - p.h and 0 <= cj <= p.Wc - p.w                      # the crop stays inside the canvas
        if (p.Hc, p.Wc) == (p.h, p.w):
            assert p.corners == [(0, 0)]
        assert sorted(p.perm) == [0, 1, 2, 3]
        assert all(2 / 3 <= v <= 1.5 for v in (p.b, p.c, p.s)) and -0.05 <= p.delta <= 0.05
        assert la.supported(la.c_plan(p))
    assert abs(flips / 2000 - 0.5) <= 0.05
    assert abs(unscaled / 2000 - 0.2) <= 0.05
    # pad offsets and corners reach both ends of their ranges on a small image
    small = A.AugmentPlanner(TRAIN, {"crop_shape": [32, 48], "crop_class_max_ratio": 0.75, "scale_range": [0.5, 0.6]}, "CITYSCAPES", 1, 2)
    pts = {small.plan(40, 60, 0, i).pt for i in range(300)}
    assert min(pts) == 0 and max(pts) >= 32 - int(40 * 0.6 * 1.06) and all(small.plan(40, 60, 0, i).corners == [(0, 0)] for i in range(20))
    # pseudo_colorjitter: strength and probability keys
    ps = A.AugmentPlanner(["pseudo_colorjitter"], {"colorjitter_strength": 1, "p_colorjitter": 0.3}, "CITYSCAPES", 1, 3)
    plans = [ps.plan(64, 64, 0, i) for i in range(2000)]
    on = [p for p in plans if p.perm]
    assert abs(len(on) / 2000 - 0.3) <= 0.05 and all(0.75 <= v <= 1.25 for p in on for v in (p.b, p.c, p.s))
    assert all(-0.02 <= p.delta <= 0.02 for p in on) and all((p.h, p.w, p.rh, p.rw) == (64, 64, 64, 64) and not p.normalise for p in plans)
    # no ratio configured: one candidate
    one = A.AugmentPlanner(["RandomCropImgLbl"], {"crop_shape": [16, 16]}, "CITYSCAPES", 1, 0).plan(64, 64, 0, 0)
    assert len(one.corners) == 1 and one.max_ratio is None and one.perm == () and not one.flip


def test_planner_validation_geometry():
    ident = A.AugmentPlanner(["torchvision_normalise"], {}, "CITYSCAPES", 1, 0).plan(1024, 2048, 0, 0)
    assert (ident.rh, ident.rw, ident.Hc, ident.Wc, ident.h, ident.w) == (1024, 2048) * 3 and ident.corners == [(0, 0)]
    assert not ident.flip and ident.perm == () and ident.normalise and (ident.pt, ident.pl) == (0, 0)
    rv = A.AugmentPlanner(["resize_val", "torchvision_normalise"], {"min_side_length": 512, "fit_stride_val": 32}, "ADE20K", 1, 0)
    for H, W in ((683, 512), (256, 341), (300, 401), (512, 512)):
        p = rv.plan(H, W, 0, 0)
        ratio = 512 / min(H, W)
        assert (p.rw, p.rh) == (int(round(W * ratio)), int(round(H * ratio))) and min(p.rw, p.rh) == 512
        assert p.Hc % 32 == 0 and p.Wc % 32 == 0 and 0 <= p.Hc - p.rh < 32 and 0 <= p.Wc - p.rw < 32
        assert (p.pt, p.pl, p.h, p.w) == (0, 0, p.Hc, p.Wc) and p.ignore == 150


@pytest.mark.parametrize("key", ("blur", "pad", "resize", "no_such_transform"))
def test_unsupported_keys_raise_naming_the_key(key):
    with pytest.raises(ValueError, match=key):
        A.AugmentPlanner(["flip", key], VALUES, "CITYSCAPES", 1, 0)


# ---- the crop choice ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.select_cases(), ids=lambda c: c[0])
def test_crop_choice_on_constructed_labels(case):
    name, lbl, plan, want = case
    img = torch.zeros(plan.H, plan.W, 3, dtype=torch.uint8)
    x, y, chosen = A.apply_plan_torch(img, torch.from_numpy(lbl), plan, cases.identity_lut())
    assert chosen == want, name
    i, j = plan.corners[chosen]
    assert np.array_equal(y.numpy(), lbl[i:i + plan.h, j:j + plan.w]) and y.dtype == torch.int64
    if name == "canvas equals crop":
        assert plan.corners[chosen] == (0, 0)
    if name == "ratio exactly at the threshold":
        assert A.candidate_verdict(torch.from_numpy(lbl[:, :2]), plan.ignore, 0.75) == (False, 3, 4)
        assert A.candidate_verdict(torch.from_numpy(lbl[:, :2]), plan.ignore, 0.7500001)[0]


# ---- the readers -------------------------------------------------------------------------------------------------------------------
def _write_trees(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(21)
    cts = tmp_path / "cts"
    for split in ("train", "val"):
        for city in ("aachen", "bonn"):
            (cts / "leftImg8bit" / split / city).mkdir(parents=True)
            (cts / "gtFine" / split / city).mkdir(parents=True)
            for n in range(2):
                stem = f"{city}_{n:06d}_000019"
                Image.fromarray(rng.integers(0, 256, (24, 32, 3), dtype=np.uint8)).save(cts / "leftImg8bit" / split / city / f"{stem}_leftImg8bit.png")
                Image.fromarray(rng.integers(0, 34, (24, 32), dtype=np.uint8)).save(cts / "gtFine" / split / city / f"{stem}_gtFine_labelIds.png")
                Image.fromarray(rng.integers(0, 34, (24, 32), dtype=np.uint8)).save(cts / "gtFine" / split / city / f"{stem}_gtFine_instanceIds.png")
    ade = tmp_path / "ade"
    for split in ("training", "validation"):
        (ade / "ADEChallengeData2016" / "images" / split).mkdir(parents=True)
        (ade / "ADEChallengeData2016" / "annotations" / split).mkdir(parents=True)
        for n in range(4):
            stem = f"ADE_{split[:5]}_{n:08d}"
            Image.fromarray(rng.integers(0, 256, (24, 32, 3), dtype=np.uint8)).save(ade / "ADEChallengeData2016" / "images" / split / f"{stem}.jpg")
            Image.fromarray(rng.integers(0, 151, (24, 32), dtype=np.uint8)).save(ade / "ADEChallengeData2016" / "annotations" / split / f"{stem}.png")
    return str(cts), str(ade)


def test_readers_pair_files_and_return_raw_tensors(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    cts, ade = _write_trees(tmp_path)
    planner = A.AugmentPlanner(["flip", "RandomCropImgLbl"], {"crop_shape": [16, 16]}, "CITYSCAPES", 1, 0)
    for split, n in (("train", 4), ("val", 4), (["train", "val"], 8)):
        ds = R.Cityscapes(cts, split, planner)
        assert len(ds) == n
        for im, tg in zip(ds.images, ds.targets):
            assert os.path.basename(im).replace("_leftImg8bit.png", "") == os.path.basename(tg).replace("_gtFine_labelIds.png", "")
            assert os.path.basename(os.path.dirname(im)) == os.path.basename(os.path.dirname(tg))         # same city
            assert im.split(os.sep)[-3] == tg.split(os.sep)[-3]                                           # same split
    ds.set_epoch(2)
    img, lbl, meta = ds[5]
    assert img.dtype == torch.uint8 and tuple(img.shape) == (24, 32, 3) and lbl.dtype == torch.uint8 and tuple(lbl.shape) == (24, 32)
    assert np.array_equal(img.numpy(), np.asarray(Image.open(ds.images[5]).convert("RGB")))
    assert np.array_equal(lbl.numpy(), np.asarray(Image.open(ds.targets[5])))
    assert meta["index"] == 5 and meta["plan"] == planner.plan(24, 32, 2, 5) and (meta["plan"].h, meta["plan"].w) == (16, 16)
    ds = R.ADE20K(ade, "train", None)
    assert len(ds) == 4 and len(R.ADE20K(ade, "validation")) == 4
    for im, tg in zip(ds.images, ds.targets):
        assert os.path.splitext(os.path.basename(im))[0] == os.path.splitext(os.path.basename(tg))[0] and "training" in im and "training" in tg
    img, lbl, meta = ds[1]
    assert img.dtype == torch.uint8 and tuple(img.shape) == (24, 32, 3) and tuple(lbl.shape) == (24, 32) and "plan" not in meta
    # the list collate keeps images of different sizes apart
    a = (torch.zeros(4, 5, 3, dtype=torch.uint8), torch.zeros(4, 5, dtype=torch.uint8), {"index": 0})
    b = (torch.zeros(6, 7, 3, dtype=torch.uint8), torch.zeros(6, 7, dtype=torch.uint8), {"index": 1})
    imgs, lbls, metas = R.list_collate([a, b])
    assert [tuple(t.shape) for t in imgs] == [(4, 5, 3), (6, 7, 3)] and [m["index"] for m in metas] == [0, 1] and len(lbls) == 2


def test_lookup_tables_restate_remap_mask():
    for ds, checks in (("CITYSCAPES", {7: 0, 0: 19, 33: 18, 8: 1, 255: 19, 34: 19}), ("ADE20K", {0: 150, 1: 0, 150: 149, 77: 76, 200: 150})):
        lut = A.network_lut(ds, 1)
        assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256,)
        # remap_mask(..., to_network=True), restated: every id listed under a key maps to the key, everything else -- and the
        # key 255 -- to len(remapping) - 1
        remap = DATASETS_INFO[ds].CLASS_INFO[1][0]
        want = np.full(256, len(remap) - 1, dtype=np.int64)
        for key, ids in remap.items():
            for v in ids:
                if 0 <= v < 256 and key != 255:
                    want[v] = key
        assert np.array_equal(lut.numpy().astype(np.int64), want), ds
        for raw_id, net in checks.items():
            assert int(lut[raw_id]) == net, (ds, raw_id)
        assert A.ignore_id(ds, 1) == len(remap) - 1
    assert all(int(A.network_lut("ADE20K", 1)[k]) == k - 1 for k in range(1, 151))


def test_import_does_not_need_pil():
    code = ("import sys\n"
            "class Block:\n"
            "    def find_spec(self, name, path=None, target=None):\n"
            "        if name == 'PIL' or name.startswith('PIL.'):\n"
            "            raise ImportError('PIL is hidden')\n"
            "sys.meta_path.insert(0, Block())\n"
            "for k in [k for k in sys.modules if k == 'PIL' or k.startswith('PIL.')]:\n"
            "    del sys.modules[k]\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            "import mscs_amd\n"
            "from mscs_amd.datasets import Cityscapes, ADE20K, SyntheticRaw, AugmentPlanner, DeviceAugment\n"
            "from mscs_amd.managers import HRNetManager\n"
            "assert not any(k == 'PIL' or k.startswith('PIL.') for k in sys.modules)\n"
            "print('imported without PIL')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0 and "imported without PIL" in r.stdout, r.stderr[-2000:]


# ---- the manager -------------------------------------------------------------------------------------------------------------------
def _cfg(tmp, **data):
    d = {"dataset": "CITYSCAPES", "experiment": 1, "batch_size": 2, "num_workers": 0, "synthetic": True, "synthetic_length": 4,
         "synthetic_valid_length": 2, "synthetic_mode": "blocky", "transform_values": {"crop_shape": [32, 64]}}
    d.update(data)
    return {"name": "aug", "mode": "training", "manager": "HRNet", "cuda": False, "parallel": False, "gpu_device": [0], "seed": 3,
            "log_every_n_steps": 1000, "log_path": str(tmp), "run_id": "run0", "save_checkpoints": False,
            "graph": {"model": "HRNet", "backbone": "hrnet18", "sync_bn": False, "pretrained": False, "align_corners": True},
            "data": d, "loss": {"name": "LossWrapper", "losses": {"CrossEntropyLoss": 1}},
            "train": {"learning_rate": 0.01, "lr_fct": "polynomial", "optim": "SGD", "lr_batchwise": True, "epochs": 1}}


RAW = {"synthetic_raw": True, "synthetic_raw_size": [48, 96], "transforms": TRAIN,
       "transform_values": {"crop_shape": [32, 64], "crop_class_max_ratio": 0.75, "scale_range": [0.5, 2]}}


@pytest.mark.timeout(600)
def test_manager_trains_on_synthetic_raw(tmp_path):
    from mscs_amd.managers import HRNetManager
    set_verbosity(40)
    m = HRNetManager(_cfg(tmp_path, **RAW), autostart=False)
    m.setup()
    ds = m.data_loaders["train_loader"].dataset
    assert isinstance(ds, R.SyntheticRaw) and len(ds) == 4
    img, lbl, meta = ds[0]
    assert img.dtype == torch.uint8 and tuple(img.shape) == (48, 96, 3) and tuple(lbl.shape) == (48, 96)
    assert set(np.unique(lbl.numpy())) <= set(np.nonzero(A.network_lut("CITYSCAPES", 1).numpy() < 19)[0]) | {0}     # raw ids
    batch = next(iter(m.data_loaders["train_loader"]))
    x, y, ready = m._upload(*batch[:3])
    assert ready is None and x.dtype == torch.float32 and tuple(x.shape) == (2, 3, 32, 64)
    assert y.dtype == torch.int64 and tuple(y.shape) == (2, 32, 64) and int(y.min()) >= 0 and int(y.max()) <= 19
    assert bool(torch.isfinite(x).all()) and m._augment.last_paths == ["torch", "torch"]
    for n, meta in enumerate(batch[2]):                     # the batch IS the composition of each sample's plan
        ex, ey, _ = A.apply_plan_torch(batch[0][n], batch[1][n], meta["plan"], A.network_lut("CITYSCAPES", 1))
        assert torch.equal(ex, x[n]) and torch.equal(ey, y[n])
    before = [p.detach().clone() for p in m.model.parameters()][:3]
    m.train_one_epoch()                                     # 4 samples, batch 2: two training steps
    assert m.global_step == 2 and np.isfinite(m.metrics["loss"])
    assert any(not torch.equal(a, b) for a, b in zip(before, list(m.model.parameters())[:3]))
    miou = m.validate()                                     # identity plan: validation images at the raw size
    assert 0.0 <= miou <= 1.0


def test_manager_synthetic_path_is_unchanged_and_errors_name_their_key(tmp_path):
    from mscs_amd.datasets import SyntheticSegmentation
    from mscs_amd.managers import HRNetManager
    set_verbosity(40)
    m = HRNetManager(_cfg(tmp_path), autostart=False)
    m.setup()
    for key, length, seed in (("train_loader", 4, 3), ("valid_loader", 2, 4)):
        ds = m.data_loaders[key].dataset
        assert type(ds) is SyntheticSegmentation and len(ds) == length
        want = SyntheticSegmentation(length, [32, 64], 20, mode="blocky", seed=seed)[0]
        got = ds[0]
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2] == want[2]
    assert not hasattr(m, "_augment")
    cfg = _cfg(tmp_path)
    cfg["data"]["synthetic"] = False
    with pytest.raises(KeyError, match="data_path"):
        HRNetManager(cfg, autostart=False).setup()
    cfg = _cfg(tmp_path, **dict(RAW, transforms_val=["resize_val", "torchvision_normalise"],
                                transform_values_val={"min_side_length": 64, "fit_stride_val": 32}))
    m = HRNetManager(cfg, autostart=False)
    m.setup()
    with pytest.raises(NotImplementedError, match="original-label"):
        m.validate()
