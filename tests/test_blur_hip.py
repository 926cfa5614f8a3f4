"""The kernels of libdcl_blur.so against the float64 torch composition (datasets/augment.py): the blur alone, the reflected rows
bitwise, whole DeviceAugment on eight plans with a chain; the empty chain is the earlier path, bitwise; the switch; reproducibility,
also beside a matrix kernel of another stream; one ``synthetic_raw`` CaDIS step of the manager with no host synchronisation."""
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

import _aug_cases as aug_cases
import _cadis_cases as cases

pytestmark = pytest.mark.gpu

# dbl_blur alone, on the 0..255 scale: six passes, each at most 17 additions and a multiply-add per output (18 roundings of a value
# of at most 255 by 2^-24 relative): 6 x 18 x 2^-24 x 255 = 1.6e-3.  A dropped outer tap moves an impulse by fw x 255 >= 7.5.
BLUR_BOUND = 2e-3
# max |fp32 composition - float64 composition| over the eight plans of _cadis_cases.eight_chain_plans() (sources seeded 7), measured
# on the CPU before any kernel ran; the kernels are allowed four times that (their sums contract into FMAs, m is summed in double).
# Both numbers are in profiles/blur_accuracy.json.
COMPOSITION_FP32_ERR = 1.801819043606434e-06
KERNEL_BOUND = 4 * COMPOSITION_FP32_ERR
# and in any case under the worst-case fp32 round-off of ANY supported plan with a chain: test_aug_hip.ROUNDOFF_BOUND's 289 filter
# terms and 20 colour operations, and the blur's 6 x 17 = 102 terms: (289 + 20 + 102) x 2^-24 / 0.224 = 1.1e-4
ROUNDOFF_BOUND = 1.2e-4


@pytest.fixture(scope="module", autouse=True)
def leave_no_state():
    """The modules that run after this one find the random streams and the device memory pool as this one found them."""
    state = cases.save_state()
    yield
    cases.restore_state(state)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_aug, _lib_blur
    _lib_aug.lib()
    _lib_blur.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def reference():
    """{name: (img, lbl, plan, float64 composition image, labels, chosen, fp32 composition image)} on the CPU, computed once."""
    import mscs_amd  # noqa: F401
    from mscs_amd.datasets import augment as A
    out = {}
    for name, (H, W), plan in cases.eight_chain_plans():
        img, lbl = cases.source(H, W, 7)
        x64, y, chosen = A.apply_plan_torch(img, lbl, plan, cases.identity_lut(), torch.float64)
        x32, y32, _ = A.apply_plan_torch(img, lbl, plan, cases.identity_lut(), torch.float32)
        assert torch.equal(y, y32)
        out[name] = (img, lbl, plan, x64, y, chosen, x32)
    return out


# the row kernel's tile is 4 rows x 256 columns, the column kernel's 64 rows x 64 columns: 131 x 531 is more than twice either
@pytest.mark.parametrize("shape", ((1, 5, 7), (3, 33, 65), (3, 96, 160), (2, 131, 531)), ids=lambda s: "x".join(map(str, s)))
def test_blur_against_the_float64_composition(dev, shape):
    from mscs_amd import _lib_blur as lb
    from mscs_amd.datasets import augment as A
    C, H, W = shape
    if shape == (2, 131, 531):
        assert H > 2 * max(lb.ROW_TILE_H, lb.COL_TILE_H) and W > 2 * max(lb.ROW_TILE_W, lb.COL_TILE_W)
    src = torch.from_numpy(cases.structured(H, W, C, seed=3)).float()              # [H, W, C]
    planes = src.permute(2, 0, 1).contiguous().to(dev)
    for R in (1, 3, 6, 8):
        assert lb.supported(C, H, W, R)
        want = A.gaussian_blur(src.double(), R).permute(2, 0, 1)
        dst = torch.full_like(planes, float("nan"))
        scratch = torch.full_like(planes, float("nan"))
        lb.blur(planes, dst, scratch, R, lb.stream_ptr(dev))
        got = dst.cpu().double()
        assert bool(torch.isfinite(got).all()), (shape, R)
        err = float((got - want).abs().max())
        print(f"{shape} R={R}: max |kernel - float64 composition| = {err:.3e} on the 0..255 scale (bound {BLUR_BOUND})")
        assert err <= BLUR_BOUND, (shape, R)
    assert not lb.supported(C, H, W, 9) and not lb.supported(C, H, W, 0) and not lb.supported(5, H, W, 3)


@pytest.mark.parametrize("pad", ((2, 2), (0, 3)))
def test_pad_rows_is_numpy_reflect(dev, pad):
    from mscs_amd import _lib_blur as lb
    rng = np.random.default_rng(5)
    src = rng.standard_normal((3, 12, 19)).astype(np.float32)
    lbl = rng.integers(0, 2 ** 40, (12, 19), dtype=np.int64)
    top, bottom = pad
    dst = torch.full((3, 12 + top + bottom, 19), float("nan"), device=dev)
    lbl_dst = torch.full((12 + top + bottom, 19), -1, dtype=torch.int64, device=dev)
    lb.pad_rows(torch.from_numpy(src).to(dev), dst, torch.from_numpy(lbl).to(dev), lbl_dst, top, bottom, lb.stream_ptr(dev))
    assert np.array_equal(dst.cpu().numpy(), np.pad(src, ((0, 0), (top, bottom), (0, 0)), mode="reflect"))
    assert np.array_equal(lbl_dst.cpu().numpy(), np.pad(lbl, ((top, bottom), (0, 0)), mode="reflect"))


def test_chain_against_the_float64_composition(dev, reference, monkeypatch):
    """Labels and the chosen crop exact; image within KERNEL_BOUND = 4 x 1.802e-06 = 7.207e-06 of the float64 composition (the fp32
    composition's own maximum error over these plans, recorded on the CPU), and under ROUNDOFF_BOUND = 1.2e-4 in any case."""
    from mscs_amd import _lib_aug as la
    from mscs_amd import _lib_blur as lb
    from mscs_amd.datasets import augment as A
    from mscs_amd.debug import cfg as dbg
    live = max(float((r[6].double() - r[3]).abs().max()) for r in reference.values())
    print("fp32 composition against float64, here:", live, " recorded:", COMPOSITION_FP32_ERR)
    recorded = json.load(open(os.path.join(ROOT, "profiles", "blur_accuracy.json")))
    assert recorded["composition_fp32_max_err"] == COMPOSITION_FP32_ERR and recorded["kernel_bound"] == KERNEL_BOUND
    aug = A.DeviceAugment(cases.identity_lut())
    monkeypatch.setattr(dbg, "aug_hip", True)
    monkeypatch.setattr(dbg, "blur_hip", True)
    worst = 0.0
    for name, (img, lbl, plan, x64, y, chosen, x32) in reference.items():
        before_a, before_b = dict(la.calls), dict(lb.calls)
        x, yl = aug([img.to(dev)], [lbl.to(dev)], [plan])
        assert aug.last_paths == ["hip"], name
        moved = {k: lb.calls[k] - before_b[k] for k in before_b}
        kinds = [item[0] for item in plan.chain]
        assert moved == {"blur": kinds.count("blur"), "pad_rows": kinds.count("pad"), "colour": kinds.count("colour"),
                         "gray_mean": 1 if "colour" in kinds and A.CONTRAST in plan.perm else 0, "from_unit": 1, "normalise": 1}, (name, moved)
        assert {k: la.calls[k] - before_a[k] for k in before_a} == {"crop_select": 1 if len(plan.corners) > 1 else 0, "gray_mean": 0,
                                                                    "apply": 1}, name
        assert x.dtype == torch.float32 and tuple(x.shape) == (1, 3, plan.out_h, plan.out_w) and yl.dtype == torch.int64
        assert tuple(yl.shape) == (1, plan.out_h, plan.out_w) and torch.equal(yl[0].cpu(), y), name
        if len(plan.corners) > 1:
            assert aug.chosen(0, plan) == chosen, name
        err = float((x[0].cpu().double() - x64).abs().max())
        print(f"{name}: max |kernels - float64 composition| = {err:.3e}  (fp32 composition: {float((x32.double() - x64).abs().max()):.3e})")
        worst = max(worst, err)
    print("worst:", worst, "bound:", KERNEL_BOUND)
    assert worst <= ROUNDOFF_BOUND
    assert worst <= KERNEL_BOUND


def test_empty_chain_is_the_earlier_path_and_the_switch(dev, reference, monkeypatch):
    from mscs_amd import _lib_aug as la
    from mscs_amd import _lib_blur as lb
    from mscs_amd.datasets import augment as A
    from mscs_amd.debug import cfg as dbg
    monkeypatch.setattr(dbg, "aug_hip", True)
    monkeypatch.setattr(dbg, "blur_hip", True)
    aug = A.DeviceAugment(cases.identity_lut())
    st = la.stream_ptr(dev)
    for name, (H, W), plan in aug_cases.eight_plans():
        assert plan.chain == ()
        img, lbl = (t.to(dev) for t in aug_cases.source(H, W, 7))
        before_a, before_b = dict(la.calls), dict(lb.calls)
        x, y = aug([img], [lbl], [plan])
        assert {k: la.calls[k] - before_a[k] for k in before_a} == {"crop_select": 0, "gray_mean": 1 if A.CONTRAST in plan.perm else 0,
                                                                    "apply": 1}, name
        assert lb.calls == before_b, name
        # the parent's three launches, issued directly
        cp = la.c_plan(plan)
        ws = torch.zeros(la.WS_INTS, dtype=torch.int32, device=dev)
        ex, ey = torch.empty_like(x[0]), torch.empty_like(y[0])
        if A.CONTRAST in plan.perm:
            la.gray_mean(img, cp, ws, st)
        la.apply(img, lbl, aug._lut_on(dev), cp, ws, ex, ey, st)
        assert torch.equal(x[0], ex) and torch.equal(y[0], ey), name
    # the switch off: a plan with a chain takes the composition, bitwise, and no dbl_* call is made
    monkeypatch.setattr(dbg, "blur_hip", False)
    before_a, before_b = dict(la.calls), dict(lb.calls)
    for name in ("pad blur colour", "colour blur"):
        img, lbl, plan, _, y, _, _ = reference[name]
        x, yl = aug([img.to(dev)], [lbl.to(dev)], [plan])
        ex, ey, _ = A.apply_plan_torch(img.to(dev), lbl.to(dev), plan, cases.identity_lut().to(dev))
        assert aug.last_paths == ["torch"] and torch.equal(x[0], ex) and torch.equal(yl[0], ey) and torch.equal(ey.cpu(), y)
    assert lb.calls == before_b and la.calls == before_a
    # refused by the library (a radius beyond DBL_MAX_RADIUS): the composition as well
    monkeypatch.setattr(dbg, "blur_hip", True)
    from dataclasses import replace
    img, lbl, plan, _, _, _, _ = reference["blur flipped"]
    aug([img.to(dev)], [lbl.to(dev)], [replace(plan, chain=(("blur", 9),))])
    assert aug.last_paths == ["torch"] and lb.calls == before_b


def _mixed_batch():
    from mscs_amd.datasets import augment as A
    planner = A.planner_for(["flip", "random_scale", "RandomCropImgLbl", "blur", "colorjitter", "torchvision_normalise"],
                            {"crop_shape": [32, 48], "crop_class_max_ratio": 0.75, "scale_range": [0.5, 2], "blur_p": 0.5},
                            "CITYSCAPES", 1, seed=9)
    imgs, lbls, plans = [], [], []
    for n, (H, W) in enumerate(((37, 53), (33, 65), (64, 128), (50, 100))):
        img, lbl = cases.source(H, W, 20 + n)
        imgs.append(img)
        lbls.append(lbl)
        plans.append(planner.plan(H, W, 0, n))
    return imgs, lbls, plans


def test_reproducible_and_stable_beside_a_matrix_kernel(dev):
    from mscs_amd.datasets import augment as A
    from mscs_amd.models import ops
    imgs, lbls, plans = _mixed_batch()
    assert any(p.chain for p in plans) and any(not p.chain for p in plans) and all(A.CONTRAST in p.perm for p in plans)
    imgs, lbls = [t.to(dev) for t in imgs], [t.to(dev) for t in lbls]
    aug = A.DeviceAugment(cases.identity_lut())
    x0, y0 = aug(imgs, lbls, plans)
    assert aug.last_paths == ["hip"] * 4
    x1, y1 = aug(imgs, lbls, plans)
    torch.cuda.synchronize()
    assert torch.equal(x0, x1) and torch.equal(y0, y1) and bool(torch.isfinite(x0).all())
    for n, plan in enumerate(plans):
        ex, ey, chosen = A.apply_plan_torch(imgs[n].cpu(), lbls[n].cpu(), plan, cases.identity_lut(), torch.float64)
        assert aug.chosen(n, plan) == chosen and torch.equal(y0[n].cpu(), ey)
        assert float((x0[n].cpu().double() - ex).abs().max()) <= ROUNDOFF_BOUND
    # on a side stream while a GEMM of the main library is busy on another
    lx = torch.randn(16384, 384, device=dev)
    lw = torch.randn(1536, 384, device=dev) * 0.05
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    for _ in range(3):
        with torch.cuda.stream(sb):
            for _ in range(8):
                ops.linear_f16x3(lx, lw)
        outs = []
        with torch.cuda.stream(sa):
            for _ in range(4):
                outs.append(aug(imgs, lbls, plans))
        torch.cuda.synchronize()
        for x, y in outs:
            assert torch.equal(x, x0) and torch.equal(y, y0)


def _cfg(tmp):
    return {"name": "cadis", "mode": "training", "manager": "HRNet", "cuda": True, "parallel": False, "gpu_device": [0], "seed": 3,
            "log_every_n_steps": 1000, "log_path": str(tmp), "run_id": "run0", "save_checkpoints": False,
            "graph": {"model": "HRNet", "backbone": "hrnet18", "sync_bn": False, "pretrained": False, "align_corners": True},
            "data": {"dataset": "CADIS", "experiment": 2, "batch_size": 2, "num_workers": 0, "synthetic_raw": True,
                     "synthetic_raw_size": [60, 96], "synthetic_length": 2, "synthetic_valid_length": 1,
                     "transforms": ["pad", "flip", "blur", "colorjitter", "torchvision_normalise"],
                     "transform_values": {"blur_p": 1}},
            "loss": {"name": "LossWrapper", "losses": {"CrossEntropyLoss": 1}},
            "train": {"learning_rate": 0.01, "lr_fct": "polynomial", "optim": "SGD", "lr_batchwise": True, "epochs": 1}}


def test_manager_step_on_synthetic_cadis(dev, tmp_path, monkeypatch):
    from mscs_amd import _lib_blur as lb
    from mscs_amd.managers import HRNetManager
    from mscs_amd.utils import set_verbosity
    set_verbosity(40)
    m = HRNetManager(_cfg(tmp_path), autostart=False)
    m.setup()
    batch = next(iter(m.data_loaders["train_loader"]))
    assert all([item[0] for item in meta["plan"].chain] == ["pad", "blur", "colour"] for meta in batch[2])
    order = []
    real_norm, real_record = lb.normalise, torch.cuda.Event.record
    monkeypatch.setattr(lb, "normalise", lambda *a, **k: (order.append("normalise"), real_norm(*a, **k))[1])
    monkeypatch.setattr(torch.cuda.Event, "record", lambda self, *a, **k: (order.append("record"), real_record(self, *a, **k))[1])

    def no_sync(*a, **k):
        raise AssertionError("torch.cuda.synchronize inside _upload")
    monkeypatch.setattr(torch.cuda, "synchronize", no_sync)
    img, lbl, ready = m._upload(*batch[:3])
    monkeypatch.undo()
    assert order == ["normalise", "normalise", "record"], order          # the label-ready event follows the last augmentation launch
    assert ready is not None and m._augment.last_paths == ["hip", "hip"]
    assert img.dtype == torch.float32 and tuple(img.shape) == (2, 3, 64, 96) and lbl.dtype == torch.int64
    m.model.train()
    m.optimiser.zero_grad()
    ret = m.forward_step(img, lbl, label_ready=ready)
    ret["loss"].backward()
    m.optimiser.step()
    torch.cuda.synchronize()
    assert math.isfinite(float(ret["loss"].detach())) and int(lbl.min()) >= 0 and int(lbl.max()) <= 17
