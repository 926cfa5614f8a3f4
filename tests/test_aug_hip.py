"""The input-augmentation kernels of libdcl_aug.so against the float64 torch composition (datasets/augment.py): image within a bound
recorded on the CPU beforehand, labels and the chosen crop exactly; the switch; reproducibility, also beside a matrix kernel of
another stream; one ``synthetic_raw`` training step of the manager with no host synchronisation in ``_upload``."""
import math

import numpy as np
import pytest
import torch

import _aug_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def leave_no_state():
    """The modules that run after this one find the random streams and the device memory pool as this one found them."""
    state = cases.save_state()
    yield
    cases.restore_state(state)

# max |fp32 composition - float64 composition| over the eight plans of _aug_cases.eight_plans() (sources seeded 7), measured on the
# CPU before any kernel ran; the kernel is allowed four times that, because its summation order differs (the filter's taps row by
# row with FMAs instead of two dense products, m summed in double).  Both numbers are in profiles/aug_time.json.
COMPOSITION_FP32_ERR = 3.944450296500257e-06
KERNEL_BOUND = 4 * COMPOSITION_FP32_ERR
# For plans other than those eight (the crop choice, the drawn batch), where only "the right pixels, the right operations" is asked: a
# worst-case fp32 round-off bound for ANY supported plan: at most 17 x 17 = 289 filter terms and some 20 operations of the colour
# chain, each rounding a value of at most 255 by 2^-24 relative, then / 255 / 0.224: (289 + 20) * 2^-24 / 0.224 = 8.2e-5.  A wrong
# tap or operation moves a pixel by 1 / 255 / 0.229 = 1.7e-2 or more.
ROUNDOFF_BOUND = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_aug
    _lib_aug.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def reference():
    """{name: (img, lbl, plan, float64 composition image, labels, fp32 composition image)} on the CPU, computed once."""
    import mscs_amd  # noqa: F401
    from mscs_amd.datasets import augment as A
    out = {}
    for name, (H, W), plan in cases.eight_plans():
        img, lbl = cases.source(H, W, 7)
        x64, y, _ = A.apply_plan_torch(img, lbl, plan, cases.identity_lut(), torch.float64)
        x32, y32, _ = A.apply_plan_torch(img, lbl, plan, cases.identity_lut(), torch.float32)
        assert torch.equal(y, y32)
        out[name] = (img, lbl, plan, x64, y, x32)
    return out


def test_kernels_against_the_float64_composition(dev, reference, monkeypatch):
    """Labels bitwise equal; image within KERNEL_BOUND = 4 x 3.944e-06 = 1.578e-05 of the float64 composition (the fp32 composition's
    own maximum error over these plans, recorded on the CPU: 3.944e-06; outputs reach |x| = 2.64).  With DCL_AUG_HIP=1 the calls
    counters move; with DCL_AUG_HIP=0 they do not and the result is the composition's."""
    from mscs_amd import _lib_aug as la
    from mscs_amd.datasets import augment as A
    from mscs_amd.debug import cfg as dbg
    live = max(float((r[5].double() - r[3]).abs().max()) for r in reference.values())
    print("fp32 composition against float64, here:", live, " recorded:", COMPOSITION_FP32_ERR)
    aug = A.DeviceAugment(cases.identity_lut())
    monkeypatch.setattr(dbg, "aug_hip", True)
    worst = 0.0
    for name, (img, lbl, plan, x64, y, x32) in reference.items():
        before = dict(la.calls)
        x, yl = aug([img.to(dev)], [lbl.to(dev)], [plan])
        assert aug.last_paths == ["hip"], name
        moved = {k: la.calls[k] - before[k] for k in before}
        assert moved == {"crop_select": 0, "gray_mean": 1 if A.CONTRAST in plan.perm else 0, "apply": 1}, (name, moved)
        assert x.dtype == torch.float32 and tuple(x.shape) == (1, 3, plan.h, plan.w) and yl.dtype == torch.int64
        assert torch.equal(yl[0].cpu(), y), name
        err = float((x[0].cpu().double() - x64).abs().max())
        print(f"{name}: max |kernel - float64 composition| = {err:.3e}  (fp32 composition: {float((x32.double() - x64).abs().max()):.3e})")
        worst = max(worst, err)
    print("worst:", worst, "bound:", KERNEL_BOUND)
    assert worst <= KERNEL_BOUND
    # the switch off: the composition, bitwise, and no kernel call
    monkeypatch.setattr(dbg, "aug_hip", False)
    before = dict(la.calls)
    for name in ("shrink", "pad interior"):
        img, lbl, plan, _, y, _ = reference[name]
        x, yl = aug([img.to(dev)], [lbl.to(dev)], [plan])
        ex, ey, _ = A.apply_plan_torch(img.to(dev), lbl.to(dev), plan, cases.identity_lut().to(dev))
        assert aug.last_paths == ["torch"] and torch.equal(x[0], ex) and torch.equal(yl[0], ey) and torch.equal(ey.cpu(), y)
    assert la.calls == before


def test_gray_mean_against_the_composition(dev, reference):
    """m itself: the kernel sums L in double, so it is compared with the float64 composition's mean at fp32 resolution (m <= 255:
    half an ulp is 2^-17; allowed 2^-15 for the fp32 arithmetic of the operations in front of contrast)."""
    from mscs_amd import _lib_aug as la
    from mscs_amd.datasets import augment as A
    for name in ("shrink", "enlarge", "identity", "pad top-left"):
        img, lbl, plan, _, _, _ = reference[name]
        cp = la.c_plan(plan)
        ws = torch.zeros(la.WS_INTS, dtype=torch.int32, device=dev)
        la.gray_mean(img.to(dev), cp, ws, la.stream_ptr(dev))
        la.gray_mean(img.to(dev), cp, ws, la.stream_ptr(dev))             # the ticket was reset: a second call gives the same
        torch.cuda.synchronize()
        assert int(ws[la.WS_TICKET]) == 0
        m = float(ws[la.WS_MEAN:la.WS_MEAN + 1].view(torch.float32))
        # the composition's m: the chain up to contrast on the chosen crop, in float64
        x = torch.zeros(plan.Hc, plan.Wc, 3, dtype=torch.float64)
        src = img.flip(1) if plan.flip else img
        x[plan.pt:plan.pt + plan.rh, plan.pl:plan.pl + plan.rw] = A.resize_image(src, plan.rh, plan.rw, torch.float64)
        i, j = plan.corners[0]
        x = x[i:i + plan.h, j:j + plan.w]
        for op in plan.perm[:plan.perm.index(A.CONTRAST)]:
            x = {A.BRIGHTNESS: lambda v: A.brightness(v, plan.b), A.SATURATION: lambda v: A.saturation(v, plan.s),
                 A.HUE: lambda v: A.hue(v, plan.delta)}[op](x)
        want = float(A._luma(x).mean())
        print(name, "m", m, "float64", want)
        assert abs(m - want) <= 2.0 ** -15, name


@pytest.mark.parametrize("case", cases.select_cases() + cases.extra_select_cases(), ids=lambda c: c[0])
def test_crop_select_on_constructed_labels(dev, case):
    from mscs_amd import _lib_aug as la
    from mscs_amd.datasets import augment as A
    name, lbl, plan, want = case
    lbl = torch.from_numpy(lbl)
    rng = np.random.default_rng(3)
    img = torch.from_numpy(rng.integers(0, 256, (plan.H, plan.W, 3), dtype=np.uint8))
    ex, ey, chosen = A.apply_plan_torch(img, lbl, plan, cases.identity_lut(), torch.float64)
    assert chosen == want
    aug = A.DeviceAugment(cases.identity_lut())
    before = la.calls["crop_select"]
    x, y = aug([img.to(dev)], [lbl.to(dev)], [plan])                       # the whole pipeline; the verdicts are read back after it
    assert aug.last_paths == ["hip"] and la.calls["crop_select"] - before == (1 if len(plan.corners) > 1 else 0)
    if len(plan.corners) > 1:
        assert aug.chosen(0, plan) == want, name
        # the verdicts and counts of every candidate are the composition's
        ws = aug.last_ws[0].cpu()
        canvas = torch.full((plan.Hc, plan.Wc), plan.ignore, dtype=torch.uint8)
        canvas[plan.pt:plan.pt + plan.rh, plan.pl:plan.pl + plan.rw] = lbl
        for p, (i, j) in enumerate(plan.corners):
            ok, mx, total = A.candidate_verdict(canvas[i:i + plan.h, j:j + plan.w], plan.ignore, plan.max_ratio)
            assert ws[3 * p:3 * p + 3].tolist() == [int(ok), mx, total], (name, p)
    assert torch.equal(y[0].cpu(), ey), name
    assert float((x[0].cpu().double() - ex).abs().max()) <= ROUNDOFF_BOUND, name


def _mixed_batch():
    from mscs_amd.datasets import augment as A
    planner = A.AugmentPlanner(["flip", "random_scale", "RandomCropImgLbl", "colorjitter", "torchvision_normalise"],
                               {"crop_shape": [32, 48], "crop_class_max_ratio": 0.75, "scale_range": [0.5, 2]}, "CITYSCAPES", 1, seed=9)
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
    assert any(len(p.corners) == 10 for p in plans) and all(A.CONTRAST in p.perm for p in plans)
    imgs, lbls = [t.to(dev) for t in imgs], [t.to(dev) for t in lbls]
    aug = A.DeviceAugment(cases.identity_lut())
    x0, y0 = aug(imgs, lbls, plans)
    assert aug.last_paths == ["hip"] * 4
    x1, y1 = aug(imgs, lbls, plans)
    torch.cuda.synchronize()
    assert torch.equal(x0, x1) and torch.equal(y0, y1) and bool(torch.isfinite(x0).all())
    for n, plan in enumerate(plans):                                       # and it is the composition's crop
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
    return {"name": "aug", "mode": "training", "manager": "HRNet", "cuda": True, "parallel": False, "gpu_device": [0], "seed": 3,
            "log_every_n_steps": 1000, "log_path": str(tmp), "run_id": "run0", "save_checkpoints": False,
            "graph": {"model": "HRNet", "backbone": "hrnet18", "sync_bn": False, "pretrained": False, "align_corners": True},
            "data": {"dataset": "CITYSCAPES", "experiment": 1, "batch_size": 2, "num_workers": 0, "synthetic_raw": True,
                     "synthetic_raw_size": [96, 192], "synthetic_length": 2, "synthetic_valid_length": 1,
                     "transforms": ["flip", "random_scale", "RandomCropImgLbl", "colorjitter", "torchvision_normalise"],
                     "transform_values": {"crop_shape": [64, 128], "crop_class_max_ratio": 0.75, "scale_range": [0.5, 2]}},
            "loss": {"name": "LossWrapper", "losses": {"CrossEntropyLoss": 1}},
            "train": {"learning_rate": 0.01, "lr_fct": "polynomial", "optim": "SGD", "lr_batchwise": True, "epochs": 1}}


def test_manager_step_on_synthetic_raw(dev, tmp_path, monkeypatch):
    from mscs_amd import _lib_aug as la
    from mscs_amd.managers import HRNetManager
    from mscs_amd.utils import set_verbosity
    set_verbosity(40)
    m = HRNetManager(_cfg(tmp_path), autostart=False)
    m.setup()
    batch = next(iter(m.data_loaders["train_loader"]))
    order = []
    real_apply, real_record = la.apply, torch.cuda.Event.record
    monkeypatch.setattr(la, "apply", lambda *a, **k: (order.append("apply"), real_apply(*a, **k))[1])
    monkeypatch.setattr(torch.cuda.Event, "record", lambda self, *a, **k: (order.append("record"), real_record(self, *a, **k))[1])

    def no_sync(*a, **k):
        raise AssertionError("torch.cuda.synchronize inside _upload")
    monkeypatch.setattr(torch.cuda, "synchronize", no_sync)
    img, lbl, ready = m._upload(*batch[:3])
    monkeypatch.undo()
    assert order == ["apply", "apply", "record"], order                    # the label-ready event is recorded after the augmentation
    assert ready is not None and m._augment.last_paths == ["hip", "hip"]
    assert img.dtype == torch.float32 and tuple(img.shape) == (2, 3, 64, 128) and lbl.dtype == torch.int64
    m.model.train()
    m.optimiser.zero_grad()
    ret = m.forward_step(img, lbl, label_ready=ready)
    ret["loss"].backward()
    m.optimiser.step()
    torch.cuda.synchronize()
    assert math.isfinite(float(ret["loss"])) and int(lbl.min()) >= 0 and int(lbl.max()) <= 19
