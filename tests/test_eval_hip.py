"""Evaluation at the original label size on the GPU (include/dcl_eval.h, utils/evaluate.py): dve_evaluate against the arg-max of the
float64 evaluation of the same two resizes (computed in torch on the CPU, tests/_eval_cases.py), exact against torch.argmax where
both stages are the identity, the confusion matrix against bincount of the kernel's own arg-max, the outputs that were not asked
for, independence of the padded part of the logits, run-to-run equality, the memory bound, the manager.

The comparison leaves a pixel out only when the float64 top-two margin is below 2e-5 * max|z| (tests/_pred_cases.py's margin
doubled: two resizes stack twice the roundings), and at most 1 % of a case's pixels may be left out: a condition, not a tolerance."""
import os

import pytest
import torch
import torch.nn.functional as F

import _eval_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_eval
    _lib_eval.lib()
    return torch.device("cuda:0")


def _dataset(C):
    return "ADE20K" if C == 150 else "CITYSCAPES"


def _cols(C):
    return C + 1 if C in (19, 150) else C


def _check(ids, ref, ok, what):
    ids = ids.cpu().long()
    left_out = float((~ok).float().mean())
    wrong = int((ids[ok] != ref[ok]).sum())
    print(what, "left out:", int((~ok).sum()), "of", ok.numel(), "wrong among the rest:", wrong)
    assert left_out <= cases.MAX_LEFT_OUT, what
    assert wrong == 0, what


def _raw(dev, z, case, label=None, lut=None, cols=None, cm=None, oob=None, ids=None):
    """dve_evaluate as it is, on the case's geometry"""
    from mscs_amd import _lib_eval as le
    C, h, w, a1, Hp, Wp, rh, rw, H0, W0, a2 = case
    p = lambda t: None if t is None else t.data_ptr()                                   # noqa: E731
    return le.lib().dve_evaluate(z.data_ptr(), C, h or Hp, w or Wp, Hp, Wp, a1, rh, rw, H0, W0, a2, p(label),
                                 label.element_size() if label is not None else 0, p(lut), cols or _cols(C), p(cm), p(oob), p(ids),
                                 le.stream_ptr(dev))


FORMS = [(case, form) for case in cases.CASES for form in (("given", "dense") if case[1] else ("given",))]


@pytest.mark.parametrize("case,form", FORMS, ids=lambda v: v if isinstance(v, str) else cases.case_id(v))
def test_evaluate_against_float64(dev, case, form):
    """Each case as it is (the lazy cases read the low-resolution map) and with its stage 1 already applied (the dense form)."""
    from mscs_amd import _lib_eval as le
    from mscs_amd.utils import evaluate_at_original
    C, h, w, a1, Hp, Wp, rh, rw, H0, W0, a2 = case
    z, ref, ok = cases.reference(case)
    if form == "dense":
        z = F.interpolate(z, size=(Hp, Wp), mode="bilinear", align_corners=bool(a1))
        out = z.to(dev)
    else:
        out = cases.wrap(z.to(dev), case)
    t = cases.target(case, hi=_cols(C)).to(dev)
    before = le.calls["evaluate"]
    cm, ids = evaluate_at_original(out, t, (rh, rw), (H0, W0), bool(a2), _dataset(C), return_ids=True)
    assert le.calls["evaluate"] == before + 1
    assert ids.dtype == torch.uint8 and tuple(ids.shape) == (1, H0, W0) and cm.dtype == torch.int32 and tuple(cm.shape) == (C, C)
    _check(ids, ref, ok, (case, form))
    want, _ = cases.bincount_cm(ids, t, C, _cols(C))
    assert torch.equal(cm.cpu().long(), want[:, :C])
    again = evaluate_at_original(out, t, (rh, rw), (H0, W0), bool(a2), _dataset(C), return_ids=True)
    assert torch.equal(again[0], cm) and torch.equal(again[1], ids)                    # bitwise the same from run to run


def test_identity_is_torch_argmax(dev):
    from mscs_amd.utils import evaluate_at_original
    case = cases.IDENTITY
    C, H, W = case[0], case[8], case[9]
    z = cases.logits(case)
    twin = z.clone()
    twin[:, 7] = twin[:, 3]                                    # two identical class planes: the lower index wins
    twin[:, 3] += 100.0
    twin[:, 7] += 100.0
    nans = z.clone()
    g = torch.Generator().manual_seed(4)
    nans.view(-1)[torch.randperm(nans.numel(), generator=g)[:400]] = float("nan")
    nans[0, :, 0, 0] = float("nan")                            # every class a NaN: the first one
    infs = z.clone()
    infs.view(-1)[torch.randperm(infs.numel(), generator=g)[:400]] = float("inf")     # 0 * Inf would be a NaN: nothing is multiplied
    t = cases.target(case).to(dev)
    for name, v in (("random", z), ("twin planes", twin), ("NaNs", nans), ("Infs", infs)):
        for view in (v, v[:, :, :, :21].contiguous(), v[:, :, :, 1:].contiguous()):     # row lengths of 24, 21 and 23
            Wv = view.shape[3]
            _, ids = evaluate_at_original(view.to(dev), t[:, :Wv].contiguous(), (H, Wv), (H, Wv), False, "CITYSCAPES", return_ids=True)
            assert torch.equal(ids.cpu().long(), view.argmax(1)), name
    # the twin planes through the interpolating path: 8 x 12 -> 32 x 48, the whole map kept, stage 2 the identity
    _, ids = evaluate_at_original(cases.wrap(twin[:, :, :8, :12].contiguous().to(dev), (C, 8, 12, 0, 32, 48)), cases.target(
        (C, 0, 0, 0, 0, 0, 0, 0, 32, 48)).to(dev), (32, 48), (32, 48), False, "CITYSCAPES", return_ids=True)
    assert bool((ids == 3).all())


@pytest.mark.parametrize("kind", ("u8lut", "i32", "i64"))
@pytest.mark.parametrize("case", (cases.CASES[1], cases.CASES[3], cases.CASES[0], cases.CASES[5]), ids=cases.case_id)
def test_confusion_matrix_is_bincount_of_the_kernels_ids(dev, case, kind):
    """C = 19: the LDS histogram; C = 256 and C = 150: global atomics (dve_plan_hist_in_lds).  Targets equal to C (the ignore
    column, sliced off), above it and negative are counted in oob; the matrix is added to."""
    from mscs_amd import _lib_eval as le
    C, H0, W0 = case[0], case[8], case[9]
    cols = _cols(C)
    assert le.plan_hist_in_lds(C, cols) == (C == 19)
    z = cases.logits(case).to(dev)
    g = torch.Generator().manual_seed(11)
    t = torch.randint(0, cols, (H0, W0), generator=g)
    lut = None
    if kind == "u8lut":
        table = cases.lut()                                    # random bytes: entries >= cols are out of range
        raw = torch.randint(0, 256, (H0, W0), generator=g, dtype=torch.uint8)
        t = table[raw.long()].long()
        label, lut = raw.to(dev), table.to(dev)
    else:
        t.view(-1)[:5] = torch.tensor([cols, cols + 7, -1, -300, 2 ** 31 - 1])[:5]
        if kind == "i64":
            t.view(-1)[5:7] = torch.tensor([2 ** 40, -2 ** 40])
        label = t.to(torch.int32 if kind == "i32" else torch.int64).to(dev)
    prior = torch.randint(0, 9, (C, cols), generator=g, dtype=torch.int32)
    cm, oob = prior.to(dev), torch.full((1,), 5, dtype=torch.int32, device=dev)
    ids = torch.empty(H0, W0, dtype=torch.uint8, device=dev)
    le.check(_raw(dev, z, case, label=label, lut=lut, cm=cm, oob=oob, ids=ids), "dve_evaluate")
    want, bad = cases.bincount_cm(ids, t, C, cols)
    assert torch.equal(cm.cpu().long(), want + prior.long())                           # added to, not overwritten
    assert int(oob.item()) == 5 + bad and (bad > 0 or kind == "u8lut")
    # cm alone: the same counts, and nothing else is written
    cm2, oob2 = torch.zeros_like(cm), torch.zeros_like(oob)
    le.check(_raw(dev, z, case, label=label, lut=lut, cm=cm2, oob=oob2), "dve_evaluate")
    assert torch.equal(cm2.cpu().long(), want) and int(oob2.item()) == bad


def test_outputs_not_asked_for_are_not_written(dev):
    from mscs_amd import _lib_eval as le
    case = cases.CASES[5]
    C, H0, W0 = case[0], case[8], case[9]
    z = cases.logits(case).to(dev)
    label = cases.target(case).to(dev)
    cm = torch.full((C, C + 1), 77, dtype=torch.int32, device=dev)
    oob = torch.full((1,), 78, dtype=torch.int32, device=dev)
    ids = torch.full((H0, W0), 79, dtype=torch.uint8, device=dev)
    only = torch.empty_like(ids)
    le.check(_raw(dev, z, case, ids=only), "dve_evaluate")                             # ids alone
    torch.cuda.synchronize()
    assert bool((cm == 77).all()) and int(oob.item()) == 78
    le.check(_raw(dev, z, case, label=label, cm=cm, oob=oob), "dve_evaluate")          # cm alone
    torch.cuda.synchronize()
    assert bool((ids == 79).all()) and int(oob.item()) == 78
    want, _ = cases.bincount_cm(only, label, C, C + 1)
    assert torch.equal(cm.cpu().long() - 77, want)
    # refused before a launch
    assert _raw(dev, z, case, label=label, cm=cm, ids=ids) != 0 and _raw(dev, z, case) != 0
    assert _raw(dev, z, case, label=label.to(torch.int64), lut=cases.lut().to(dev), cm=cm, oob=oob) != 0
    torch.cuda.synchronize()
    assert bool((ids == 79).all()) and int(oob.item()) == 78


@pytest.mark.parametrize("case", (cases.DENSE, cases.CASES[0]), ids=cases.case_id)
def test_padding_does_not_enter(dev, case):
    """Stage 2 is a resize FROM the crop: class 0 set to 1e30 everywhere outside rows [0, rh) x columns [0, rw) of the dense
    logits changes neither ids nor the matrix.  (A resize of the whole map, sliced afterwards, would read those values at the
    crop's last rows and columns.)  On the lazy case the stage-1 map is formed first and poisoned: the dense form of the case."""
    from mscs_amd.utils import evaluate_at_original
    C, h, w, a1, Hp, Wp, rh, rw, H0, W0, a2 = case
    z = cases.logits(case)
    if h:
        z = F.interpolate(z, size=(Hp, Wp), mode="bilinear", align_corners=bool(a1))
    poisoned = z.clone()
    poisoned[:, 0, rh:, :] = 1e30
    poisoned[:, 0, :, rw:] = 1e30
    assert not torch.equal(poisoned, z)
    t = cases.target(case).to(dev)
    a = evaluate_at_original(z.to(dev), t, (rh, rw), (H0, W0), bool(a2), "ADE20K", return_ids=True)
    b = evaluate_at_original(poisoned.to(dev), t, (rh, rw), (H0, W0), bool(a2), "ADE20K", return_ids=True)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])
    assert not bool((b[1] == 0).all())


def test_upsampled_logits_stay_low_resolution(dev):
    from mscs_amd.utils import evaluate_at_original
    case = cases.CASES[0]
    C, h, w, a1, Hp, Wp, rh, rw, H0, W0, a2 = case
    out = cases.wrap(cases.logits(case).to(dev), case)
    evaluate_at_original(out, cases.target(case).to(dev), (rh, rw), (H0, W0), bool(a2), "ADE20K", return_ids=True)
    assert out._full is None


def test_switch_off_takes_the_composition(dev, monkeypatch):
    from mscs_amd import _lib_eval as le
    from mscs_amd.debug import cfg as dbg
    from mscs_amd.utils import evaluate_at_original
    from mscs_amd.utils.metrics import take_out_of_range
    case = cases.CASES[0]
    C, h, w, a1, Hp, Wp, rh, rw, H0, W0, a2 = case
    z, ref, ok = cases.reference(case)
    t = cases.target(case)
    t[0, :3] = 200                                             # out of range: counted, not raised, on the device
    take_out_of_range(dev)
    monkeypatch.setattr(dbg, "eval_hip", False)
    before = le.calls["evaluate"]
    out = cases.wrap(z.to(dev), case)
    cm, ids = evaluate_at_original(out, t.to(dev), (rh, rw), (H0, W0), bool(a2), "ADE20K", return_ids=True)
    assert le.calls["evaluate"] == before and ids.is_cuda and ids.dtype == torch.uint8 and out._full is not None
    _check(ids, ref, ok, "composition")
    want, bad = cases.bincount_cm(ids, t, C, C + 1)
    assert torch.equal(cm.cpu().long(), want[:, :C]) and bad == 3 and int(take_out_of_range(dev).item()) == 3
    monkeypatch.setattr(dbg, "eval_hip", True)
    cm2, ids2 = evaluate_at_original(cases.wrap(z.to(dev), case), t.to(dev), (rh, rw), (H0, W0), bool(a2), "ADE20K", return_ids=True)
    assert le.calls["evaluate"] == before + 1 and int(take_out_of_range(dev).item()) == 3
    same = ids2 == ids
    assert bool(same.cpu()[ok].all())                          # kernel and composition agree wherever float64 decides


def test_memory_stays_at_the_outputs(dev):
    """C = 150, lazy 128 x 128 -> 512 x 512, crop 512 x 500, out 1024 x 1000: the outputs are 1 MB (ids) + 91 KB (matrix); the
    composition's two maps would be 157 MB + 614 MB.  The bound of 16 MiB is arithmetic, not a measurement."""
    from mscs_amd import _lib_eval as le
    from mscs_amd.utils import evaluate_at_original
    from mscs_amd.models.ops_logits import UpsampledLogits
    z = torch.randn(1, 150, 128, 128, generator=torch.Generator().manual_seed(1), device="cpu").to(dev)
    t = torch.randint(0, 151, (1024, 1000), generator=torch.Generator().manual_seed(2)).to(torch.uint8).to(dev)
    evaluate_at_original(UpsampledLogits(z[:, :, :8, :8].contiguous(), (32, 32), False), t[:64, :64].contiguous(), (32, 30), (64, 64),
                         False, "ADE20K")                      # (the counter of out-of-range targets exists before the measurement)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    before = le.calls["evaluate"]
    out = UpsampledLogits(z, (512, 512), False)
    cm, ids = evaluate_at_original(out, t, (512, 500), (1024, 1000), False, "ADE20K", return_ids=True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(dev) - base
    print("peak above the inputs:", rise, "bytes")
    assert le.calls["evaluate"] == before + 1 and out._full is None
    assert rise < 16 * 2 ** 20
    assert int(cm.sum()) == 1024 * 1000 - int((t == 150).sum()) and tuple(ids.shape) == (1, 1024, 1000)


def test_manager_validates_on_the_gpu(dev, tmp_path):
    """The ADE20K resize_val config of tests/test_eval_host.py on the device with graph.lazy_logits: one kernel call per validation
    image, on the model's 1/4 map, and the matrix of the composition on the dense output wherever the two arg-max maps agree."""
    import numpy as np
    from mscs_amd import _lib_eval as le
    from mscs_amd.managers import HRNetManager
    from mscs_amd.utils import evaluate as ev, set_verbosity
    from mscs_amd.utils.metrics import take_out_of_range
    manager_cfg = cases.manager_cfg
    set_verbosity(40)
    rng = (torch.get_rng_state(), np.random.get_state())
    take_out_of_range(dev)
    try:
        cfg = manager_cfg(tmp_path, cuda=True)
        cfg["graph"]["lazy_logits"] = True
        m = HRNetManager(cfg, autostart=False)
        m.setup()
        seen = []
        real = ev.evaluate_at_original

        def spy(output, *a, **k):
            seen.append(output)
            return real(output, *a, **k)
        ev.evaluate_at_original = spy
        try:
            before = le.calls["evaluate"]
            miou = m.validate()
        finally:
            ev.evaluate_at_original = real
        assert le.calls["evaluate"] == before + 2 and 0.0 <= miou <= 1.0
        for out in seen:
            assert hasattr(out, "materialize") and out._full is None and tuple(out.lowres.shape) == (1, 150, 16, 32)
            assert tuple(out.size) == (64, 128)
        # the same through infer(), lazily as well
        path = m.save_checkpoint(path=str(tmp_path / "chk.pt"))
        mi = HRNetManager(manager_cfg(tmp_path / "infer", cuda=True, mode="inference", load_checkpoint=path, tta=False), autostart=False)
        mi.setup()
        before = le.calls["evaluate"]
        mious = mi.infer()
        assert le.calls["evaluate"] == before + 2 and 0.0 <= float(mious["mean_iou"]) <= 1.0
        assert not os.path.exists(tmp_path / "infer" / "run0")
    finally:
        torch.set_rng_state(rng[0])
        np.random.set_state(rng[1])
