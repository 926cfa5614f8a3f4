"""OhemCrossEntropy without a GPU: ``ohem_reference`` against a literal restatement of the public HRNet formula; the tie table (the
off-by-one test of the rank); the edge cases n == 0, n == 1 and m == 0; the wiring through LossWrapper and TwoScaleLoss with dense
logits and with an UpsampledLogits; the plan header of the kernels (csrc/dcl_ohem_plan.h) in a stand-alone sanitizer build."""
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import _ohem_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mod():
    """the module losses/OhemCrossEntropy.py (the package attribute of that name is the class)"""
    import importlib

    import mscs_amd  # noqa: F401
    return importlib.import_module("mscs_amd.losses.OhemCrossEntropy")


def public_formula(score, target, weight, ignore_label, thresh, min_kept):
    """The public HRNet OhemCrossEntropy._ohem_forward, line for line (score at the label size)."""
    pred = F.softmax(score, dim=1)
    pixel_losses = F.cross_entropy(score, target, weight=weight, ignore_index=ignore_label, reduction='none').contiguous().view(-1)
    mask = target.contiguous().view(-1) != ignore_label
    tmp_target = target.clone()
    tmp_target[tmp_target == ignore_label] = 0
    pred = pred.gather(1, tmp_target.unsqueeze(1))
    pred, ind = pred.contiguous().view(-1,)[mask].contiguous().sort()
    min_value = pred[min(min_kept, pred.numel() - 1)]
    threshold = max(min_value, thresh)
    pixel_losses = pixel_losses[mask][ind]
    pixel_losses = pixel_losses[pred < threshold]
    return pixel_losses.mean(), threshold, int((pred < threshold).sum())


@pytest.mark.parametrize("cs", cases.ALL, ids=cases.ident)
def test_reference_is_the_public_formula(cs):
    ci, si = cs
    d = cases.inputs(ci)
    thresh, mk = cases.settings(d["n"])[si]
    loss, thr, kept, p = cases.reference(ci, si)
    z = d["z"].double()
    if d["size"] is not None:
        z = F.interpolate(z, size=d["size"], mode="bilinear", align_corners=d["align"])
    w = None if d["w"] is None else d["w"].double()
    want, want_thr, want_m = public_formula(z, d["t"], w, d["ignore"], thresh, mk)
    assert int(kept.sum()) == want_m and want_m > 0
    assert abs(float(thr) - float(want_thr)) <= 1e-14            # (softmax against exp(log_softmax): a few ulp of float64)
    assert abs(float(loss) - float(want)) <= 1e-12 * abs(float(want))
    # which regime the setting is in (what the five settings are there to cover)
    n = d["n"]
    v = torch.sort(p[~torch.isnan(p)]).values[min(mk, n - 1)]
    assert {0: float(thr) == thresh, 1: float(thr) == float(v) > thresh, 3: min(mk, n - 1) == n - 1 and mk > n,
            4: mk == n - 1}.get(si, True)
    # at most the pivot is ambiguous, and the float32 composition finds the same mask
    assert int(cases.ambiguous(ci, si).sum()) <= 1
    m = _mod()
    with torch.no_grad():
        loss32, _, kept32, _ = m.ohem_reference(d["z"], d["t"], d["w"], d["ignore"], thresh, mk, size=d["size"], align_corners=d["align"])
    assert torch.equal(kept32, kept)
    assert abs(float(loss32) - float(loss)) <= 1e-6 * abs(float(loss))


def test_tie_table_boundaries():
    """min_kept equal to a cumulative group count keeps that whole group (the pivot is the first pixel of the NEXT group and the
    comparison is strict); one less excludes the group (the pivot is its last pixel)."""
    m = _mod()
    tt = cases.tie_table()
    z, t, cum, sizes = tt["z"].double(), tt["t"], tt["cum"], tt["sizes"]
    assert all(s > 0 for s in sizes) and cum[-1] == 1200
    for g in range(7):
        for mk, want in ((cum[g], cum[g]), (cum[g] - 1, cum[g] - sizes[g]), (cum[g] + 1, cum[g])):
            if mk < 1:
                continue
            loss, thr, kept, p = m.ohem_reference(z, t, None, -1, 0.0, mk)
            assert int(kept.sum()) == want, (g, mk)
            if want:
                pf = public_formula(z, t, None, -1, 0.0, mk)
                assert pf[2] == want and abs(float(pf[0]) - float(loss)) <= 1e-12
            else:
                assert float(loss) == 0.0                              # m == 0 by ties: the group starts at rank 0
    # the last group: k clamps to n - 1, the pivot is in the last group, which is never kept
    _, _, kept, _ = m.ohem_reference(z, t, None, -1, 0.0, 10 ** 6)
    assert int(kept.sum()) == cum[6]
    # the threshold in between two table values keeps the groups below it, whatever the rank says
    _, _, kept, _ = m.ohem_reference(z, t, None, -1, 0.5 * (tt["p"][4] + tt["p"][5]), 1)
    assert int(kept.sum()) == cum[4]


def test_edge_cases():
    m = _mod()
    z = torch.randn(1, 4, 3, 5, dtype=torch.float64, requires_grad=True)
    # n == 0: zero loss, zero gradient, a graph that backpropagates
    t = torch.full((1, 3, 5), 4)
    loss, thr, kept, _ = m.ohem_reference(z, t, None, 4, 0.7, 10)
    assert float(loss) == 0.0 and int(kept.sum()) == 0 and loss.requires_grad
    loss.backward()
    assert float(z.grad.abs().max()) == 0.0
    # n == 1: k = 0, v = p; below thresh it is kept, at or above it is not (m == 0: zero loss, zero gradient)
    t[0, 1, 2] = 1
    p = float(torch.softmax(z[0, :, 1, 2], 0)[1])
    for thresh, want in ((p + 0.01, 1), (p - 0.01, 0)):
        z.grad = None
        loss, thr, kept, _ = m.ohem_reference(z, t, None, 4, thresh, 10)
        assert int(kept.sum()) == want and abs(float(thr) - max(p, thresh)) < 1e-15
        loss.backward()
        if want:
            assert abs(float(loss) + torch.log_softmax(z[0, :, 1, 2], 0)[1].item()) < 1e-12 and float(z.grad.abs().max()) > 0
        else:
            assert float(loss) == 0.0 and float(z.grad.abs().max()) == 0.0
    # m == 0 by ties: every valid pixel has the same p
    z0 = torch.zeros(1, 4, 3, 5, dtype=torch.float64, requires_grad=True)
    loss, thr, kept, _ = m.ohem_reference(z0, torch.ones(1, 3, 5, dtype=torch.int64), None, 4, 0.1, 5)
    loss.backward()
    assert float(loss) == 0.0 and int(kept.sum()) == 0 and float(thr) == 0.25 and float(z0.grad.abs().max()) == 0.0
    # a given mask overrides the selection
    given = torch.zeros(1, 3, 5, dtype=torch.bool)
    given[0, 0, :3] = True
    t1 = torch.ones(1, 3, 5, dtype=torch.int64)
    loss, _, kept, _ = m.ohem_reference(z, t1, None, 4, 0.0, 1, kept=given)
    assert torch.equal(kept, given) and abs(float(loss) + float(torch.log_softmax(z[0, :, 0, :3], 0)[1].mean())) < 1e-12


def _wrapper_cfg(**extra):
    cfg = {"losses": {"OhemCrossEntropy": 1.0}, "device": "cpu", "dataset": "CITYSCAPES", "experiment": 1, "ohem_thresh": 0.6,
           "ohem_min_kept": 700}
    cfg.update(extra)
    return cfg


def test_loss_wrapper_and_two_scale_loss_take_the_name():
    """Both construct (a KeyError before the class existed) and equal the reference on the CPU, with dense logits and with an
    UpsampledLogits, which is handed to the module and not materialised by LossWrapper."""
    m = _mod()
    from mscs_amd.losses import LossWrapper, OhemCrossEntropy
    from mscs_amd.losses.TwoScaleLoss import CITYSCAPES_CLASS_WEIGHTS
    from mscs_amd.models.ops_logits import UpsampledLogits
    d = cases.inputs(0)
    w = torch.tensor(CITYSCAPES_CLASS_WEIGHTS)
    assert d["ignore"] == 19
    lw = LossWrapper(_wrapper_cfg())
    fn = lw.loss_classes["OhemCrossEntropy"]
    assert isinstance(fn, OhemCrossEntropy) and (fn.ignore_label, fn.thresh, fn.min_kept) == (19, 0.6, 700)
    assert OhemCrossEntropy({"dataset": "ADE20K", "experiment": 1}).weight is None
    dflt = OhemCrossEntropy({"dataset": "CITYSCAPES", "experiment": 1, "ohem_min_kept": 0})
    assert (dflt.thresh, dflt.min_kept) == (0.7, 1) and OhemCrossEntropy({"dataset": "CITYSCAPES", "experiment": 1}).min_kept == 100000
    full = F.interpolate(d["z"], size=d["size"], mode="bilinear", align_corners=d["align"])
    want = m.ohem_reference(full, d["t"], w, 19, 0.6, 700)[0]
    assert float(lw(full, d["t"])) == float(want) and float(lw.loss_vals["OhemCrossEntropy"]) == float(want)
    zl = d["z"].clone().requires_grad_(True)
    lazy = UpsampledLogits(zl, d["size"], d["align"])
    got = lw(lazy, d["t"])
    assert float(got) == float(want) and lazy._full is not None      # (the CPU path of the lazy object materialises by itself)
    got.backward()
    zr = d["z"].clone().requires_grad_(True)
    m.ohem_reference(zr, d["t"], w, 19, 0.6, 700, size=d["size"], align_corners=d["align"])[0].backward()
    assert torch.equal(zl.grad, zr.grad) and float(zl.grad.abs().max()) > 0
    # both heads of TwoScaleLoss on it
    heads = {"interm": {"name": "OhemCrossEntropy", "weight": 0.4, "ohem_thresh": 0.6, "ohem_min_kept": 700},
             "final": {"name": "OhemCrossEntropy", "weight": 1.0, "ohem_thresh": 0.9, "ohem_min_kept": 50}}
    lw2 = LossWrapper(_wrapper_cfg(losses={"TwoScaleLoss": 1.0}, **heads))
    ts = lw2.loss_classes["TwoScaleLoss"]
    assert isinstance(ts.loss_interm, OhemCrossEntropy) and ts.loss_final.min_kept == 50 and ts.loss_final.ignore_label == 19
    interm = torch.roll(d["z"], 1, 0)
    want2 = m.ohem_reference(full, d["t"], w, 19, 0.9, 50)[0] + 0.4 * m.ohem_reference(
        F.interpolate(interm, size=d["size"], mode="bilinear", align_corners=d["align"]), d["t"], w, 19, 0.6, 700)[0]
    dense = lw2(full, d["t"], interm_prediction=F.interpolate(interm, size=d["size"], mode="bilinear", align_corners=d["align"]))
    lazy2 = lw2(UpsampledLogits(d["z"], d["size"], d["align"]), d["t"],
                interm_prediction=UpsampledLogits(interm, d["size"], d["align"]))
    assert abs(float(dense) - float(want2)) <= 1e-6 * float(want2) and float(lazy2) == float(dense)


def test_logits_of_another_size_raise():
    from mscs_amd.losses import OhemCrossEntropy
    d = cases.inputs(0)
    fn = OhemCrossEntropy({"dataset": "CITYSCAPES", "experiment": 1})
    with pytest.raises(ValueError, match="label size"):
        fn(d["z"], d["t"])


def test_plan_header_under_sanitizers(tmp_path):
    """tests/ohem_plan_main.cpp: the bin picking against a sorted array, the digits, the workspace layout -- a stand-alone program
    with the address and undefined-behaviour sanitizers inside it."""
    from mscs_amd import _lib
    gxx = shutil.which("g++") or shutil.which("c++")
    cxx = gxx or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    static = ["-static-libasan", "-static-libubsan"] if gxx else []
    exe = str(tmp_path / "ohem_plan_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static +
                       ["-I", _lib.CSRC_DIR, os.path.join(ROOT, "tests", "ohem_plan_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ohem plan ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
