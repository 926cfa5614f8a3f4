"""OhemCrossEntropy on its kernels (csrc/dcl_ohem.hip, include/dcl_ohem.h): the selection is exact (bitwise against a sort of the
library's own probability map); the mask, the loss and the gradient against the float64 reference; bitwise reproducible, also beside
a matrix kernel of another stream; the backward is dcl_upsample_ce_bwd on the hard-target map; the switch and the fall-backs; one
HRNet training step of the manager without a host synchronisation inside the loss.

The bounds of the float64 comparison are FOUR TIMES THE ERROR OF THE FLOAT32 COMPOSITION (ohem_reference in float32 on the CPU against
itself in float64, same case, same mask; computed before any kernel runs), but not below a round-off floor, because a composition
that happens to be exact on a case is no bound for arithmetic in another order:

  * l_i = w_t (lse_i - z_t).  z_t is a bilinear interpolation, three rounded sums of products at magnitude <= Z = max |z| (1.5 ulp);
    lse = m + log(sum) is one more rounding at magnitude <= Z + ln C (0.5 ulp) on top of the relative error of the sum of
    exponentials; the difference rounds once more (0.5 ulp).  With the ulp taken at Z + ln C:  |err l_i| <= 4 ulp(Z + ln C) max w,
    and the mean over the kept pixels errs by no more.  LOSS_FLOOR = 4 ulp32(Z + ln C) max(w).
  * dz_j[c] = sum over the output pixels i in the footprint of j of  wy wx kept_i w_t (softmax_c(i) - [c = t_i]) / m.
    softmax_c = exp(z_c - lse): the argument errs by <= 4 ulp(Z + ln C) as above, which is the relative error of the result (<= 1),
    plus 1.3e-7 for the exponential itself; the weights wy wx of a footprint sum to at most S = 2.25 scale^2 (1 for dense logits); the
    accumulation of its T = (2 scale + 2)^2 terms adds T 2^-24 relative to S max(w) / m.
    GRAD_FLOOR = max(w) S / m (4 ulp32(Z + ln C) + 1.3e-7 + T 2^-24).
Neither number is taken from the code under test."""
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

import _ohem_cases as cases

pytestmark = pytest.mark.gpu

ACCURACY = {}            # case id -> the bounds and the errors observed (profiles/ohem_accuracy.json is a copy of this)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib, _lib_ohem
    _lib.lib()
    _lib_ohem.lib()
    return torch.device("cuda:0")


def _mod():
    import importlib
    return importlib.import_module("mscs_amd.losses.OhemCrossEntropy")


def _run(dev, z, t, w, ignore, thresh, mk, size=None, align=False, grad=True):
    """(loss, dz or None, holder) of the kernel path"""
    m = _mod()
    zd = z.to(dev).requires_grad_(grad)
    holder = {"want_kept": True}
    loss = m.ohem_cross_entropy(zd, t.to(dev), None if w is None else w.to(dev), ignore, thresh, mk, size=size, align_corners=align,
                                holder=holder)
    assert holder["path"] == "hip"
    dz = None
    if grad:
        loss.backward()
        dz = zd.grad
    return loss.detach(), dz, holder


def _case(dev, ci, si, grad=True):
    d = cases.inputs(ci)
    thresh, mk = cases.settings(d["n"])[si]
    return d, thresh, mk, _run(dev, d["z"], d["t"], d["w"], d["ignore"], thresh, mk, d["size"], d["align"], grad)


def _res(holder):
    from mscs_amd import _lib_ohem as oh
    r = holder["res"].cpu()
    f = r.view(torch.float32)
    return {"loss": f[oh.RES_LOSS], "denom": float(f[oh.RES_DENOM]), "v": f[oh.RES_V], "thr": f[oh.RES_THR], "n": int(r[oh.RES_N]),
            "m": int(r[oh.RES_M]), "k": int(r[oh.RES_K]), "empty": int(r[oh.RES_EMPTY])}


def _check_exact(holder, t, C, ignore, thresh, mk):
    """v == sort(p_lib[valid])[k] bitwise, m == (p_lib < thr).sum(), and the maps are those of the mask"""
    r = _res(holder)
    p = holder["p"].cpu()
    bits = p.view(torch.int32)
    valid = (t >= 0) & (t < C) & (t != ignore)
    assert torch.equal(bits != -1, valid), "exactly the invalid pixels hold the invalid pattern"
    n = int(valid.sum())
    assert r["n"] == n and r["empty"] == (1 if n == 0 else 0)
    if n == 0:
        assert r["k"] == 0 and float(r["v"]) == 0.0 and r["m"] == 0 and float(r["loss"]) == 0.0
        return r
    k = min(max(mk, 1), n - 1)
    assert r["k"] == k
    pv = p[valid]
    assert bool((pv >= 0).all()) and bool(torch.isfinite(pv).all())
    want_v = torch.sort(pv).values[k]
    assert int(r["v"].view(torch.int32)) == int(want_v.view(torch.int32)), (float(r["v"]), float(want_v))
    thr = torch.maximum(want_v, torch.tensor(thresh, dtype=torch.float32))
    assert int(r["thr"].view(torch.int32)) == int(thr.view(torch.int32))
    kept = valid & (p < thr)
    assert r["m"] == int(kept.sum()) and r["denom"] == float(max(r["m"], 1))
    assert torch.equal(holder["kept"].cpu().bool(), kept)
    assert torch.equal(holder["hard"].cpu(), torch.where(kept, t, torch.full_like(t, ignore)))
    assert bool((holder["l"].cpu()[~valid] == 0).all())
    return r


@pytest.mark.parametrize("cs", cases.ALL, ids=cases.ident)
def test_selection_is_exact(dev, cs):
    ci, si = cs
    d, thresh, mk, (loss, _, holder) = _case(dev, ci, si, grad=False)
    r = _check_exact(holder, d["t"], d["C"], d["ignore"], thresh, mk)
    assert float(loss) == float(r["loss"]) and r["m"] > 0


def test_selection_on_the_tie_table(dev):
    tt = cases.tie_table()
    cum, sizes = tt["cum"], tt["sizes"]
    for g in range(7):
        for mk, want in ((cum[g], cum[g]), (cum[g] - 1, cum[g] - sizes[g]), (cum[g] + 1, cum[g])):
            if mk < 1:
                continue
            loss, dz, holder = _run(dev, tt["z"], tt["t"], None, -1, 0.0, mk)
            r = _check_exact(holder, tt["t"], 6, -1, 0.0, mk)
            assert r["m"] == want, (g, mk, r)
            if want == 0:                                   # m == 0 by ties: zero loss, zero gradient
                assert float(loss) == 0.0 and float(dz.abs().max()) == 0.0
    _, _, holder = _run(dev, tt["z"], tt["t"], None, -1, 0.0, 10 ** 9, grad=False)
    assert _check_exact(holder, tt["t"], 6, -1, 0.0, 10 ** 9)["m"] == cum[6]


def test_the_third_pass_decides(dev):
    c = cases.top22()
    n = int((c["t"] != c["ignore"]).sum())
    for mk in (1, n // 7, n // 2, n - 2, n - 1, n + 5):
        _, _, holder = _run(dev, c["z"], c["t"], None, c["ignore"], 0.0, mk, grad=False)
        bits = holder["p"].cpu().view(torch.int32)[c["t"] != c["ignore"]]
        assert bool(((bits >> 10) == c["centre_bits"]).all()), "the case is built so that every p shares its top 22 bits"
        assert int(bits.unique().numel()) > 100
        _check_exact(holder, c["t"], 3, c["ignore"], 0.0, mk)


def test_no_valid_pixel_and_a_single_one(dev):
    z = torch.randn(2, 4, 5, 7, generator=torch.Generator().manual_seed(3))
    t = torch.full((2, 20, 28), 4)
    loss, dz, holder = _run(dev, z, t, None, 4, 0.7, 10, size=(20, 28))
    r = _check_exact(holder, t, 4, 4, 0.7, 10)
    assert r["empty"] == 1 and float(loss) == 0.0 and float(dz.abs().max()) == 0.0 and bool(torch.isfinite(dz).all())
    t[1, 3, 9] = 2
    p = float(_run(dev, z, t, None, 4, 0.99999, 10, size=(20, 28), grad=False)[2]["p"][1, 3, 9])
    for thresh, want in ((min(p + 0.01, 1.0), 1), (p, 0)):           # strict: a pixel AT the threshold is not kept
        loss, dz, holder = _run(dev, z, t, None, 4, thresh, 10, size=(20, 28))
        r = _check_exact(holder, t, 4, 4, thresh, 10)
        assert (r["n"], r["k"], r["m"]) == (1, 0, want)
        assert (float(loss) > 0 and float(dz.abs().max()) > 0) if want else (float(loss) == 0.0 and float(dz.abs().max()) == 0.0)


@pytest.mark.parametrize("cs", cases.ALL, ids=cases.ident)
def test_mask_against_float64(dev, cs):
    ci, si = cs
    d, thresh, mk, (_, _, holder) = _case(dev, ci, si, grad=False)
    _, thr, kept, _ = cases.reference(ci, si)
    amb = cases.ambiguous(ci, si)
    assert int(amb.sum()) <= cases.MAX_AMBIGUOUS
    got = holder["kept"].cpu().bool()
    assert torch.equal(got[~amb], kept[~amb]), int((got != kept).sum())
    assert abs(float(_res(holder)["thr"]) - float(thr)) <= 1e-5 * float(thr)


def _same(a, b):
    """bitwise (p holds a NaN pattern at the invalid pixels: floats are compared as words)"""
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def _ulp32(x):
    return 2.0 ** (math.floor(math.log2(x)) - 23)


@pytest.mark.parametrize("cs", cases.ALL, ids=cases.ident)
def test_loss_and_gradient_against_float64(dev, cs):
    ci, si = cs
    m = _mod()
    d = cases.inputs(ci)
    thresh, mk = cases.settings(d["n"])[si]
    args = dict(size=d["size"], align_corners=d["align"])
    _, _, kept64, _ = cases.reference(ci, si)

    def composition(dtype, kept):
        z = d["z"].clone().requires_grad_(True)
        loss = m.ohem_reference(z, d["t"], d["w"], d["ignore"], thresh, mk, dtype=dtype, kept=kept, **args)[0]
        loss.backward()
        return loss.detach().double(), z.grad.double()
    # the float32 composition's own error, before any kernel runs
    l64, g64 = composition(torch.float64, kept64)
    l32, g32 = composition(torch.float32, kept64)
    comp_loss, comp_grad = float((l32 - l64).abs()), float((g32 - g64).abs().max())
    scale = cases.CASES[ci][4]
    wmax = 1.0 if d["w"] is None else float(d["w"].max())
    u = _ulp32(float(d["z"].abs().max()) + math.log(d["C"]))
    m64 = int(kept64.sum())
    loss_floor = 4 * u * wmax
    S, T = (1.0, 1) if scale == 1 else (2.25 * scale * scale, (2 * scale + 2) ** 2)
    grad_floor = wmax * S / m64 * (4 * u + 1.3e-7 + T * 2.0 ** -24)
    loss_bound, grad_bound = max(4 * comp_loss, loss_floor), max(4 * comp_grad, grad_floor)
    # the kernels; the reference is given THEIR mask, so that the comparison does not depend on ambiguous pixels
    loss, dz, holder = _run(dev, d["z"], d["t"], d["w"], d["ignore"], thresh, mk, d["size"], d["align"])
    kept_lib = holder["kept"].cpu().bool()
    lref, gref = composition(torch.float64, kept_lib)
    err_loss, err_grad = abs(float(loss) - float(lref)), float((dz.cpu().double() - gref).abs().max())
    ACCURACY[cases.ident(cs)] = {"loss": float(lref), "grad_max": float(gref.abs().max()), "kept": int(kept_lib.sum()),
                                 "composition_f32_loss_err": comp_loss, "composition_f32_grad_err": comp_grad,
                                 "loss_floor": loss_floor, "grad_floor": grad_floor, "loss_bound": loss_bound, "grad_bound": grad_bound,
                                 "kernel_loss_err": err_loss, "kernel_grad_err": err_grad}
    print(cases.ident(cs), ACCURACY[cases.ident(cs)])
    assert err_loss <= loss_bound, (err_loss, loss_bound)
    assert err_grad <= grad_bound, (err_grad, grad_bound)


def test_accuracy_record():
    """The figures of the test above, written where DCL_OHEM_ACCURACY_OUT says (profiles/ohem_accuracy.json is such a copy)."""
    out = os.environ.get("DCL_OHEM_ACCURACY_OUT")
    if out and ACCURACY:
        with open(out, "w") as f:
            json.dump({"bound": "max(4 x error of the float32 composition against float64, round-off floor); tests/test_ohem_hip.py",
                       "cases": ACCURACY}, f, indent=1, sort_keys=True)
    assert all(v["kernel_loss_err"] <= v["loss_bound"] and v["kernel_grad_err"] <= v["grad_bound"] for v in ACCURACY.values())


def test_bitwise(dev):
    """run to run; beside a matrix kernel on another stream; dz = dcl_upsample_ce_bwd on the hard-target map with 1 / m; the arg-max
    map of the lazy logits is the plain cross_entropy path's."""
    from mscs_amd import _lib
    from mscs_amd.models import ops
    from mscs_amd.models.ops_logits import UpsampledLogits
    for ci, si in ((0, 2), (1, 1), (3, 4)):
        d = cases.inputs(ci)
        thresh, mk = cases.settings(d["n"])[si]
        run = lambda: _run(dev, d["z"], d["t"], d["w"], d["ignore"], thresh, mk, d["size"], d["align"])     # noqa: E731
        loss0, dz0, h0 = run()
        loss1, dz1, h1 = run()
        torch.cuda.synchronize()
        keys = ("p", "l", "lse", "hard", "kept", "res", "pred")
        assert torch.equal(loss0, loss1) and torch.equal(dz0, dz1) and all(_same(h0[k], h1[k]) for k in keys)
        # the backward is the existing entry on the hard-target map, with 1 / m as its device scalar
        z, t = d["z"].to(dev), d["t"].to(dev)
        n, c, h, w = z.shape
        H, W = d["size"] or (h, w)
        r = _res(h0)
        gscale = torch.ones(1, device=dev) / torch.tensor([float(r["m"])], device=dev)
        want = torch.empty_like(z)
        wt = None if d["w"] is None else d["w"].to(dev)
        _lib.check(_lib.lib().dcl_upsample_ce_bwd(_lib.ptr(z), n, c, h, w, H, W, 1 if d["align"] and d["size"] else 0,
                                                  _lib.ptr(h0["hard"]), _lib.ptr(wt), d["ignore"], _lib.ptr(h0["lse"]),
                                                  _lib.ptr(gscale), _lib.ptr(want), _lib.stream_ptr(dev)), "dcl_upsample_ce_bwd")
        assert torch.equal(dz0, want)
        if d["size"]:
            a, b = UpsampledLogits(z, d["size"], d["align"]), UpsampledLogits(z, d["size"], d["align"])
            la = a.ohem_cross_entropy(t, wt, d["ignore"], thresh, mk)
            b.cross_entropy(t, weight=wt, ignore_index=d["ignore"])
            assert torch.equal(la, loss0) and a._full is None and a.pred.dtype == torch.uint8 and torch.equal(a.pred, b.pred)
        if ci != 0:
            continue
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
                    outs.append(run())
            torch.cuda.synchronize()
            for lo, dzo, ho in outs:
                assert torch.equal(lo, loss0) and torch.equal(dzo, dz0) and all(_same(ho[k], h0[k]) for k in keys)


def test_switch_and_fallbacks(dev, monkeypatch):
    from mscs_amd import _lib_ohem as oh
    from mscs_amd.debug import cfg as dbg
    m = _mod()
    d = cases.inputs(0)
    thresh, mk = cases.settings(d["n"])[2]
    z, t, w = d["z"].to(dev), d["t"].to(dev), d["w"].to(dev)

    def composed(zz, tt, ww, size=d["size"]):
        holder = {}
        before = dict(oh.calls)
        got = m.ohem_cross_entropy(zz, tt, ww, d["ignore"], thresh, mk, size=size, align_corners=d["align"], holder=holder)
        want = m.ohem_reference(zz, tt, ww, d["ignore"], thresh, mk, size=size, align_corners=d["align"])[0]
        assert holder["path"] == "torch" and oh.calls == before and torch.equal(got, want)
        return got
    # DCL_OHEM_HIP=0 gives the composition, which agrees with the kernels
    monkeypatch.setattr(dbg, "ohem_hip", False)
    off = composed(z, t, w)
    monkeypatch.setattr(dbg, "ohem_hip", True)
    on = _run(dev, d["z"], d["t"], d["w"], d["ignore"], thresh, mk, d["size"], d["align"], grad=False)[0]
    assert abs(float(on) - float(off)) <= 1e-5 * float(off)
    # C = 256, fp16 logits and CPU tensors take the composition
    g = torch.Generator().manual_seed(4)
    z256 = torch.randn(1, 256, 6, 8, generator=g).to(dev)
    t256 = torch.randint(0, 256, (1, 24, 32), generator=g).to(dev)
    holder = {}
    m.ohem_cross_entropy(z256, t256, None, d["ignore"], 0.7, 10, size=(24, 32), holder=holder)
    assert holder["path"] == "torch"
    composed(z.half(), t, w.half())
    composed(d["z"], d["t"], d["w"])


def test_config_without_the_name_launches_nothing_of_it(dev):
    from mscs_amd import _lib_ohem as oh
    from mscs_amd.losses import LossWrapper
    from mscs_amd.models.ops_logits import UpsampledLogits
    d = cases.inputs(0)
    lw = LossWrapper({"losses": {"CrossEntropyLoss": 1.0}, "device": dev, "dataset": "CITYSCAPES", "experiment": 1})
    before = dict(oh.calls)
    lazy = UpsampledLogits(d["z"].to(dev).requires_grad_(True), d["size"], d["align"])
    loss = lw(lazy, d["t"].to(dev))
    loss.backward()
    want = F.cross_entropy(F.interpolate(d["z"].double(), size=d["size"], mode="bilinear"), d["t"], weight=d["w"].double(),
                           ignore_index=19)
    assert oh.calls == before and lazy._full is None and abs(float(loss) - float(want)) <= 1e-5 * float(want)
    # and with the name the three entries run once each, on the lazy object
    lw = LossWrapper({"losses": {"CrossEntropyLoss": 0, "OhemCrossEntropy": 1.0}, "device": dev, "dataset": "CITYSCAPES",
                      "experiment": 1, "ohem_min_kept": 500})
    lazy = UpsampledLogits(d["z"].to(dev).requires_grad_(True), d["size"], d["align"])
    loss = lw(lazy, d["t"].to(dev))
    loss.backward()
    assert {k: oh.calls[k] - before[k] for k in before} == {"target_prob": 1, "select": 1, "reduce": 1} and lazy._full is None
    ref = _mod().ohem_reference(d["z"], d["t"], d["w"], 19, 0.7, 500, size=d["size"], align_corners=d["align"], dtype=torch.float64)[0]
    assert abs(float(loss) - float(ref)) <= 1e-5 * float(ref)
    # both heads of TwoScaleLoss: each lazy object goes to its module as it is
    lw = LossWrapper({"losses": {"TwoScaleLoss": 1.0}, "device": dev, "dataset": "CITYSCAPES", "experiment": 1,
                      "interm": {"name": "OhemCrossEntropy", "weight": 0.4, "ohem_min_kept": 500},
                      "final": {"name": "OhemCrossEntropy", "weight": 1.0, "ohem_min_kept": 500}})
    before = dict(oh.calls)
    final, interm = (UpsampledLogits(zz.to(dev).requires_grad_(True), d["size"], d["align"]) for zz in (d["z"], torch.roll(d["z"], 1, 0)))
    loss = lw(final, d["t"].to(dev), interm_prediction=interm)
    loss.backward()
    assert {k: oh.calls[k] - before[k] for k in before} == {"target_prob": 2, "select": 2, "reduce": 2}
    assert final._full is None and interm._full is None and float(interm.lowres.grad.abs().max()) > 0
    ref2 = _mod().ohem_reference(torch.roll(d["z"], 1, 0), d["t"], d["w"], 19, 0.7, 500, size=d["size"], align_corners=d["align"],
                                 dtype=torch.float64)[0]
    assert abs(float(loss.detach()) - float(ref + 0.4 * ref2)) <= 1e-5 * float(ref + 0.4 * ref2)


def test_hrnet_training_step_mines_without_a_host_synchronisation(dev, tmp_path, monkeypatch):
    from mscs_amd import _lib_ohem as oh
    from mscs_amd.managers import HRNetManager
    from mscs_amd.utils import set_verbosity
    set_verbosity(40)
    cfg = {"name": "ohem", "mode": "training", "manager": "HRNet", "cuda": True, "parallel": False, "gpu_device": [0], "seed": 3,
           "log_every_n_steps": 1000, "log_path": str(tmp_path), "run_id": "run0", "save_checkpoints": False,
           "graph": {"model": "HRNet", "backbone": "hrnet18", "sync_bn": False, "pretrained": False, "align_corners": True,
                     "lazy_logits": True},
           "data": {"dataset": "CITYSCAPES", "experiment": 1, "batch_size": 2, "num_workers": 0, "synthetic": True,
                    "synthetic_length": 4, "transform_values": {"crop_shape": [64, 128]}},
           "loss": {"name": "LossWrapper", "losses": {"CrossEntropyLoss": 0, "OhemCrossEntropy": 1}, "ohem_thresh": 0.9,
                    "ohem_min_kept": 2000},
           "train": {"learning_rate": 0.01, "lr_fct": "polynomial", "optim": "SGD", "lr_batchwise": True, "epochs": 1}}
    mgr = HRNetManager(cfg, autostart=False)
    mgr.setup()
    mgr.model.train()
    gen = torch.Generator().manual_seed(0)
    img = torch.randn(2, 3, 64, 128, generator=gen).to(dev)
    lbl = torch.randint(0, 20, (2, 64, 128), generator=gen).to(dev)
    real = mgr.loss.forward

    def guarded(*a, **k):
        torch.cuda.set_sync_debug_mode("error")
        try:
            return real(*a, **k)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    monkeypatch.setattr(mgr.loss, "forward", guarded)
    before = dict(oh.calls)
    mgr.optimiser.zero_grad()
    ret = mgr.forward_step(img, lbl)
    ret["loss"].backward()
    mgr.optimiser.step()
    torch.cuda.synchronize()
    assert {k: oh.calls[k] - before[k] for k in before} == {"target_prob": 1, "select": 1, "reduce": 1}
    assert math.isfinite(float(ret["loss"].detach())) and float(ret["loss"].detach()) > 0
    assert type(ret["output"]).__name__ == "UpsampledLogits" and ret["output"]._full is None
