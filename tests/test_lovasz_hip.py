"""Lovasz-Softmax on the gfx950 kernels (csrc/dcl_lovasz.hip through losses/LovaszSoftmax.py) against the reference's recorded
results, against an fp64 restatement written here, and against this repository's fp32 PyTorch path as the yardstick of what fp32
can hold.

Tolerance (tests 2-4): |HIP - fp64| <= max(2 |PyTorch fp32 on the same device - fp64|, 8 * 2^-23 * |fp64 value|): the factor 2
allows another, equally valid order of the sums, the floor is eight fp32 roundings of the result.  The gradient is held the same
way on max |delta| / max |grad|.  Pixels that share an fp32 key with another pixel of their segment may legitimately swap ranks
(the sort's tie order is not part of the loss), so they are left out of the gradient comparison; their share is capped.
Every comparison prints its distances (run with -s)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
TIE_CAP = 1e-3          # share of elements that may sit in an fp32 tie


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_lovasz
    _lib_lovasz.lib()
    return torch.device("cuda:0")


def _module(cfg):
    from mscs_amd.losses import LovaszSoftmax
    return LovaszSoftmax(dict({"dataset": "CITYSCAPES", "experiment": 1}, **cfg))


def _run(cfg, logits, label, dev, hip):
    """(loss, gradient) on the device, through the HIP kernels or (hip = False) the PyTorch path, as float64 CPU tensors"""
    from mscs_amd.debug import cfg as dbg
    m = _module(cfg)
    x = logits.to(dev).requires_grad_(True)
    old = dbg.lovasz_hip
    dbg.lovasz_hip = hip
    try:
        loss = m(x, label.to(dev))
        loss.backward()
    finally:
        dbg.lovasz_hip = old
    assert loss.dim() == 0 and loss.dtype == torch.float32
    return loss.detach().double().cpu(), x.grad.double().cpu()


def _lovasz_grad64(fg_sorted):
    gts = fg_sorted.sum()
    inter = gts - fg_sorted.cumsum(0)
    union = gts + (1.0 - fg_sorted).cumsum(0)
    jac = 1.0 - inter / union
    if fg_sorted.numel() > 1:
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
    return jac


def _ref64(cfg, logits, label):
    """The loss restated in float64 from the same fp32 logits: (loss, gradient)."""
    m = _module(cfg)
    x = logits.double().requires_grad_(True)
    p = torch.softmax(x, dim=1)
    c = p.shape[1]
    lab = label.long()
    groups = [(p[i:i + 1], lab[i:i + 1]) for i in range(p.shape[0])] if m.per_image else [(p, lab)]
    losses = []
    for pg, lg in groups:
        pf = pg.permute(0, 2, 3, 1).reshape(-1, c)
        lf = lg.reshape(-1)
        if m.classes_to_ignore is not None:
            keep = lf != m.classes_to_ignore
            pf, lf = pf[keep], lf[keep]
        classes = range(c) if m.classes_to_consider in ("all", "present") else m.classes_to_consider
        terms = []
        for k in classes:
            fg = (lf == k).double()
            if pf.shape[0] == 0 or (m.classes_to_consider == "present" and fg.sum() == 0):
                continue
            err = (fg - pf[:, k]).abs()
            es, perm = torch.sort(err, dim=0, descending=True, stable=True)
            terms.append(torch.dot(es, _lovasz_grad64(fg[perm])))
        losses.append(sum(terms) / len(terms) if terms else pf.sum() * 0.0)
    loss = sum(losses) / len(losses)
    loss.backward()
    return loss.detach(), x.grad


def _tie_pixels(cfg, logits, label):
    """bool [N, H, W]: pixels that share their fp32 key with another pixel of the same segment, for some class; and the share of
    the N*C*H*W elements that sit in such ties.  Keys recomputed on the CPU in fp32."""
    m = _module(cfg)
    p = torch.softmax(logits.float(), dim=1)
    n, c, h, w = p.shape
    lab = label.long()
    valid = torch.ones_like(lab, dtype=torch.bool) if m.classes_to_ignore is None else lab != m.classes_to_ignore
    tied = torch.zeros(n, c, h, w, dtype=torch.bool)
    for k in range(c):
        e = ((lab == k).float() - p[:, k]).abs()
        for sl in ([slice(i, i + 1) for i in range(n)] if m.per_image else [slice(0, n)]):
            ev, vv = e[sl].reshape(-1), valid[sl].reshape(-1)
            _, inv, cnt = torch.unique(ev, return_inverse=True, return_counts=True)
            tied[sl, k] = ((cnt[inv] > 1) & vv).view(e[sl].shape)
    return tied.any(1), float(tied.sum()) / tied.numel()


def _labels(gen, shape, classes, ignore=None, ignored_share=0.0, dtype=torch.int64):
    lab = classes[torch.randint(0, len(classes), shape, generator=gen)]
    if ignored_share:
        lab[torch.rand(shape, generator=gen) < ignored_share] = ignore
    return lab.to(dtype)


def _case(name):
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    rn = lambda *s: torch.randn(*s, generator=g) * 2.0
    ar = torch.arange
    if name == "odd":                       # 2 x 5 x 37 x 53: odd sizes, the last class is the ignore id
        return {"classes_to_ignore": 5}, rn(2, 5, 37, 53), _labels(g, (2, 37, 53), ar(6))
    if name == "odd_two_tiles":             # a segment of 3 * 37 * 53 = 5883 elements: one full tile and a partial one
        return {"classes_to_ignore": 5, "classes_to_consider": "all"}, rn(3, 5, 37, 53), _labels(g, (3, 37, 53), ar(6))
    if name == "city_1":                    # a segment spans several workgroups in the sort and the scan
        return {}, rn(1, 19, 96, 160), _labels(g, (1, 96, 160), ar(20), dtype=torch.uint8)
    if name == "city_2_per_image":
        return {"per_image": True}, rn(2, 19, 96, 160), _labels(g, (2, 96, 160), ar(20))
    if name == "ade_150":                   # ADE20K's class count, 12 classes present
        return {"classes_to_ignore": 150}, rn(1, 150, 24, 24), _labels(g, (1, 24, 24), ar(0, 150, 13), dtype=torch.int32)
    if name == "one_pixel":
        return {"classes_to_ignore": None}, rn(1, 3, 1, 1), torch.tensor([[[1]]])
    if name == "ignored_30_per_image":      # about 30 % ignored, image 1 ignored altogether
        lab = _labels(g, (3, 33, 47), ar(7), ignore=7, ignored_share=0.3)
        lab[1] = 7
        return {"per_image": True, "classes_to_ignore": 7}, rn(3, 7, 33, 47), lab
    if name == "ignored_30":
        return {"classes_to_ignore": 7}, rn(2, 7, 33, 47), _labels(g, (2, 33, 47), ar(7), ignore=7, ignored_share=0.3)
    if name == "list":
        return ({"classes_to_ignore": 7, "classes_to_consider": [0, 2, 5]}, rn(2, 7, 33, 47),
                _labels(g, (2, 33, 47), ar(7), ignore=7, ignored_share=0.1))
    if name == "one_class_present":
        return {"classes_to_ignore": 7}, rn(2, 7, 33, 47), _labels(g, (2, 33, 47), torch.tensor([3, 7]))
    if name == "saturated":                 # +-60: softmax is 0 or 1 to the last bit at most pixels
        x = (torch.randint(0, 2, (2, 5, 37, 53), generator=g) * 2 - 1).float() * 60.0
        return {"classes_to_ignore": 5}, x, _labels(g, (2, 37, 53), ar(6))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _reference(name):
    cfg, x, lab = _case(name)
    return cfg, x, lab, _ref64(cfg, x, lab), _tie_pixels(cfg, x, lab)


def _hold_to_fp64(name, dev, check_grad=True):
    cfg, x, lab, (l64, g64), (tie, share) = _reference(name)
    lh, gh = _run(cfg, x, lab, dev, hip=True)
    lt, gt = _run(cfg, x, lab, dev, hip=False)
    d_hip, d_torch = abs(lh - l64).item(), abs(lt - l64).item()
    print(f"\n[lovasz parity] {name}: shape {tuple(x.shape)} cfg {json.dumps(cfg)} loss64 {l64.item():.9f} "
          f"|hip-64| {d_hip:.3e} |torch32-64| {d_torch:.3e} floor {8 * EPS * abs(l64.item()):.3e}")
    assert d_hip <= max(2 * d_torch, 8 * EPS * abs(l64.item())), (name, d_hip, d_torch)
    if not check_grad:
        return gh
    keep = (~tie)[:, None].expand_as(g64)
    gmax = g64.abs().max().item()
    r_hip = ((gh - g64).abs() * keep).max().item() / gmax
    r_torch = ((gt - g64).abs() * keep).max().item() / gmax
    print(f"[lovasz parity] {name}: grad max|d|/max|g| hip {r_hip:.3e} torch32 {r_torch:.3e} floor {8 * EPS:.3e} "
          f"tied share {share:.2e}")
    assert share <= TIE_CAP, (name, share)
    assert r_hip <= max(2 * r_torch, 8 * EPS), (name, r_hip, r_torch)
    return gh


# ---- 1. the reference's recorded results ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "per_image", "all"])
def test_reference_golden(dev, name):
    z = np.load(os.path.join(GOLDEN, "G10_lovasz.npz"))
    cfg = json.loads(str(z[name + "_cfg"]))
    x, lab = torch.from_numpy(z["logits"]), torch.from_numpy(z["label"])          # uint8 labels, as recorded
    loss, grad = _run(cfg, x, lab, dev, hip=True)
    np.testing.assert_allclose(loss.item(), z[name + "_loss"], rtol=1e-5)
    tie, share = _tie_pixels(cfg, x, lab)
    assert share <= TIE_CAP, share
    want = torch.from_numpy(z[name + "_grad"]).double()
    keep = (~tie)[:, None].expand_as(want)
    err = ((grad - want).abs() * keep).max().item()
    print(f"\n[lovasz parity] golden {name}: loss {loss.item():.8f} fixture {float(z[name + '_loss']):.8f} "
          f"grad max|d| {err:.3e} max|g| {want.abs().max().item():.3e} tied share {share:.2e}")
    assert err <= 1e-6 * want.abs().max().item() + 1e-9          # the bound tests/test_models.py holds the PyTorch path to


# ---- 2. fp64 at awkward shapes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "odd_two_tiles", "city_1", "city_2_per_image", "ade_150", "one_pixel",
                                  "ignored_30_per_image", "ignored_30", "list"])
def test_fp64_parity(dev, name):
    gh = _hold_to_fp64(name, dev)
    cfg, x, lab = _case(name)
    ign = _module(cfg).classes_to_ignore
    if ign is not None:
        assert bool((gh * (lab == ign)[:, None]).eq(0).all()), "gradient on an ignored pixel"


# ---- 3. saturated logits -------------------------------------------------------------------------------------------------------
def test_saturated_logits(dev):
    gh = _hold_to_fp64("saturated", dev, check_grad=False)
    _, _, lab = _case("saturated")
    assert bool(torch.isfinite(gh).all())
    assert bool((gh * (lab == 5)[:, None]).eq(0).all())


# ---- 4. degenerate cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [{}, {"per_image": True}, {"classes_to_consider": "all"}])
def test_all_pixels_ignored(dev, cfg):
    x = torch.randn(2, 19, 24, 40, generator=torch.Generator().manual_seed(3))
    loss, grad = _run(cfg, x, torch.full((2, 24, 40), 19), dev, hip=True)
    assert loss.item() == 0.0
    assert bool(grad.eq(0).all())


def test_exactly_one_class_present(dev):
    _hold_to_fp64("one_class_present", dev)


# ---- 5. no host synchronisation ------------------------------------------------------------------------------------------------
def test_no_host_sync(dev):
    cfg, x, lab = _case("city_2_per_image")
    m = _module(cfg)
    xd, ld = x.to(dev), lab.to(dev)
    m(xd.clone().requires_grad_(True), ld).backward()          # loads the library, fills the allocator's pools
    xg = xd.clone().requires_grad_(True)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m(xg, ld).backward()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(xg.grad).all())


# ---- 6. bitwise reproducibility ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["city_2_per_image", "city_1"])
def test_bitwise_reproducible(dev, name):
    cfg, x, lab = _case(name)
    if name == "city_1":
        x, lab = torch.cat([x, x.flip(0, 3)]), torch.cat([lab, lab.flip(0, 2)])          # 2 x 19 x 96 x 160, not per image
    a, b = _run(cfg, x, lab, dev, hip=True), _run(cfg, x, lab, dev, hip=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 7. through LossWrapper ----------------------------------------------------------------------------------------------------
def test_through_loss_wrapper(dev):
    from mscs_amd.losses import LossWrapper
    z = np.load(os.path.join(GOLDEN, "G10_lovasz.npz"))
    x, lab = torch.from_numpy(z["logits"]).to(dev), torch.from_numpy(z["label"].astype(np.int64)).to(dev)
    base = {"losses": {"CrossEntropyLoss": 1, "LovaszSoftmax": 0.5}, "device": dev, "dataset": "CITYSCAPES", "experiment": 1}
    direct = _module({})(x, lab)
    lw = LossWrapper(dict(base))
    total = lw(x.clone().requires_grad_(True), lab)
    assert torch.equal(lw.loss_vals["LovaszSoftmax"], 0.5 * direct)
    assert torch.allclose(total, lw.loss_vals["CrossEntropyLoss"] + lw.loss_vals["LovaszSoftmax"])
    total.backward()
    off = LossWrapper(dict(base, dc_off_at_epoch=5))
    off(x, lab, epoch=2)
    assert off.loss_vals["LovaszSoftmax"].item() == 0.0
    off(x, lab, epoch=5)
    assert torch.equal(off.loss_vals["LovaszSoftmax"], 0.5 * direct)
