"""The OCR context kernels (csrc/dcl_ocr.hip) through their autograd Functions against an fp64 restatement from the same fp32
inputs; run-to-run equality; memory; the reference's recorded values (fixtures G15) on the device; training steps of OCRNet.

Tiles of the kernels (include/dcl_ocr.h): a workgroup holds DCO_TILE_N = 64 pixels with all classes padded to a multiple of 16
(compiled for 16, 32, 64, 128, 160 and 256 classes); channels go in chunks of DCO_CHUNK_C = 64 and in reduction steps of 16; sums
over N are split into at most DCO_MAX_SPLIT = 16 ranges of tiles.  The shapes below cover N = 1, below / exactly / one over a
tile, many tiles with an odd tail, every compiled class padding, channel counts below a chunk, no multiple of 32, and several chunks.

Tolerance (as tests/test_attn_hip.py): for each of ctx, dx, dlogits, out, dq, dkey, dval
    max|HIP - fp64| / max|fp64|  <=  max(3 e_eager, 8 * 2^-23)
with e_eager the same distance of the eager fp32 composition on the same device.  Where the fp64 result is identically zero (one
class: dq = dkey = 0; one pixel: dlogits = 0) the distance is measured against the size of the terms that cancel.  Every comparison
prints its distances."""
import copy
import json
import os

import pytest
import torch

from conftest import GOLDEN

import _ocr_golden as og

pytestmark = pytest.mark.gpu

FLOOR = 8 * 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib, _lib_ocr
    _lib.lib()
    _lib_ocr.lib()
    return torch.device("cuda:0")


class _switch:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from mscs_amd.debug import cfg as dbg
        self.keep, dbg.ocr_hip = dbg.ocr_hip, self.on

    def __exit__(self, *a):
        from mscs_amd.debug import cfg as dbg
        dbg.ocr_hip = self.keep


def _compare(what, got, eager, ref, terms):
    bad = []
    for k in ref:
        assert bool(torch.isfinite(got[k]).all()), (what, k, "not finite")
        den = float(ref[k].abs().max()) or terms[k]
        e_hip = float((got[k].double() - ref[k]).abs().max()) / den
        e_eager = float((eager[k].double() - ref[k]).abs().max()) / den
        bar = max(3 * e_eager, FLOOR)
        print(f"{what} {k}: hip {e_hip:.3e} eager {e_eager:.3e} ratio {e_hip / max(e_eager, 1e-30):.2f} bar {bar:.3e}")
        if not e_hip <= bar:
            bad.append((k, e_hip, e_eager, bar))
    assert not bad, (what, bad)


# ---- gather ----------------------------------------------------------------------------------------------------------------------

def _gather_inputs(dev, B, C, K, N, std, dominant):
    g = torch.Generator(device=dev).manual_seed(B * 1000 + C * 7 + K * 3 + N)
    x = torch.randn(B, C, N, 1, device=dev, generator=g)
    logits = torch.randn(B, K, N, 1, device=dev, generator=g) * std
    if dominant:
        logits[:, K // 2, N // 3] += 60.0                      # one pixel owns a class: p = 1 there, exp underflows elsewhere
    dctx = torch.randn(B, C, K, 1, device=dev, generator=g)
    return x, logits, dctx


def _gather_grads(fn, x, logits, dctx, scale):
    x, logits = x.clone().requires_grad_(True), logits.clone().requires_grad_(True)
    ctx = fn(x, logits, scale)
    dx, dl = torch.autograd.grad(ctx, (x, logits), dctx.to(ctx.dtype))
    return {"ctx": ctx.detach(), "dx": dx, "dlogits": dl}


def _gather_hip(x, logits, scale):
    from mscs_amd.models.ops_ocr import _Gather
    B, C, N, _ = x.shape
    return _Gather.apply(x.view(B, C, N), logits.view(B, logits.shape[1], N), scale).permute(0, 2, 1).unsqueeze(3)


# (B, C, K, N, std of the logits, scale, one dominant pixel)
GATHER_SHAPES = [
    (2, 16, 1, 1, 1.0, 1.0, False),               # one pixel, one class: dlogits = 0 by cancellation
    (2, 16, 5, 37, 1.0, 1.0, False),              # below a tile
    (1, 48, 19, 64, 1.0, 1.0, False),             # exactly one tile; C no multiple of 32
    (2, 48, 19, 65, 1.0, 0.5, False),             # one over; a scale other than 1
    (2, 48, 150, 35 * 57, 1.0, 1.0, False),       # many tiles, odd tail, several splits, 160-class padding
    (1, 512, 150, 300, 1.0, 1.0, False),          # the model's own width: eight channel chunks
    (1, 16, 256, 200, 1.0, 1.0, False),           # the most classes
    (1, 32, 19, 1000, 10.0, 1.0, False),          # peaky: the max moves between tiles
    (1, 32, 33, 500, 1.0, 1.0, True),             # one pixel dominates a class; 64-class padding
    (1, 80, 100, 130, 3.0, 1.0, False),           # 128-class padding, two chunks with a partial one
]


@pytest.mark.parametrize("shape", GATHER_SHAPES, ids=lambda s: "x".join(str(v) for v in s[:4]) + ("dom" if s[6] else ""))
def test_gather_matches_fp64(dev, shape):
    from mscs_amd.models.ops_ocr import gather_eager
    B, C, K, N, std, scale, dominant = shape
    x, logits, dctx = _gather_inputs(dev, B, C, K, N, std, dominant)
    ref = _gather_grads(gather_eager, x.double(), logits.double(), dctx.double(), scale)
    eager = _gather_grads(gather_eager, x, logits, dctx, scale)
    got = _gather_grads(_gather_hip, x, logits, dctx, scale)
    torch.cuda.synchronize()
    size = C * float(dctx.abs().max() * x.abs().max())
    _compare(f"gather {shape}", got, eager, ref, {"ctx": 1.0, "dx": 1.0, "dlogits": scale * size})


# ---- object attention ------------------------------------------------------------------------------------------------------------

def _attn_inputs(dev, B, Ck, K, N, std, column):
    g = torch.Generator(device=dev).manual_seed(B * 1000 + Ck * 7 + K * 3 + N + 1)
    q = torch.randn(B, Ck, N, device=dev, generator=g) * std
    key = torch.randn(B, Ck, K, device=dev, generator=g) * std
    val = torch.randn(B, Ck, K, device=dev, generator=g)
    if column:
        key[:, :, K // 3] *= 30.0                              # one class's key dominates the rows it correlates with
    dout = torch.randn(B, Ck, N, device=dev, generator=g)
    return q, key, val, dout


def _attn_grads(fn, q, key, val, dout):
    q, key, val = (t.clone().requires_grad_(True) for t in (q, key, val))
    out = fn(q, key, val)
    dq, dk, dv = torch.autograd.grad(out, (q, key, val), dout.to(out.dtype))
    return {"out": out.detach(), "dq": dq, "dkey": dk, "dval": dv}


def _attn_hip(q, key, val):
    from mscs_amd.models.ops_ocr import _ObjectAttention
    return _ObjectAttention.apply(q, key, val)


# (B, Ck, K, N, std of q and key, one key column scaled by 30)
ATTN_SHAPES = [
    (2, 16, 1, 1, 1.0, False),                    # one pixel, one class: dq = dkey = 0
    (2, 16, 5, 37, 1.0, False),
    (1, 48, 19, 64, 1.0, False),
    (2, 48, 19, 65, 1.0, False),
    (2, 48, 150, 35 * 57, 1.0, False),
    (1, 256, 150, 300, 1.0, False),               # the model's own key width: four channel chunks
    (1, 16, 256, 200, 1.0, False),
    (1, 32, 19, 1000, 3.0, False),                # peaky rows (scores of std 9 sqrt(32) / sqrt(32))
    (1, 32, 33, 500, 1.0, True),
    (1, 80, 100, 130, 1.0, False),
]


@pytest.mark.parametrize("shape", ATTN_SHAPES, ids=lambda s: "x".join(str(v) for v in s[:4]) + ("col" if s[5] else ""))
def test_object_attention_matches_fp64(dev, shape):
    from mscs_amd.models.ops_ocr import object_attention_eager
    B, Ck, K, N, std, column = shape
    q, key, val, dout = _attn_inputs(dev, B, Ck, K, N, std, column)
    ref = _attn_grads(object_attention_eager, q.double(), key.double(), val.double(), dout.double())
    eager = _attn_grads(object_attention_eager, q, key, val, dout)
    got = _attn_grads(_attn_hip, q, key, val, dout)
    torch.cuda.synchronize()
    # a reference that is identically zero (one class: dq = dkey = 0) is measured against the size of the terms that cancel
    base = Ck * Ck ** -0.5 * float(dout.abs().max() * val.abs().max())
    _compare(f"attention {shape}", got, eager, ref,
             {"out": 1.0, "dval": 1.0, "dq": base * float(key.abs().max()), "dkey": base * float(q.abs().max()) * N})


def test_all_seven_results_are_bitwise_reproducible(dev):
    B, C, K, N = 2, 48, 150, 35 * 57
    x, logits, dctx = _gather_inputs(dev, B, C, K, N, 1.0, False)
    q, key, val, dout = _attn_inputs(dev, B, C, K, N, 1.0, False)
    runs = []
    for _ in range(2):
        r = _gather_grads(_gather_hip, x, logits, dctx, 1.0)
        r.update(_attn_grads(_attn_hip, q, key, val, dout))
        runs.append(r)
    assert sorted(runs[0]) == ["ctx", "dkey", "dlogits", "dq", "dval", "dx", "out"]
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def _peak_beyond(dev, step, clear, named):
    step()                                                   # (warm: library load, allocator pools)
    clear()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    keep = step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    return peak, peak - named(keep)


def test_gather_memory(dev):
    from mscs_amd.models.ops_ocr import _Gather
    B, C, K, N = 1, 512, 19, 16384
    x, logits, dctx = _gather_inputs(dev, B, C, K, N, 1.0, False)
    x, logits, dctx = x.view(B, C, N).requires_grad_(True), logits.view(B, K, N).requires_grad_(True), dctx.view(B, C, K).permute(0, 2, 1).contiguous()

    def clear():
        x.grad = logits.grad = None

    def step():
        clear()
        ctx = _Gather.apply(x, logits, 1.0)
        ctx.backward(dctx)
        return ctx
    peak, extra = _peak_beyond(dev, step, clear, lambda ctx: 4 * (ctx.numel() + x.grad.numel() + logits.grad.numel()))
    print(f"gather N={N}: peak {peak} bytes over the inputs, {extra} beyond ctx, dx and dlogits; a copy of x is {4 * x.numel()}")
    assert extra < 4 * x.numel(), extra


def test_object_attention_memory(dev):
    B, Ck, K, N = 1, 256, 150, 16384
    q, key, val, dout = _attn_inputs(dev, B, Ck, K, N, 1.0, False)
    q, key, val = (t.requires_grad_(True) for t in (q, key, val))

    def clear():
        q.grad = key.grad = val.grad = None

    def step():
        clear()
        out = _attn_hip(q, key, val)
        out.backward(dout)
        return out
    peak, extra = _peak_beyond(dev, step, clear, lambda out: 4 * (out.numel() + q.grad.numel() + key.grad.numel() + val.grad.numel()))
    print(f"attention N={N}: peak {peak} bytes over the inputs, {extra} beyond out, dq, dkey and dval; the [N, K] scores are {4 * N * K}")
    assert extra < 4 * N * K, extra


# ---- module level: the reference's recorded values -----------------------------------------------------------------------------

@pytest.mark.parametrize("case", og.CASES)
def test_fixtures_on_device_match_the_reference(dev, case):
    """G15 on the device with the switch on; the ``calls`` counters prove that the library ran.

    The reference of the comparison is the same modules in float64 on the device, from the fixture's weights and inputs; it must
    reproduce the record to 1e-4 or to the noise the eager path shows (the record is an fp32 computation; that this package's
    modules ARE the reference's function is what tests/test_ocr_host.py holds to 1e-5 on the CPU).  Behind the kernels every
    result passes through batch norms over few samples (K x B of them for the class branch: 19 in case b, 2 in case c), which amplify fp32 round-off by a factor
    common to every path: in case c the EAGER path on the device is 1.9e-3 from the record in gx0.  So the noise of the chain is
    measured, not assumed: the record and the eager path on the device are two independent fp32 evaluations of the reference's
    own arithmetic, and the larger of their distances to float64 is the chain's fp32 noise.  All gradients share ONE forward
    pass, so their ratios are not independent draws, and the noise level is taken over the whole chain:
        ctx (written by the kernel itself)   max|HIP - fp64| / max|fp64| <= max(3 e_eager, 8 * 2^-23)     per tensor
        everything downstream                max|HIP - fp64| / max|fp64| <= 3 * max over all tensors of max(e_eager, e_record)
    Measured on the card, case b: over the 25 tensors the largest distance is 1.4e-5 for HIP, 1.3e-5 for the eager path and 1.9e-5 for
    the record; one per-tensor ratio HIP / eager is above 3 (f_down.0.weight: 1.4e-5 against 3.0e-6), twenty-four are below.  The
    per-tensor bar is held where no batch statistic amplifies: test_fixtures_with_running_statistics_hold_the_bar_per_tensor."""
    from mscs_amd import _lib_ocr as la
    g = og.load(case)
    before = dict(la.calls)
    with _switch(False):
        ref = og.run(og.build(g, dev, torch.float64), g, dev, torch.float64)
        eager_run = og.run(og.build(g, dev), g, dev)
    assert before == la.calls, "debug.cfg.ocr_hip = False still called the library"
    record, eager = og.distances(og.golden(g), ref), og.distances(eager_run, ref)
    for k, v in record.items():         # the record against float64: within 1e-4, or within the noise the eager path shows on this chain
        assert v <= max(1e-4, 3 * max(eager.values())), ("the float64 modules on the device are off the reference's record", k, v)
    with _switch(True):
        hip_run = og.run(og.build(g, dev), g, dev)
    assert {k: la.calls[k] - before[k] for k in before} == {"gather_fwd": 1, "gather_bwd": 1, "attn_fwd": 1, "attn_bwd": 1}, \
        "the HIP path was not taken"
    d = og.distances(hip_run, ref)
    chain = 3 * max(max(eager[k], record[k]) for k in d)
    bad = []
    for k, v in d.items():
        bar = max(3 * eager[k], FLOOR) if k == "ctx" else max(chain, FLOOR)
        print(f"G15 {case} {k}: hip {v:.3e} eager {eager[k]:.3e} record {record[k]:.3e} bar {bar:.3e}")
        if not v <= bar:
            bad.append((k, v, eager[k], bar))
    assert not bad, (case, bad)


@pytest.mark.parametrize("case", og.CASES)
def test_fixtures_with_running_statistics_hold_the_bar_per_tensor(dev, case):
    """The same modules, weights and inputs with the norms on their running statistics (eval mode: an affine map per channel, no
    batch statistic and so no few-sample amplification): every output and gradient, tensor by tensor, against float64 on the device,
        max|HIP - fp64| / max|fp64| <= max(3 e_eager, 8 * 2^-23)."""
    from mscs_amd import _lib_ocr as la
    g = og.load(case)
    with _switch(False):
        ref = og.run(og.build(g, dev, torch.float64, train=False), g, dev, torch.float64)
        eager = og.distances(og.run(og.build(g, dev, train=False), g, dev), ref)
    before = dict(la.calls)
    with _switch(True):
        d = og.distances(og.run(og.build(g, dev, train=False), g, dev), ref)
    assert all(la.calls[k] == before[k] + 1 for k in before), "the HIP path was not taken"
    bad = []
    for k, v in d.items():
        bar = max(3 * eager[k], FLOOR)
        print(f"G15 {case} eval {k}: hip {v:.3e} eager {eager[k]:.3e} bar {bar:.3e}")
        if not v <= bar:
            bad.append((k, v, eager[k], bar))
    assert not bad, (case, bad)


def test_forward_without_grad_takes_the_library(dev):
    from mscs_amd import _lib_ocr as la
    from mscs_amd.models import ops_ocr
    from mscs_amd.models import amax as am
    x, logits, _ = _gather_inputs(dev, 2, 32, 7, 100, 1.0, False)
    q, key, val, _ = _attn_inputs(dev, 2, 32, 7, 100, 1.0, False)
    before = dict(la.calls)
    with torch.no_grad():
        ctx = ops_ocr.gather(x, logits, 1)
        out = ops_ocr.object_attention(q, key, val)
    assert la.calls["gather_fwd"] == before["gather_fwd"] + 1 and la.calls["attn_fwd"] == before["attn_fwd"] + 1
    assert ctx.shape == (2, 32, 7, 1) and out.shape == (2, 32, 100)
    assert torch.allclose(ctx, ops_ocr.gather_eager(x, logits, 1), atol=1e-5)
    assert torch.allclose(out, ops_ocr.object_attention_eager(q, key, val), atol=1e-5)
    assert am.tag_of(ctx) is None and am.tag_of(out) is None          # no absmax tag rather than a stale one


# ---- model level -----------------------------------------------------------------------------------------------------------------

def _shipped_small():
    with open(os.path.join(GOLDEN, "reference_configs", "hrnetocr_contrastive_ADE20K.json")) as f:
        cfg = json.load(f)
    cfg["graph"].update(pretrained=False, backbone="hrnet18", dataset="ADE20K")
    cfg["loss"].update(dataset="ADE20K", experiment=1, losses={"TwoScaleLoss": 1})
    return cfg


def _library_wgrad(p):
    """The one kind of tensor excepted below: weights of 3 x 3 convolutions with a channel count that is no multiple of 16, whose
    gradient hrnet18 leaves to the library's convolution backward (atomics: not reproducible from run to run)."""
    return p.dim() == 4 and p.shape[-1] == 3 and bool(p.shape[0] % 16 or p.shape[1] % 16)


def _step(dev, state, hip, dtype=torch.float32):
    from mscs_amd.losses import LossWrapper
    from mscs_amd.models import OCRNet
    cfg = _shipped_small()
    if dtype == torch.float64:         # the same model code on stock kernels in float64: the reference of the comparison
        cfg["graph"].update(branch_conv="library", head_conv="library", conv1x1="library", fused_bn=False)
    cfg["loss"]["device"] = "cuda"
    with _switch(hip):
        model = OCRNet(config=cfg["graph"], experiment=1)
        if state is not None:
            model.load_state_dict(state, strict=True)
        state = copy.deepcopy(model.state_dict())
        model = model.to(dev).to(dtype).train()
        loss_fn = LossWrapper(cfg["loss"])
        g = torch.Generator().manual_seed(0)
        img = torch.randn(2, 3, 64, 128, generator=g).to(dev).to(dtype).requires_grad_(True)
        lbl = torch.randint(0, 150, (2, 64, 128), generator=g).to(dev)
        interm, out, feats = model(img)
        loss = loss_fn(out, lbl, interm_prediction=interm, deep_features=feats, epoch=0)
        loss.backward()
        torch.cuda.synchronize()
    res = {"loss": loss.detach().reshape(1), "interm logits": interm.detach(), "logits": out.detach(), "d loss / d image": img.grad}
    for n, p in model.named_parameters():
        if p.grad is not None:
            res["g:" + n] = p.grad.detach()
    return res, state, {n: p for n, p in model.named_parameters()}


def test_training_step_switch_on_against_off(dev):
    """OCRNet(hrnet18), 2 x 3 x 64 x 128, TwoScaleLoss (CE + CE): the step with the kernels against the step with the eager
    composition, each measured against the same step in float64 on stock kernels."""
    from mscs_amd import _lib_ocr as la
    from mscs_amd.utils import set_verbosity
    set_verbosity(40)
    torch.manual_seed(0)
    ref, state, _ = _step(dev, None, False, torch.float64)
    before = dict(la.calls)
    off, _, _ = _step(dev, state, False)
    assert before == la.calls
    on, _, params = _step(dev, state, True)
    assert all(la.calls[k] == before[k] + 1 for k in before), "the HIP path was not taken"
    excepted = [n for n, p in params.items() if _library_wgrad(p)]
    # The OCR head is everything outside the backbone and the projector.  Two of its tensors are excepted, by the same rule as the
    # backbone's: the 3 x 3 convolutions that read hrnet18's 270-channel concatenation (18 + 36 + 72 + 144: no multiple of 16),
    # whose weight gradients the library sums with atomics, with the switch on and off alike.  (With hrnet48 the concatenation has
    # 720 channels and the package's own kernels take them.)  Nothing else of the head is excepted.
    concat_readers = {"conv_high_map.0.weight", "interm_prediction_head.0.weight"}
    assert all(tuple(params[n].shape) == (512, 270, 3, 3) for n in concat_readers)
    assert len(excepted) < len(params) / 4, (len(excepted), len(params))
    in_head = [n for n in excepted if not n.startswith(("backbone.", "projector_model."))]
    assert set(in_head) == concat_readers, in_head
    assert set(ref) == set(off) == set(on)
    missing = [n for n in params if not n.startswith("projector_model") and "g:" + n not in on]
    assert not missing, missing[:5]
    bad, worst = [], (0.0, None)
    for k in ref:
        if k.startswith("g:") and k[2:] in excepted:
            continue
        den = float(ref[k].abs().max()) or 1.0
        e_on = float((on[k].double() - ref[k]).abs().max()) / den
        e_off = float((off[k].double() - ref[k]).abs().max()) / den
        bar = max(3 * e_off, FLOOR)
        if not k.startswith("g:backbone."):
            print(f"step {k}: on {e_on:.3e} off {e_off:.3e} bar {bar:.3e}")
        worst = max(worst, (e_on / bar, k))
        if not e_on <= bar:
            bad.append((k, e_on, e_off, bar))
    print(f"step: {len(ref)} tensors, {len(excepted)} excepted, worst on / bar {worst[0]:.2f} at {worst[1]}")
    assert not bad, (len(bad), bad[:8])


def test_contrastive_step(dev):
    """One manager step of OCRNet(hrnet18) with TwoScaleLoss and the multi-scale contrastive loss: finite, and every parameter
    that is not frozen has a gradient."""
    from mscs_amd import _lib_ocr as la
    from mscs_amd.managers import OCRNetManager
    from mscs_amd.utils import set_verbosity
    set_verbosity(40)
    cfg = {"name": "ocr_step", "mode": "training", "manager": "OCRNet", "cuda": True, "parallel": False, "seed": 3,
           "graph": {"model": "OCRNet", "backbone": "hrnet18", "sync_bn": False, "out_stride": 4, "pretrained": False,
                     "align_corners": True,
                     "ms_projector": {"mlp": [[1, -1, 1]], "scales": 4, "d": 64, "use_bn": True, "before_context": True}},
           "data": {"dataset": "ADE20K", "experiment": 1, "batch_size": 2, "synthetic": True, "synthetic_length": 4,
                    "transform_values": {"crop_shape": [128, 128]}},
           "loss": {"name": "LossWrapper", "temperature": 0.1, "scales": 4, "weights": [1.0, 0.7, 0.4, 0.1],
                    "cross_scale_contrast": True, "min_views_per_class": 2, "max_features_total": 600,
                    "interm": {"name": "CrossEntropyLoss", "args": [], "weight": 0.4},
                    "final": {"name": "CrossEntropyLoss", "args": [], "weight": 1.0},
                    "losses": {"TwoScaleLoss": 1.0, "DenseContrastiveLossV2_ms": 0.1}},
           "train": {"learning_rate": 0.01, "lr_fct": "polynomial", "optim": "SGD", "lr_batchwise": True, "epochs": 1}}
    mgr = OCRNetManager(cfg, autostart=False)
    mgr.setup()
    mgr.model.train()
    assert type(mgr.model).__name__ == "OCRNet"
    gen = torch.Generator().manual_seed(0)
    img = torch.randn(2, 3, 128, 128, generator=gen).to(dev)
    lbl = torch.zeros(2, 128, 128, dtype=torch.int64)
    lbl[0, 64:], lbl[1, :64], lbl[1, 64:] = 1, 1, 2            # half-image blocks: every class keeps pixels at the coarsest scale
    before = dict(la.calls)
    ret = mgr.forward_step(img, lbl.to(dev))
    ret["loss"].backward()
    torch.cuda.synchronize()
    assert all(la.calls[k] == before[k] + 1 for k in before), "the HIP path was not taken"
    assert bool(torch.isfinite(ret["loss"])) and "TwoScaleLoss" in mgr.loss.loss_vals
    assert any(k.startswith("DenseContrastiveLossV2_ms") for k in mgr.loss.loss_vals), sorted(mgr.loss.loss_vals)
    missing = [n for n, p in mgr.model.named_parameters() if p.requires_grad and p.grad is None]
    assert not missing, missing[:5]
    assert all(bool(torch.isfinite(p.grad).all()) for p in mgr.model.parameters() if p.grad is not None)
