"""The global self-attention kernels (csrc/dcl_attn.hip) through the autograd Function, against an fp64 restatement from the
same fp32 inputs; run-to-run equality; no quadratic memory; Projector(trans=True) on the device against the reference's
recorded values (fixtures G14) in its three return modes; a training step of HRNet with the block in every projector head.

Tolerance (as tests/test_window_attention.py and the Lovasz tests): for each of out, dq, dk, dv
    max|HIP - fp64| / max|fp64|  <=  max(3 e_eager, 8 * 2^-23)
with e_eager the same distance of the eager fp32 composition on the same device: 3 for another order of the sums plus the dropped
lo.lo term, the floor for two split operands (each exact to 2^-22 of its absmax) plus the f32 accumulation.  Every comparison
prints its distances."""

import pytest
import torch

import _attn_golden as ag

pytestmark = pytest.mark.gpu

FLOOR = 8 * 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib, _lib_attn
    _lib.lib()
    _lib_attn.lib()
    return torch.device("cuda:0")


def _inputs(dev, B, N, heads, D, std, dominant):
    g = torch.Generator(device=dev).manual_seed(B * 1000 + N + heads * 7 + D)
    C = heads * D
    qkv = torch.randn(B, N, 3 * C, device=dev, generator=g) * std
    if dominant:
        qkv[:, 7, C:2 * C] *= 30.0                         # one key dominates every row: the running max jumps, O is rescaled
    dout = torch.randn(B, N, C, device=dev, generator=g)
    return qkv, dout


def _grads(fn, qkv, dout, heads, scale):
    x = qkv.clone().requires_grad_(True)
    out = fn(x, heads, scale)
    (g,) = torch.autograd.grad(out, x, dout.to(out.dtype))
    C = qkv.shape[-1] // 3
    return {"out": out.detach(), "dq": g[..., :C], "dk": g[..., C:2 * C], "dv": g[..., 2 * C:]}


def _hip(x, heads, scale):
    from mscs_amd.models.ops_attn import _Attention
    return _Attention.apply(x, heads, scale)


# (B, N, heads, D, std of q / k / v, qk_scale or None, one dominant key)
SHAPES = [
    (2, 1, 1, 16, 1.0, None, False),              # one token
    (2, 20, 2, 16, 1.0, None, False),             # less than a tile
    (1, 128, 1, 64, 1.0, None, False),            # exactly one query block
    (2, 129, 1, 64, 1.0, 0.37, False),            # one over; an explicit qk_scale
    (2, 35 * 57, 1, 48, 1.0, None, False),        # D no multiple of 32, many key tiles, odd tail
    (1, 300, 3, 32, 4.0, None, False),            # peaky rows: the max moves between tiles
    (1, 500, 1, 256, 1.0, None, False),           # the widest head
    (1, 300, 1, 64, 1.0, None, True),             # k[:, 7] *= 30
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s[:4]) + ("dom" if s[6] else ""))
def test_attention_matches_fp64(dev, shape):
    from mscs_amd.models.ops_attn import attention_eager
    B, N, heads, D, std, qk_scale, dominant = shape
    scale = qk_scale or D ** -0.5
    qkv, dout = _inputs(dev, B, N, heads, D, std, dominant)
    ref = _grads(attention_eager, qkv.double(), dout.double(), heads, scale)
    eager = _grads(attention_eager, qkv, dout, heads, scale)
    got = _grads(_hip, qkv, dout, heads, scale)
    torch.cuda.synchronize()
    C = heads * D
    # a reference that is identically zero (one token: dq = dk = 0) is measured against the size of the terms that cancel
    terms = D * scale * float(dout.abs().max() * qkv[..., 2 * C:].abs().max() * qkv[..., :2 * C].abs().max())
    bad = []
    for k in ("out", "dq", "dk", "dv"):
        assert bool(torch.isfinite(got[k]).all()), (shape, k, "not finite")
        den = float(ref[k].abs().max()) or terms
        e_hip = float((got[k].double() - ref[k]).abs().max()) / den
        e_eager = float((eager[k].double() - ref[k]).abs().max()) / den
        bar = max(3 * e_eager, FLOOR)
        print(f"attn {shape} {k}: hip {e_hip:.3e} eager {e_eager:.3e} ratio {e_hip / max(e_eager, 1e-30):.2f} bar {bar:.3e}")
        if not e_hip <= bar:
            bad.append((k, e_hip, e_eager, bar))
    assert not bad, (shape, bad)


def test_attention_is_bitwise_reproducible(dev):
    B, N, heads, D = 2, 35 * 57, 1, 48
    qkv, dout = _inputs(dev, B, N, heads, D, 1.0, False)
    a = _grads(_hip, qkv, dout, heads, D ** -0.5)
    b = _grads(_hip, qkv, dout, heads, D ** -0.5)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_no_quadratic_memory(dev):
    B, N, heads, D = 1, 4096, 1, 64
    qkv, dout = _inputs(dev, B, N, heads, D, 1.0, False)
    x = qkv.clone().requires_grad_(True)
    _hip(x, heads, D ** -0.5).backward(dout)              # (warm: library load, allocator pools)
    x.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = _hip(x, heads, D ** -0.5)
    out.backward(dout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    named = out.numel() * 4 + x.grad.numel() * 4          # out and dqkv (qkv and dout were allocated before the measurement)
    extra = peak - named
    print(f"attention N={N}: peak {peak} bytes over the inputs, {extra} beyond out and dqkv; an N x N fp32 matrix is {4 * N * N}")
    assert extra < 8 << 20, extra


# ---- module level: Projector(trans=True) with the reference's weights ---------------------------------------------------------

MODES = ("plain", "nhwc", "lazy")


def _module_run(g, dev, mode, hip):
    from mscs_amd.debug import cfg as dbg
    from mscs_amd.models.Projector import LazyProjection
    keep = dbg.attn_hip
    dbg.attn_hip = hip
    try:
        m = ag.build(g, dev)
        m.nhwc, m.lazy = mode == "nhwc", mode == "lazy"
        seen = []

        def finish(o):
            if mode == "lazy":
                assert isinstance(o, LazyProjection)
                seen.append(o)
                return o.materialize()
            assert torch.is_tensor(o)
            return o
        res = ag.run(m, g, dev, finish)
        return res, seen
    finally:
        dbg.attn_hip = keep


@pytest.mark.parametrize("case", ag.CASES)
def test_projector_trans_on_device_matches_the_reference(dev, case):
    from mscs_amd import _lib_attn as la
    g = ag.load(case)
    before = la.calls["fwd"], la.calls["bwd"]
    eager = ag.distances(_module_run(g, dev, "plain", False)[0], g)       # the switch off: the composition on the device
    assert before == (la.calls["fwd"], la.calls["bwd"]), "debug.cfg.attn_hip = False still called the library"
    for k, v in eager.items():
        print(f"G14 {case} eager {k}: {v:.3e}")
        assert v <= 1e-4, ("the eager path on the device is off the reference", k, v)
    first = None
    for mode in MODES:
        before = la.calls["fwd"], la.calls["bwd"]
        res, lazies = _module_run(g, dev, mode, True)
        heads_run = g["n"]
        assert (la.calls["fwd"] - before[0], la.calls["bwd"] - before[1]) == (heads_run, heads_run), "the HIP path was not taken"
        d = ag.distances(res, g)
        bad = []
        for k, v in d.items():
            bar = max(3 * eager[k], FLOOR)
            print(f"G14 {case} {mode} {k}: hip {v:.3e} eager {eager[k]:.3e} bar {bar:.3e}")
            if not v <= bar:
                bad.append((k, v, bar))
        assert not bad, (case, mode, bad)
        if first is None:
            first = res
        else:                                             # the modes agree in value
            for a, b in zip(first[0] + first[1], res[0] + res[1]):
                assert float((a - b).abs().max()) <= FLOOR * float(a.abs().max()), (case, mode)
        if mode == "lazy":
            gen = torch.Generator().manual_seed(5)
            for lz, full in zip(lazies, res[0]):
                n, d_, h, w = lz.shape
                T = 50
                pair_b = torch.randint(0, n, (T,), generator=gen).to(dev)
                pix = torch.randint(0, h * w, (T, 1), generator=gen).to(dev)
                rows = lz.rows(pair_b, pix).detach().double().cpu()
                want = full.reshape(n, d_, h * w)[pair_b.cpu(), :, pix.cpu()[:, 0]]
                c = lz.hidden.shape[1]
                # both are fp32 sums of c products in some order: the worst-case bound of such a sum, twice
                tol = 2 * c * 2.0 ** -24 * float(lz.hidden.abs().max() * lz.conv.weight.abs().max()) * c
                err = float((rows - want).abs().max())
                print(f"G14 {case} lazy rows vs map: {err:.3e} (tol {tol:.3e})")
                assert rows.shape == (T, d_) and err <= tol


def test_step_with_attention_in_every_projector_head(dev):
    """hrnet18, 64 x 64, batch 2, CE + multi-scale contrastive loss through the manager: finite loss, finite non-zero gradients
    of every attention parameter, and two runs from the same seed bitwise equal (no float atomics in the new kernels): the loss,
    the gradient of the input image (the end of every data-gradient chain, the attention blocks' included), and the gradient of
    every parameter but one kind.  The exception is not this path's: the weight gradients of hrnet18's 3 x 3 convolutions
    with a channel count that is no multiple of 16 (18, 36, 72, the head's 270) are left to the library's convolution backward (models/ops_conv.py,
    the last branch of the weight gradient), which sums with atomics.  Measured on the card, three runs each: 66 of 936 gradients
    differ from run to run WITHOUT ``trans`` and the same 66 of 945 with it (branch 0's 18 -> 18 convolutions and transition1's
    256 -> 18 / 256 -> 36, about 2e-7 of the maximum), loss and everything else equal; in a later pair of runs the head's 270 -> 270
    convolution differed as well.  tests/test_step_reproducible.py runs hrnet48, whose channel counts the package's own kernels
    take."""
    from mscs_amd import _lib_attn as la
    from mscs_amd.managers import HRNetManager
    from mscs_amd.utils import set_verbosity
    set_verbosity(40)
    S = 3
    cfg = {
        "name": "attn_step", "mode": "training", "manager": "HRNet", "cuda": True, "seed": 0, "parallel": False,
        "batch_is_global": False,
        "graph": {"model": "HRNet", "backbone": "hrnet18", "sync_bn": True, "out_stride": 4, "pretrained": False,
                  "align_corners": True,
                  "ms_projector": {"mlp": [[1, 64, 1]], "scales": S, "d": 64, "use_bn": True, "trans": True, "heads": 2}},
        "data": {"dataset": "CITYSCAPES", "experiment": 1, "batch_size": 2, "num_workers": 0, "synthetic": True,
                 "synthetic_length": 4, "transform_values": {"crop_shape": [64, 64]}},
        "loss": {"name": "LossWrapper", "losses": {"CrossEntropyLoss": 1, "DenseContrastiveLossV2_ms": 0.1},
                 "dataset": "CITYSCAPES", "experiment": 1, "temperature": 0.1, "scales": S, "weights": [1.0, 0.7, 0.4][:S],
                 "cross_scale_contrast": True, "min_views_per_class": 5, "max_views_per_class": 2500,
                 "max_features_total": 10000},
        "train": {"learning_rate": 0.01, "lr_fct": "polynomial", "optim": "SGD", "lr_batchwise": True, "epochs": 4,
                  "momentum": 0.9, "weight_decay": 0.0005},
    }
    import copy
    states = []
    for run in range(2):
        torch.manual_seed(0)
        mgr = HRNetManager(copy.deepcopy(cfg), autostart=False)
        mgr.setup()
        mgr.model.train()
        gen = torch.Generator().manual_seed(0)
        img = torch.randn(2, 3, 64, 64, generator=gen).to(dev).requires_grad_(True)
        # three classes in half-image blocks: each keeps >= 8 pixels at the coarsest scale (4 x 4), so that every scale has anchors
        lbl = torch.zeros(2, 64, 64, dtype=torch.int64)
        lbl[0, 32:], lbl[1, :32], lbl[1, 32:] = 1, 1, 2
        lbl = lbl.to(dev)
        before = la.calls["fwd"], la.calls["bwd"]
        mgr.optimiser.zero_grad(set_to_none=True)
        ret = mgr.forward_step(img, lbl)
        ret["loss"].backward()
        torch.cuda.synchronize()
        assert (la.calls["fwd"] - before[0], la.calls["bwd"] - before[1]) == (S, S), "the HIP attention was not taken"
        assert bool(torch.isfinite(ret["loss"]))
        state = {"loss": ret["loss"].detach().clone(), "d loss / d image": img.grad.detach().clone()}
        assert float(state["d loss / d image"].abs().max()) > 0
        names = [n for n, _ in mgr.model.named_parameters() if "projector_model" in n and (".qkv." in n or ".proj." in n)]
        assert len(names) == 3 * S, names
        for n, p in mgr.model.named_parameters():
            library_wgrad = p.dim() == 4 and p.shape[-1] == 3 and bool(p.shape[0] % 16 or p.shape[1] % 16)
            if p.grad is not None and not library_wgrad:
                state[n] = p.grad.detach().clone()
        for n in names:
            assert bool(torch.isfinite(state[n]).all()) and float(state[n].abs().max()) > 0, n
        states.append(state)
        del mgr
    assert states[0].keys() == states[1].keys() and len(states[0]) > 600
    bad = [k for k in states[0] if not torch.equal(states[0][k], states[1][k])]
    assert not bad, f"{len(bad)} of {len(states[0])} tensors differ between two runs, e.g. {bad[:5]}"
