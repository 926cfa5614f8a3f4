"""The HRNet head's norm folded into its classifier (reference models/HRNet.py:596-600: conv3x3 -> BatchNorm2d -> conv1x1, no activation
in between): conv1x1(bn(z), W) = (W diag(sc)) z + W sh -- models/ops_head.py _HeadNormClassifier, csrc/dcl_bn.hip k_head_norm_dz.
Against nn.BatchNorm2d + nn.Conv2d evaluated in float64 on the CPU: logits, the input gradient, the three parameter gradients and the
running statistics; and against this package's own unfolded path (the norm writes its output, the classifier reads it)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _case(shape, k, seed):
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    z = torch.randn(shape, generator=g) * 1.3 + 0.4 * torch.randn(1, c, 1, 1, generator=g)     # per-channel means of the size of the spread
    gl = torch.randn(n, k, h, w, generator=g) * 1e-3
    wt = torch.randn(k, c, 1, 1, generator=g) * (1.0 / c) ** 0.5
    gamma = torch.rand(c, generator=g) + 0.5
    gamma[::7] *= -1.0
    beta = torch.randn(c, generator=g) * 0.3
    return z, gl, wt, gamma, beta


class _DzProbe(torch.autograd.Function):
    """Identity in front of the head: its backward is handed dz exactly as the head convolution's backward would be (the tensor
    the head's backward returned, with its absmax tag), and records it with the tag into ``seen``."""

    @staticmethod
    def forward(ctx, x, seen):
        ctx.seen = seen
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        from mscs_amd.models.amax import tag_of
        ctx.seen.append((g, tag_of(g)))
        return g, None


def _assert_dz_tag(probe, exact):
    """The dz tag is present; its maximum is max|dz| exactly (fold) or at least that (a tag from elsewhere may be a bound)."""
    assert len(probe) == 1
    dz, t = probe[0]
    assert t is not None
    want = dz.abs().max().item()
    got = t.max().item()
    assert (got == want) if exact else (got >= want), (got, want)


def _reference64(z, gl, wt, gamma, beta, momentum=0.1):
    c, k = z.shape[1], wt.shape[0]
    bn = torch.nn.BatchNorm2d(c, momentum=momentum).double()
    conv = torch.nn.Conv2d(c, k, 1, bias=False).double()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); conv.weight.copy_(wt)
    zr = z.double().requires_grad_(True)
    out = conv(bn(zr))
    out.backward(gl.double())
    return out.detach(), zr.grad, bn.weight.grad, bn.bias.grad, conv.weight.grad, bn.running_mean, bn.running_var


# (N, C, H, W), K: the benchmark's head in small (720 channels, 19 classes), ragged pixel counts, K = 1 / a multiple of four / the maximum
@pytest.mark.parametrize("shape,k", [((2, 720, 16, 32), 19), ((3, 48, 7, 12), 19), ((1, 96, 5, 4), 1), ((2, 64, 9, 20), 20),
                                     ((2, 32, 8, 8), 32), ((12, 144, 32, 64), 19)])
def test_folded_head_norm_matches_float64(dev, shape, k):
    from mscs_amd.models import fused_bn, ops
    z, gl, wt, gamma, beta = _case(shape, k, seed=sum(shape) + k)
    want = _reference64(z, gl, wt, gamma, beta)
    c = shape[1]
    bn = fused_bn.FusedBatchNorm2d(c, momentum=0.1).to(dev)
    conv = torch.nn.Conv2d(c, k, 1, bias=False).to(dev)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); conv.weight.copy_(wt)
    bn_w, conv_w = copy.deepcopy(bn), copy.deepcopy(conv)
    zf = z.to(dev).requires_grad_(True)
    assert ops.head_norm_classifier_ok(zf, bn, conv)
    probe = []
    out = ops.head_norm_classifier(_DzProbe.apply(zf, probe), bn, conv)
    out.backward(gl.to(dev))
    got = (out.detach(), zf.grad, bn.weight.grad, bn.bias.grad, conv.weight.grad, bn.running_mean, bn.running_var)
    names = ("logits", "dz", "dgamma", "dbeta", "dW", "running_mean", "running_var")
    for name, a, b in zip(names, want, got):
        scale = max(a.abs().max().item(), 1e-12)
        err = (a - b.double().cpu()).abs().max().item() / scale
        assert err <= 2e-5, (name, shape, k, err)
    assert int(bn.num_batches_tracked.item()) == 1
    # the unfolded path of this package on the same inputs: the same numbers up to fp32 round-off of a different summation order
    zu = z.to(dev).requires_grad_(True)
    out_u = conv_w(bn_w(zu))
    out_u.backward(gl.to(dev))
    for name, a, b in (("logits", out_u.detach(), out.detach()), ("dz", zu.grad, zf.grad), ("dgamma", bn_w.weight.grad, bn.weight.grad),
                       ("dW", conv_w.weight.grad, conv.weight.grad)):
        assert (a - b).abs().max().item() <= 3e-5 * max(a.abs().max().item(), 1e-12), name
    # the absmax side channel of dz (the head convolution's data / weight gradients read it instead of a pass over dz): exact
    _assert_dz_tag(probe, exact=True)


def test_hrnet_head_takes_the_folded_path_and_eval_mode_does_not(dev):
    """`HRNet._head_tail`: training mode -> one _HeadNormClassifier node and no norm output; evaluation mode -> the modules as they are
    (running statistics), same logits as the reference composition."""
    import importlib
    from mscs_amd.models import ops
    H = importlib.import_module("mscs_amd.models.HRNet")
    cfg = {"model": "HRNet", "backbone": "hrnet18", "sync_bn": False, "pretrained": False, "align_corners": True, "dataset": "CITYSCAPES",
           "ms_projector": {"mlp": [[1, -1, 1]], "scales": 2, "d": 32, "use_bn": True}}
    torch.manual_seed(0)
    m = H.HRNet(cfg, 1).to(dev)
    z = torch.randn(2, m.cls_head[1].num_features, 16, 32, device=dev, requires_grad=True)
    m.train()
    out = m._head_tail(z)
    assert type(out.grad_fn).__name__ == "_HeadNormClassifierBackward"
    out = m._head_tail(z)               # the second call reads the guard the first one filled (ops_head.FOLD_MAX_MEAN_RATIO)
    assert type(out.grad_fn).__name__ == "_HeadNormClassifierBackward"
    m.eval()
    with torch.no_grad():
        a = m._head_tail(z)
        b = m.cls_head[2](m.cls_head[1](z))
    assert torch.equal(a, b)
    keep = ops.FOLD_HEAD_NORM
    try:
        ops.FOLD_HEAD_NORM = False
        m.train()
        assert type(m._head_tail(z).grad_fn).__name__ != "_HeadNormClassifierBackward"
    finally:
        ops.FOLD_HEAD_NORM = keep


def _ratio_case(shape, k, r, seed):
    """z with per-channel means of r x the channel's std (random sign), negative gamma on every seventh channel"""
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    std = torch.rand(1, c, 1, 1, generator=g) + 0.5
    sign = torch.where(torch.rand(1, c, 1, 1, generator=g) < 0.5, -1.0, 1.0)
    z = torch.randn(shape, generator=g) * std + sign * r * std
    gl = torch.randn(n, k, h, w, generator=g) * 1e-3
    wt = torch.randn(k, c, 1, 1, generator=g) * (1.0 / c) ** 0.5
    gamma = torch.rand(c, generator=g) + 0.5
    gamma[::7] *= -1.0
    beta = torch.randn(c, generator=g) * 0.3
    return z, gl, wt, gamma, beta


def _head_tail_at_ratio(dev, shape, k, r):
    """HRNet._head_tail in training mode after one warm-up call on the same inputs, running statistics started at the data's:
    the seven outputs' errors (of max) against float64, the autograd node it took, and the dz probe."""
    import importlib
    import types
    from mscs_amd.models import fused_bn
    from mscs_amd.models.ops import DirectConv2d
    H = importlib.import_module("mscs_amd.models.HRNet")
    z, gl, wt, gamma, beta = _ratio_case(shape, k, r, seed=sum(shape) + k)
    c = shape[1]
    bn = fused_bn.FusedBatchNorm2d(c, momentum=0.1).to(dev)
    cls = DirectConv2d(c, k, 1, bias=False).to(dev)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); cls.weight.copy_(wt)
        bn.running_mean.copy_(z.double().mean((0, 2, 3)).float()); bn.running_var.copy_(z.double().var((0, 2, 3)).float())
    head = types.SimpleNamespace(cls_head=torch.nn.Sequential(torch.nn.Identity(), bn, cls).train())
    zd = z.to(dev)
    H.HRNet._head_tail(head, zd)                                    # warm-up: the guard sees this layer's statistics
    rm0, rv0 = bn.running_mean.double().cpu(), bn.running_var.double().cpu()
    bn.weight.grad = bn.bias.grad = cls.weight.grad = None
    zf = zd.clone().requires_grad_(True)
    probe = []
    out = H.HRNet._head_tail(head, _DzProbe.apply(zf, probe))
    node = type(out.grad_fn).__name__
    out.backward(gl.to(dev))
    ref = torch.nn.BatchNorm2d(c, momentum=0.1).double()
    conv = torch.nn.Conv2d(c, k, 1, bias=False).double()
    with torch.no_grad():
        ref.weight.copy_(gamma); ref.bias.copy_(beta); conv.weight.copy_(wt); ref.running_mean.copy_(rm0); ref.running_var.copy_(rv0)
    zr = z.double().requires_grad_(True)
    o64 = conv(ref(zr))
    o64.backward(gl.double())
    want = (o64.detach(), zr.grad, ref.weight.grad, ref.bias.grad, conv.weight.grad, ref.running_mean, ref.running_var)
    got = (out.detach(), zf.grad, bn.weight.grad, bn.bias.grad, cls.weight.grad, bn.running_mean, bn.running_var)
    names = ("logits", "dz", "dgamma", "dbeta", "dW", "running_mean", "running_var")
    errs = {nm: (a - b.double().cpu()).abs().max().item() / max(a.abs().max().item(), 1e-12) for nm, a, b in zip(names, want, got)}
    return errs, node, probe


# (N, C, H, W), K: the benchmark's head at a reduced batch; channel counts that are not multiples of four on small ragged maps, where
# dcl_head_norm_dz splits the channels into groups of 10 (four groups for 37, fifteen for 150) that end inside a four-channel trip
_RATIO_SHAPES = [((4, 720, 64, 128), 19), ((3, 37, 10, 12), 19), ((2, 150, 6, 20), 7)]


@pytest.mark.parametrize("r", [0.3, 3.0, 30.0, 300.0])
@pytest.mark.parametrize("shape,k", _RATIO_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_head_tail_at_large_channel_means_against_float64(dev, shape, k, r):
    """The fold's products run on the uncentred z, so its fp32 error grows with r = |mean| / std of the norm's channels.  Measured
    before the guard (the fold forced at every r, worst of the seven outputs, of max, against float64):

        r                    0.3      1        3        10       30       100      300
        (4, 720, 64, 128)    1.2e-6   1.7e-6   2.9e-6   8.3e-6   2.7e-5   9.6e-5   2.6e-4
        (3, 37, 10, 12)      2.3e-7   3.0e-7   8.5e-7   2.6e-6   6.5e-6   2.2e-5   8.9e-5
        (2, 150, 6, 20)      3.3e-7   3.6e-7   8.6e-7   3.1e-6   7.9e-6   2.7e-5   7.3e-5
        unfolded, worst      2.4e-7 ... 1.5e-5 at r = 300 (4 x 720 x 64 x 128, dW)

    (the logits, dgamma and dW grow about linearly in r; dz, dbeta and the running statistics stay flat).  The benchmark's head
    leaves 2e-5 near r = 20; ops_head.FOLD_MAX_MEAN_RATIO = 8 refuses the fold above that with a margin of 2.5, and cls(bn(z)) is
    centred on the running mean.  After one warm-up call: all seven outputs within 2e-5 of float64 at every r, the fold still
    taken for r <= 3, the dz tag exact on the fold and a bound on the fallback."""
    errs, node, probe = _head_tail_at_ratio(dev, shape, k, r)
    print(shape, k, r, node, {nm: f"{e:.2e}" for nm, e in errs.items()})
    for nm, e in errs.items():
        assert e <= 2e-5, (nm, shape, r, e, node)
    folded = node == "_HeadNormClassifierBackward"
    if r <= 3:
        assert folded
    _assert_dz_tag(probe, exact=folded)


def test_head_hooks_fire_and_see_the_unfolded_tensors(dev):
    """Forward hooks on the head's norm and classifier fire (the fold calls neither module, so a hooked head is not folded); the
    output is bitwise that of the unfolded path, and the norm's hook receives the norm's written output."""
    import importlib
    import types
    from mscs_amd.models import fused_bn, ops
    from mscs_amd.models.ops import DirectConv2d
    H = importlib.import_module("mscs_amd.models.HRNet")
    z, gl, wt, gamma, beta = _case((2, 96, 16, 32), 19, seed=3)
    bn = fused_bn.FusedBatchNorm2d(96).to(dev)
    cls = DirectConv2d(96, 19, 1, bias=False).to(dev)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); cls.weight.copy_(wt)
    head = types.SimpleNamespace(cls_head=torch.nn.Sequential(torch.nn.Identity(), bn, cls).train())
    zd = z.to(dev)
    state = copy.deepcopy(head.cls_head.state_dict())
    keep = ops.FOLD_HEAD_NORM
    try:
        ops.FOLD_HEAD_NORM = False
        want = H.HRNet._head_tail(head, zd)
    finally:
        ops.FOLD_HEAD_NORM = keep
    head.cls_head.load_state_dict(state)
    seen = {}
    hs = [bn.register_forward_hook(lambda m, i, o: seen.__setitem__("bn", o.detach().clone())),
          cls.register_forward_hook(lambda m, i, o: seen.__setitem__("cls", o.detach().clone()))]
    try:
        out = H.HRNet._head_tail(head, zd)
    finally:
        for h in hs:
            h.remove()
    assert type(out.grad_fn).__name__ != "_HeadNormClassifierBackward"
    assert set(seen) == {"bn", "cls"}
    assert torch.equal(out, want) and torch.equal(seen["cls"], want)
    head.cls_head.load_state_dict(state)
    assert torch.equal(seen["bn"], bn(zd).detach())
    # a global forward hook disables the fold as well
    g = torch.nn.modules.module.register_module_forward_hook(lambda m, i, o: None)
    try:
        assert not ops.head_norm_classifier_ok(zd, bn, cls)
    finally:
        g.remove()
    assert ops.head_norm_classifier_ok(zd, bn, cls)


def test_hrnet48_training_steps_keep_the_fold(dev, monkeypatch):
    """The benchmark's model (HRNet-W48 with the multi-scale projector, 512 x 1024, SGD) takes the fold in every step once the
    guard has values: one _HeadNormClassifier backward per step over four steps, and the guard's recorded ratio below the
    threshold."""
    import importlib
    from mscs_amd.models import ops_head
    H = importlib.import_module("mscs_amd.models.HRNet")
    graph = {"backbone": "hrnet48", "pretrained": False, "dataset": "CITYSCAPES", "align_corners": True,
             "ms_projector": {"mlp": [[1, -1, 1]], "scales": 2, "d": 256, "use_bn": True}}
    torch.manual_seed(0)
    m = H.HRNet(graph, 1).to(dev).train()
    opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9)
    calls = []
    orig = ops_head._HeadNormClassifier.backward
    monkeypatch.setattr(ops_head._HeadNormClassifier, "backward", staticmethod(lambda ctx, dl: calls.append(1) or orig(ctx, dl)))
    ce = torch.nn.CrossEntropyLoss(ignore_index=19)
    g = torch.Generator(device=dev).manual_seed(0)
    for step in range(4):
        img = torch.randn(1, 3, 512, 1024, device=dev, generator=g)
        lbl = torch.randint(0, 20, (1, 512, 1024), device=dev, generator=g)
        out, proj = m(img)
        opt.zero_grad()
        (ce(out, lbl) + sum(p.mean() for p in proj) * 0.0).backward()
        opt.step()
        assert len(calls) == step + 1, step
    guard = ops_head._FOLD_GUARD[m.cls_head[1]]
    guard[1].synchronize()
    assert 0.0 < guard[0].item() <= ops_head.FOLD_MAX_MEAN_RATIO
