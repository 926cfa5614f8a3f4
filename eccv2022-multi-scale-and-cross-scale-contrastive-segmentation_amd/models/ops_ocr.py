"""The OCR context core (reference models/OCR.py: SpatialGatherModule.forward and the middle of ObjectAttentionBlock2D.forward) on
libdcl_ocr.so (csrc/dcl_ocr.hip): ``gather(feats, logits, scale)`` maps [B, C, H, W] features and [B, K, H, W] logits to the
[B, C, K, 1] class representations, ``object_attention(query, key, value)`` maps [B, Ck, N] queries and [B, Ck, K] keys / values
to the [B, Ck, N] context, both without a transposed copy or a [B, N, K] tensor, forward and backward.  ``*_eager`` are the
reference's own compositions (CPU, other dtypes, shapes the kernels do not take, or ``debug.cfg.ocr_hip`` off).

The results are fresh tensors that carry no absmax tag (models/amax.py): a consumer that wants one measures it."""
import torch
import torch.nn.functional as F

from ..debug import cfg as _dbg


def gather_eager(feats: torch.Tensor, probs: torch.Tensor, scale: float = 1) -> torch.Tensor:
    """The reference's arithmetic, operation by operation: [B, C, H, W], [B, K, H, W] -> [B, C, K, 1]."""
    batch_size, k = probs.size(0), probs.size(1)
    probs = probs.view(batch_size, k, -1)
    feats = feats.view(batch_size, feats.size(1), -1)
    feats = feats.permute(0, 2, 1)
    probs = F.softmax(scale * probs, dim=2)
    return torch.matmul(probs, feats).permute(0, 2, 1).unsqueeze(3)


def object_attention_eager(query: torch.Tensor, key: torch.Tensor, value: torch.Tensor) -> torch.Tensor:
    """The reference's arithmetic on query [B, Ck, N], key / value [B, Ck, K] -> context [B, Ck, N] (contiguous)."""
    ck = query.size(1)
    query = query.permute(0, 2, 1)
    value = value.permute(0, 2, 1)
    sim_map = torch.matmul(query, key)
    sim_map = (ck ** -.5) * sim_map
    sim_map = F.softmax(sim_map, dim=-1)
    context = torch.matmul(sim_map, value)
    return context.permute(0, 2, 1).contiguous()


def _workspace(la, op, b, c, k, n, dev):
    nbytes = la.workspace_bytes(op, b, c, k, n)
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev), nbytes


class _Gather(torch.autograd.Function):
    """ctx[B, K, C] = softmax_N(scale logits) x^T on dco_gather_fwd; the backward (dco_gather_bwd) reads x once and writes dx and
    dlogits in full from the saved per-(image, class) maximum and sum."""

    @staticmethod
    def forward(ctx, x, logits, scale):
        from .. import _lib_ocr as la
        L = la.lib()
        B, C, N = x.shape
        K = logits.shape[1]
        dev = x.device
        out = torch.empty((B, K, C), dtype=torch.float32, device=dev)
        stats = torch.empty((B, K, 2), dtype=torch.float32, device=dev)
        ws, nbytes = _workspace(la, la.GATHER_FWD, B, C, K, N, dev)
        la.check(L.dco_gather_fwd(la.ptr(x), la.ptr(logits), B, C, K, N, float(scale), la.ptr(ws), nbytes, la.ptr(out),
                                  la.ptr(stats), la.stream_ptr(dev)), "dco_gather_fwd")
        la.calls["gather_fwd"] += 1
        ctx.save_for_backward(x, logits, out, stats)
        ctx.scale = float(scale)
        return out

    @staticmethod
    def backward(ctx, dctx):
        from .. import _lib_ocr as la
        x, logits, out, stats = ctx.saved_tensors
        B, C, N = x.shape
        K = logits.shape[1]
        dev = x.device
        dctx = dctx.contiguous()
        if dctx.data_ptr() % 16:
            dctx = dctx.clone()
        dx, dlogits = torch.empty_like(x), torch.empty_like(logits)
        ws, nbytes = _workspace(la, la.GATHER_BWD, B, C, K, N, dev)
        la.check(la.lib().dco_gather_bwd(la.ptr(x), la.ptr(logits), la.ptr(out), la.ptr(stats), la.ptr(dctx), B, C, K, N,
                                         ctx.scale, la.ptr(ws), nbytes, la.ptr(dx), la.ptr(dlogits), la.stream_ptr(dev)),
                 "dco_gather_bwd")
        la.calls["gather_bwd"] += 1
        return dx, dlogits, None


class _ObjectAttention(torch.autograd.Function):
    """out = val softmax_K(Ck^-0.5 q^T key)^T on dco_attn_fwd; nothing but the inputs is saved, the backward (dco_attn_bwd)
    recomputes the probabilities."""

    @staticmethod
    def forward(ctx, q, key, val):
        from .. import _lib_ocr as la
        L = la.lib()
        B, Ck, N = q.shape
        K = key.shape[2]
        dev = q.device
        out = torch.empty_like(q)
        ws, nbytes = _workspace(la, la.ATTN_FWD, B, Ck, K, N, dev)
        la.check(L.dco_attn_fwd(la.ptr(q), la.ptr(key), la.ptr(val), B, Ck, K, N, float(Ck) ** -0.5, la.ptr(ws), nbytes,
                                la.ptr(out), la.stream_ptr(dev)), "dco_attn_fwd")
        la.calls["attn_fwd"] += 1
        ctx.save_for_backward(q, key, val)
        return out

    @staticmethod
    def backward(ctx, dout):
        from .. import _lib_ocr as la
        q, key, val = ctx.saved_tensors
        B, Ck, N = q.shape
        K = key.shape[2]
        dev = q.device
        dout = dout.contiguous()
        if dout.data_ptr() % 16:
            dout = dout.clone()
        dq, dkey, dval = torch.empty_like(q), torch.empty_like(key), torch.empty_like(val)
        ws, nbytes = _workspace(la, la.ATTN_BWD, B, Ck, K, N, dev)
        la.check(la.lib().dco_attn_bwd(la.ptr(q), la.ptr(key), la.ptr(val), la.ptr(dout), B, Ck, K, N, float(Ck) ** -0.5,
                                       la.ptr(ws), nbytes, la.ptr(dq), la.ptr(dkey), la.ptr(dval), la.stream_ptr(dev)),
                 "dco_attn_bwd")
        la.calls["attn_bwd"] += 1
        return dq, dkey, dval


def _hip_tensor(t: torch.Tensor) -> bool:
    return t.is_cuda and t.dtype == torch.float32


def _aligned(*ts) -> bool:
    """the C ABI wants 16-byte aligned tensors (a contiguous view at an odd storage offset is not)"""
    return all(t.data_ptr() % 16 == 0 for t in ts)


def gather_hip_applies(feats: torch.Tensor, probs: torch.Tensor) -> bool:
    if not (_dbg.ocr_hip and _hip_tensor(feats) and _hip_tensor(probs) and feats.dim() == 4 and probs.dim() == 4
            and feats.shape[0] == probs.shape[0] and feats.shape[2:] == probs.shape[2:]
            and not torch.is_autocast_enabled()):
        return False
    from .. import _lib_ocr as la
    b, c, h, w = feats.shape
    return la.supported(b, c, probs.shape[1], h * w)


def object_attention_hip_applies(query: torch.Tensor, key: torch.Tensor, value: torch.Tensor) -> bool:
    if not (_dbg.ocr_hip and _hip_tensor(query) and _hip_tensor(key) and _hip_tensor(value) and query.dim() == 3
            and key.dim() == 3 and key.shape == value.shape and key.shape[:2] == query.shape[:2]
            and not torch.is_autocast_enabled()):
        return False
    from .. import _lib_ocr as la
    b, ck, n = query.shape
    return la.supported(b, ck, key.shape[2], n)


def gather(feats: torch.Tensor, probs: torch.Tensor, scale: float = 1) -> torch.Tensor:
    """[B, C, H, W], [B, K, H, W] -> [B, C, K, 1] (a permuted view of [B, K, C], as the reference returns it): the HIP kernels
    where they apply (a missing library is an error then), else the composition."""
    if gather_hip_applies(feats, probs):
        b, c, h, w = feats.shape
        x, logits = feats.contiguous().view(b, c, h * w), probs.contiguous().view(b, probs.shape[1], h * w)
        if _aligned(x, logits):
            return _Gather.apply(x, logits, scale).permute(0, 2, 1).unsqueeze(3)
    return gather_eager(feats, probs, scale)


def object_attention(query: torch.Tensor, key: torch.Tensor, value: torch.Tensor) -> torch.Tensor:
    """query [B, Ck, N], key / value [B, Ck, K] -> context [B, Ck, N]."""
    if object_attention_hip_applies(query, key, value):
        q, k, v = query.contiguous(), key.contiguous(), value.contiguous()
        if _aligned(q, k, v):
            return _ObjectAttention.apply(q, k, v)
    return object_attention_eager(query, key, value)
