"""Global multi-head self-attention core (reference models/Transformers.py:27-44) on libdcl_attn.so (csrc/dcl_attn.hip):
``attention(qkv, heads, scale)`` maps the qkv Linear's output [B, N, 3 C] to [B, N, C] without an N x N tensor, forward and
backward; ``attention_eager`` is the reference's own composition (CPU, other dtypes, shapes the kernels do not take, or
``debug.cfg.attn_hip`` off)."""
import torch
import torch.nn.functional as F

from ..debug import cfg as _dbg


def attention_eager(qkv: torch.Tensor, heads: int, scale: float) -> torch.Tensor:
    """The reference's arithmetic, operation by operation (it materialises the [B, heads, N, N] scores)."""
    B, N, C3 = qkv.shape
    C = C3 // 3
    qkv = qkv.reshape(B, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    attn = (q @ k.transpose(-2, -1)) * scale
    attn = attn.softmax(dim=-1)
    return (attn @ v).transpose(1, 2).reshape(B, N, C)


class _Attention(torch.autograd.Function):
    """out = softmax(scale q k^T) v per image and head on dat_attn_fwd; the backward (dat_attn_bwd) recomputes the scores from
    the saved log-sum-exp and writes all of dqkv."""

    @staticmethod
    def forward(ctx, qkv, heads, scale):
        from .. import _lib_attn as la
        L = la.lib()
        B, N, C3 = qkv.shape
        C = C3 // 3
        D = C // heads
        dev = qkv.device
        out = torch.empty((B, N, C), dtype=torch.float32, device=dev)
        lse = torch.empty((B, heads, N), dtype=torch.float32, device=dev)
        nbytes = la.workspace_bytes(B, N, heads, D, False)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        la.check(L.dat_attn_fwd(la.ptr(qkv), B, N, heads, D, float(scale), la.ptr(ws), nbytes, la.ptr(out), la.ptr(lse),
                                la.stream_ptr(dev)), "dat_attn_fwd")
        la.calls["fwd"] += 1
        ctx.save_for_backward(qkv, out, lse)
        ctx.heads, ctx.scale = heads, float(scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        from .. import _lib_attn as la
        qkv, out, lse = ctx.saved_tensors
        B, N, C3 = qkv.shape
        D = C3 // 3 // ctx.heads
        dev = qkv.device
        dout = dout.contiguous()
        dqkv = torch.empty_like(qkv)
        nbytes = la.workspace_bytes(B, N, ctx.heads, D, True)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        la.check(la.lib().dat_attn_bwd(la.ptr(qkv), la.ptr(out), la.ptr(lse), la.ptr(dout), B, N, ctx.heads, D, ctx.scale,
                                       la.ptr(ws), nbytes, la.ptr(dqkv), la.stream_ptr(dev)), "dat_attn_bwd")
        la.calls["bwd"] += 1
        return dqkv, None, None


def attention_hip_applies(qkv: torch.Tensor, heads: int) -> bool:
    if not (_dbg.attn_hip and qkv.is_cuda and qkv.dtype == torch.float32 and qkv.dim() == 3
            and not torch.is_autocast_enabled()):
        return False
    from .. import _lib_attn as la
    B, N, C3 = qkv.shape
    C = C3 // 3
    return C3 == 3 * C and C % heads == 0 and la.supported(B, N, heads, C // heads)


def attention(qkv: torch.Tensor, heads: int, scale: float) -> torch.Tensor:
    """[B, N, 3 C] -> [B, N, C]: the HIP kernels where they apply (a missing library is an error then), else the composition."""
    if attention_hip_applies(qkv, heads):
        return _Attention.apply(qkv.contiguous(), heads, scale)
    return attention_eager(qkv, heads, scale)


def token_linear(x2: torch.Tensor, weight: torch.Tensor, bias):
    """x2 [M, K] weight[N, K]^T + bias on the split-f16 GEMM where TokenLinear would take it, else F.linear."""
    from . import ops_linear as ol
    if (ol.TokenLinear.f16x3 and x2.is_cuda and x2.dtype == torch.float32 and weight.dtype == torch.float32
            and weight.requires_grad and torch.is_grad_enabled() and not torch.is_autocast_enabled()
            and ol._token_gemm_ok(x2, weight)):
        return ol._TokenLinear.apply(x2, weight, bias)
    return F.linear(x2, weight, bias)


def is_pixel_major(x: torch.Tensor) -> bool:
    """An [n, c, h, w] map whose memory is [n, h, w, c] rows (channels-last strides) and not also NCHW-contiguous."""
    return x.dim() == 4 and not x.is_contiguous() and x.permute(0, 2, 3, 1).is_contiguous()


def conv1x1_pixel_major(x: torch.Tensor, conv: torch.nn.Conv2d) -> torch.Tensor:
    """A plain 1x1 convolution of a pixel-major map as a Linear over its token rows; the result is pixel-major as well."""
    from . import amax as _am
    n, c, h, w = x.shape
    rows = _am.carry(x, x.permute(0, 2, 3, 1).reshape(n * h * w, c))
    y = token_linear(rows, conv.weight.view(conv.out_channels, c), conv.bias)
    return _am.carry(y, y.view(n, h, w, conv.out_channels).permute(0, 3, 1, 2))
