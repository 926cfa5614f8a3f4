"""``SelfAttention``: the global multi-head self-attention block the reference's Projector appends with ``trans: true``
(reference models/Transformers.py:5-50).  Same constructor, parameter names (``qkv``, ``proj``) and state_dict keys, same
``forward(x, unflatten_output=True)``; the attention core runs on libdcl_attn.so (models/ops_attn.py) and never forms the
N x N matrix.  Dropout is never applied: the reference hard-codes ``self.dropout_rate = 0.0``.

Reference quirk, reproduced: a 4-D input is NOT transposed to tokens.  ``x.permute(0, 1, 2, 3).view(B, -1, C)`` rereads the
NCHW-contiguous memory as [B, H W, C] rows, and the result goes back as ``view(B, H, W, C).permute(0, 3, 1, 2)``: NCHW shape,
channels-last strides."""
import torch
from torch import nn

from .amax import carry
from .ops_attn import attention
from .ops_linear import TokenLinear


class SelfAttention(nn.Module):
    def __init__(self, dim, heads=1, qkv_bias=False, qk_scale=None, dropout_rate=0.0):
        super().__init__()
        self.num_heads = heads
        head_dim = dim // heads
        self.scale = qk_scale or head_dim ** -0.5
        self.qkv = TokenLinear(dim, dim * 3, bias=qkv_bias)
        self.dropout_rate = 0.0
        self.proj = TokenLinear(dim, dim)

    def forward(self, x, unflatten_output=True):
        H, W, was_flattened = -1, -1, False
        if x.dim() == 4:
            was_flattened = unflatten_output
            B, C, H, W = x.shape
            x = carry(x, x.contiguous())                  # (a fused producer may hand over other strides)
            x = carry(x, x.view(B, -1, C))                # the reference's token view of the NCHW memory
        B, N, C = x.shape
        y = self.proj(attention(self.qkv(x), self.num_heads, self.scale))
        if was_flattened:
            return carry(y, y.view(B, H, W, C).permute(0, 3, 1, 2))
        return y
