"""Shared by tests/test_pred_host.py, tests/test_pred_hip.py and tests/test_pred_footprint.py: the shapes, the inputs, the float64
evaluation of the resize and the rule that leaves near-ties out."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

#         (C, h, w, H, W): odd sizes, widths that are no multiple of the run, non-integer factors, the class limits, the identity
SHAPES = [(1, 3, 5, 9, 11), (19, 5, 7, 17, 23), (19, 8, 12, 32, 48), (150, 13, 9, 50, 33), (256, 4, 6, 16, 22), (19, 16, 24, 16, 24)]
IDENTITY = SHAPES[-1]
MARGIN = 1e-5       # x max|z|: about 20 x what four fp32 roundings of a convex combination can move a difference of two values
MAX_LEFT_OUT = 0.01


def logits(C, h, w, n=1):
    return torch.randn(n, C, h, w, generator=torch.Generator().manual_seed(1000 * C + h))


def src_index(in_size, out_size, align, dst):
    """The rule of include/dcl_pred.h in fp32, written directly: (i0, i1, l0, l1)"""
    f = np.float32
    if align:
        scale = f(in_size - 1) / f(out_size - 1) if out_size > 1 else f(0)
        s = scale * f(dst)
    else:
        scale = f(in_size) / f(out_size)
        s = max(scale * (f(dst) + f(0.5)) - f(0.5), f(0))
    i0 = min(int(s), in_size - 1)
    l1 = f(s) - f(i0)
    return i0, i0 + (1 if i0 < in_size - 1 else 0), f(1) - l1, l1


def resize_np(z, H, W, align):
    """The same resize in float64 numpy: z [N, C, h, w] -> [N, C, H, W]"""
    z = np.asarray(z, dtype=np.float64)

    def axis(n_in, n_out):
        d = np.arange(n_out, dtype=np.float64)
        if align:
            src = ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0) * d
        else:
            src = np.maximum(n_in / n_out * (d + 0.5) - 0.5, 0.0)
        i0 = np.minimum(src.astype(np.int64), n_in - 1)
        l1 = src - i0
        return i0, i0 + (i0 < n_in - 1), 1.0 - l1, l1
    y0, y1, ly0, ly1 = axis(z.shape[2], H)
    x0, x1, lx0, lx1 = axis(z.shape[3], W)
    top = z[:, :, y0][:, :, :, x0] * lx0 + z[:, :, y0][:, :, :, x1] * lx1
    bot = z[:, :, y1][:, :, :, x0] * lx0 + z[:, :, y1][:, :, :, x1] * lx1
    return top * ly0[:, None] + bot * ly1[:, None]


def decided(full, zmax):
    """(arg-max [N, H, W] int64, mask of the pixels whose float64 top-two margin is at least MARGIN * max|z|) of float64 logits"""
    full = torch.as_tensor(full)
    if full.shape[1] == 1:
        return torch.zeros(full[:, 0].shape, dtype=torch.int64), torch.ones(full[:, 0].shape, dtype=torch.bool)
    top = full.topk(2, dim=1)
    return full.argmax(1), (top.values[:, 0] - top.values[:, 1]) >= MARGIN * zmax


@functools.lru_cache(maxsize=None)
def reference(C, h, w, H, W, align, n=1):
    """(z fp32, arg-max of the float64 evaluation of the same resize in torch on the CPU, mask of the decided pixels), computed once"""
    z = logits(C, h, w, n)
    full = z.double() if (h, w) == (H, W) else F.interpolate(z.double(), size=(H, W), mode="bilinear", align_corners=bool(align))
    ids, ok = decided(full, float(z.abs().max()))
    assert float((~ok).float().mean()) <= MAX_LEFT_OUT
    return z, ids, ok


def tables(seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (256,), generator=g, dtype=torch.uint8), torch.randint(0, 256, (256, 3), generator=g, dtype=torch.uint8)
