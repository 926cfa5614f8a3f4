"""The merge of test-time-augmentation views (reference models/TTA_wrapper.py, models/TTA_wrapper_CTS.py) on libdcl_tta.so
(csrc/dcl_tta.hip), one image at a time:

  ``merge``         acc += weight * resize(unflip(resize(z -> view size)) -> image size), the view's logits never written
  ``window_accum``  canvas[window] += exp(up(z)) or exp(0.5 * (up(z) + unflip(up(zf)))) of one sliding-window crop
  ``canvas_merge``  acc += resize(canvas / window count -> image size)

``*_eager`` are the reference's own compositions in torch, operation by operation (CPU, other dtypes, shapes the kernels do not
take, ``debug.cfg.tta_hip`` off; they are also what tools/tta_time.py times the kernels against).  The plan (image-size rule,
window grid) is host arithmetic restated here from csrc/dcl_tta_plan.h; tests/test_tta_host.py holds the two together."""
import math

import torch
import torch.nn.functional as F

from ..debug import cfg as _dbg


# ---- the plan -------------------------------------------------------------------------------------------------------------------
def cts_size(H: int, W: int, base_size: int, scale: float):
    """(new_h, new_w): the longer side becomes int(base_size * scale + 0.5), the other keeps the aspect ratio."""
    long_size = int(base_size * scale + 0.5)
    if H > W:
        return long_size, int(W * long_size / H + 0.5)
    return int(H * long_size / W + 0.5), long_size


def windows_1d(n: int, crop: int, stride: int):
    """[(lo, hi), ...] of the sliding windows along an axis of length n: the last one is shifted back, and a window is shorter
    than the crop when the axis is.  Empty when the reference's count is below one."""
    count = int(math.ceil(1.0 * (n - crop) / stride)) + 1
    out = []
    for r in range(count):
        hi = min(r * stride + crop, n)
        out.append((max(int(hi - crop), 0), hi))
    return out


def counts_1d(n: int, spans):
    """windows over each of the n positions of an axis (int32 tensor); the count of a pixel is the product of its row's and its
    column's"""
    cnt = torch.zeros(n, dtype=torch.int32)
    for lo, hi in spans:
        cnt[lo:hi] += 1
    return cnt


# ---- the model's logits ---------------------------------------------------------------------------------------------------------
def view_logits(out):
    """(z, (Hm, Wm), align): the [1, C, h, w] map a model call returned and the size / flag of the bilinear resize that still has
    to be applied to it.  A plain tensor is its own full-resolution map (the resize to its own size is the identity)."""
    if hasattr(out, 'materialize'):                                  # models.ops_logits.UpsampledLogits
        return out.lowres, tuple(out.size), bool(out.align_corners)
    return out, (int(out.shape[-2]), int(out.shape[-1])), False


def full_logits(out):
    return out.materialize() if hasattr(out, 'materialize') else out


def hip_applies(x: torch.Tensor) -> bool:
    """The fused path is for one CUDA fp32 image with the switch on; the shape test comes with each call (``supported``)."""
    return bool(_dbg.tta_hip and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] == 1
                and not torch.is_autocast_enabled())


def supported(z: torch.Tensor, size, out_hw) -> bool:
    """Whether the kernels take z [1, C, h, w] resized to ``size`` and merged into a [C, H, W] accumulator; a missing library is an
    error here, not a reason for the composition."""
    from .. import _lib_tta as lt
    return bool(z.is_cuda and z.dtype == torch.float32 and z.dim() == 4 and z.shape[0] == 1
                and lt.supported(z.shape[1], z.shape[2], z.shape[3], size[0], size[1], out_hw[0], out_hw[1]))


# ---- the kernels ----------------------------------------------------------------------------------------------------------------
def merge(z, size, align_inner, flip, acc, align_outer, weight=1.0):
    """acc [C, H, W] += weight * resize(unflipW(resize(z [C, h, w] -> size)) -> H x W), in place."""
    from .. import _lib_tta as lt
    z = z.contiguous()
    assert acc.is_contiguous() and acc.dtype == torch.float32 and acc.dim() == 3 and z.dim() == 3 and z.shape[0] == acc.shape[0]
    C, h, w = z.shape
    lt.check(lt.lib().dtt_merge(lt.ptr(z), C, h, w, int(size[0]), int(size[1]), 1 if align_inner else 0, 1 if flip else 0,
                                lt.ptr(acc), acc.shape[1], acc.shape[2], 1 if align_outer else 0, float(weight),
                                lt.stream_ptr(acc.device)), "dtt_merge")
    lt.calls["merge"] += 1
    return acc


def window_accum(z, zf, crop, align_inner, canvas, h0, w0, wh, ww):
    """canvas [C, Hc, Wc][:, h0:h0+wh, w0:w0+ww] += exp(m)[:, :wh, :ww]; m = up(z) (zf None) or 0.5 * (up(z) + unflipW(up(zf))),
    up = the resize of [C, h, w] to the crop's size."""
    from .. import _lib_tta as lt
    z = z.contiguous()
    zf = None if zf is None else zf.contiguous()
    assert canvas.is_contiguous() and canvas.dtype == torch.float32 and canvas.dim() == 3 and z.dim() == 3
    assert z.shape[0] == canvas.shape[0] and (zf is None or zf.shape == z.shape)
    C, h, w = z.shape
    lt.check(lt.lib().dtt_window_accum(lt.ptr(z), lt.ptr(zf), C, h, w, int(crop[0]), int(crop[1]), 1 if align_inner else 0,
                                       lt.ptr(canvas), canvas.shape[1], canvas.shape[2], int(h0), int(w0), int(wh), int(ww),
                                       lt.stream_ptr(canvas.device)), "dtt_window_accum")
    lt.calls["window_accum"] += 1
    return canvas


def canvas_merge(canvas, rowcnt, colcnt, acc, align):
    """acc [C, H, W] += resize(canvas [C, Hc, Wc] / (rowcnt[y] * colcnt[x]) -> H x W); the counts are int32 device vectors."""
    from .. import _lib_tta as lt
    assert canvas.is_contiguous() and acc.is_contiguous() and canvas.dim() == 3 and acc.dim() == 3 and canvas.shape[0] == acc.shape[0]
    assert rowcnt.dtype == torch.int32 and colcnt.dtype == torch.int32 and rowcnt.is_contiguous() and colcnt.is_contiguous()
    assert rowcnt.numel() == canvas.shape[1] and colcnt.numel() == canvas.shape[2] and rowcnt.device == canvas.device
    C, Hc, Wc = canvas.shape
    lt.check(lt.lib().dtt_canvas_merge(lt.ptr(canvas), lt.ptr(rowcnt), lt.ptr(colcnt), C, Hc, Wc, lt.ptr(acc), acc.shape[1],
                                       acc.shape[2], 1 if align else 0, lt.stream_ptr(acc.device)), "dtt_canvas_merge")
    lt.calls["canvas_merge"] += 1
    return acc


# ---- the reference's compositions -----------------------------------------------------------------------------------------------
def _resize(t, size, align):
    return F.interpolate(t, size=[int(size[0]), int(size[1])], mode='bilinear', align_corners=bool(align))


def merge_eager(z, size, align_inner, flip, acc, align_outer, weight=1.0):
    """``merge`` as the reference composes it: the view's logits at its size, un-mirrored, resized to the image size, added."""
    y = z[None]
    if tuple(y.shape[-2:]) != (int(size[0]), int(size[1])):
        y = _resize(y, size, align_inner)
    if flip:
        y = torch.flip(y, dims=[3])
    y = _resize(y, acc.shape[-2:], align_outer)[0]
    acc += y if weight == 1.0 else weight * y
    return acc


def window_accum_eager(z, zf, crop, align_inner, canvas, h0, w0, wh, ww):
    pred = _resize(z[None], crop, align_inner)
    if zf is not None:
        pred = pred + torch.flip(_resize(zf[None], crop, align_inner), dims=[3])
        pred = pred * 0.5
    canvas[:, h0:h0 + wh, w0:w0 + ww] += pred.exp()[0, :, :wh, :ww]
    return canvas


def canvas_merge_eager(canvas, rowcnt, colcnt, acc, align):
    count = (rowcnt[:, None] * colcnt[None, :]).to(canvas.dtype)
    acc += _resize((canvas / count)[None], acc.shape[-2:], align)[0]
    return acc
