"""Sliding-window test-time augmentation with equal-size windows (reference models/TTA_wrapper_PC.py, models/TTAWrapperSlide.py) on
libdcl_slide.so (csrc/dcl_slide.hip), one image at a time:

  ``crops``   the windows of one scale, and their mirrors, as one batch read from the original image: resize, border padding,
              slices and flips are never written
  ``gather``  canvas = mean over the covering windows of exp(up(z)) or exp(0.5 * (up(z) + unflip(up(zf)))), stored once

``*_eager`` are the reference's own compositions in torch, operation by operation (CPU, other dtypes, shapes the kernels do not
take, ``debug.cfg.slide_hip`` off; they are also what tools/slide_time.py times the kernels against).  The plan (window grids,
cover counts) is host arithmetic restated here from csrc/dcl_slide_plan.h; tests/test_slide_host.py holds the two together."""
import math

import torch
import torch.nn.functional as F

from ..debug import cfg as _dbg
from .ops_tta import cts_size, windows_1d  # noqa: F401  (the size rule and the shifted-back grid are shared with TTAWrapperCTS)

MAX_WIN = 64          # DSW_MAX_WIN


# ---- the plan -------------------------------------------------------------------------------------------------------------------
def pc_windows_1d(n: int, crop: int, stride: int):
    """[(lo, hi), ...] of the PASCAL-Context windows along an axis of length n (already padded to the crop): lo = r * stride, no
    shift-back, the last window may be partial.  Empty when the reference's count is below one."""
    count = int(math.ceil(1.0 * (n - crop) / stride)) + 1
    return [(r * stride, min(r * stride + crop, n)) for r in range(count)]


def pc_strides(crop_size):
    return int(crop_size[0] * 2.0 / 3.0), int(crop_size[1] * 2.0 / 3.0)


def cover_1d(n: int, wh: int, los):
    """windows [lo, min(lo + wh, n)) over each of the n positions of an axis (a list)"""
    return [sum(1 for lo in los if lo <= i < lo + wh) for i in range(n)]


def hip_applies(x: torch.Tensor) -> bool:
    """The fused path is for one CUDA fp32 image with the switch on; the shape test comes with each scale (``supported``)."""
    return bool(_dbg.slide_hip and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] == 1
                and not torch.is_autocast_enabled())


def supported(x, num_classes, low, win, rows_lo, cols_lo, canvas_hw) -> bool:
    """Whether the kernels take one scale: x [1, Cin, H, W], R x Q windows of ``win``, logits [R * Q, num_classes, *low], canvas
    [num_classes, *canvas_hw] with every pixel under a window.  A missing library is an error here, not a reason for the
    composition."""
    from .. import _lib_slide as ls
    R, Q = len(rows_lo), len(cols_lo)
    if not ls.supported(x.shape[1], x.shape[2], x.shape[3], int(num_classes), int(low[0]), int(low[1]), int(win[0]), int(win[1]), R, Q,
                        int(canvas_hw[0]), int(canvas_hw[1])):
        return False
    return ls.plan_cover(int(canvas_hw[0]), int(win[0]), rows_lo)[0] >= 1 and ls.plan_cover(int(canvas_hw[1]), int(win[1]), cols_lo)[0] >= 1


# ---- the kernels ----------------------------------------------------------------------------------------------------------------
def crops(x, size, rows_lo, cols_lo, win, pad, mirror):
    """[R * Q * (1 + mirror), Cin, wh, ww]: window r * Q + q of the half-pixel bilinear resize of x [Cin, H, W] to ``size``, read at
    (rows_lo[r], cols_lo[q]), ``pad[c]`` beyond the resized image; with ``mirror`` the second half holds the windows mirrored
    along W."""
    from .. import _lib_slide as ls
    x = x.contiguous()
    assert x.dim() == 3 and x.dtype == torch.float32 and len(pad) == x.shape[0]
    Cin, H, W = x.shape
    R, Q = len(rows_lo), len(cols_lo)
    out = torch.empty((R * Q * (2 if mirror else 1), Cin, int(win[0]), int(win[1])), dtype=torch.float32, device=x.device)
    ls.check(ls.lib().dsw_crops(ls.ptr(x), Cin, H, W, int(size[0]), int(size[1]), ls.ints(rows_lo), R, ls.ints(cols_lo), Q, int(win[0]),
                                int(win[1]), ls.floats(pad), 1 if mirror else 0, ls.ptr(out), ls.stream_ptr(x.device)), "dsw_crops")
    ls.calls["crops"] += 1
    return out


def gather(z, zf, win, align_inner, rows_lo, cols_lo, canvas):
    """canvas [C, Hc, Wc] = mean over the windows covering each pixel of exp(m); m = up(z[n]) (zf None) or
    0.5 * (up(z[n]) + unflipW(up(zf[n]))), up = the resize of [C, h, w] to ``win``.  Stored: what the canvas held is overwritten."""
    from .. import _lib_slide as ls
    z = z.contiguous()
    zf = None if zf is None else zf.contiguous()
    R, Q = len(rows_lo), len(cols_lo)
    assert canvas.is_contiguous() and canvas.dtype == torch.float32 and canvas.dim() == 3 and z.dim() == 4 and z.dtype == torch.float32
    assert z.shape[0] == R * Q and z.shape[1] == canvas.shape[0] and (zf is None or (zf.shape == z.shape and zf.dtype == z.dtype))
    _, C, h, w = z.shape
    ls.check(ls.lib().dsw_gather(ls.ptr(z), ls.ptr(zf), C, h, w, int(win[0]), int(win[1]), 1 if align_inner else 0, ls.ints(rows_lo), R,
                                 ls.ints(cols_lo), Q, ls.ptr(canvas), canvas.shape[1], canvas.shape[2], ls.stream_ptr(canvas.device)),
             "dsw_gather")
    ls.calls["gather"] += 1
    return canvas


# ---- the reference's compositions -----------------------------------------------------------------------------------------------
def _resize(t, size, align):
    return F.interpolate(t, size=[int(size[0]), int(size[1])], mode='bilinear', align_corners=bool(align))


def pad_to(img, size, pad):
    """the reference's pad_image: a constant bottom / right border of ``pad[c]`` up to ``size``; img [1, Cin, h, w]"""
    h, w = int(img.shape[2]), int(img.shape[3])
    ph, pw = max(int(size[0]) - h, 0), max(int(size[1]) - w, 0)
    if ph == 0 and pw == 0:
        return img
    out = torch.as_tensor(list(pad), dtype=img.dtype, device=img.device).view(1, -1, 1, 1).expand(1, img.shape[1], h + ph, w + pw).clone()
    out[:, :, :h, :w] = img
    return out


def crops_eager(x, size, rows_lo, cols_lo, win, pad, mirror):
    """``crops`` as the reference composes it: the resized image, each slice, its border, its mirror."""
    img = _resize(x[None], size, False)
    plain = []
    for r in rows_lo:
        for q in cols_lo:
            plain.append(pad_to(img[:, :, r:r + int(win[0]), q:q + int(win[1])], win, pad))
    out = torch.cat(plain)
    return torch.cat([out, torch.flip(out, dims=[3])]) if mirror else out


def gather_eager(z, zf, win, align_inner, rows_lo, cols_lo, canvas):
    """``gather`` as the reference composes it: per window the resized logits, the mean with the un-mirrored ones, exp, ``+=`` into
    the zero-filled canvas and into a count map, then the division."""
    C, Hc, Wc = canvas.shape
    wh, ww = int(win[0]), int(win[1])
    preds = torch.zeros_like(canvas)
    count = torch.zeros((1, Hc, Wc), dtype=canvas.dtype, device=canvas.device)
    n = 0
    for r in rows_lo:
        for q in cols_lo:
            pred = _resize(z[n:n + 1], win, align_inner)
            if zf is not None:
                pred = pred + torch.flip(_resize(zf[n:n + 1], win, align_inner), dims=[3])
                pred = pred * 0.5
            h1, w1 = min(r + wh, Hc), min(q + ww, Wc)
            preds[:, r:h1, q:w1] += pred.exp()[0, :, :h1 - r, :w1 - q]
            count[:, r:h1, q:w1] += 1
            n += 1
    canvas.copy_(preds / count)
    return canvas
