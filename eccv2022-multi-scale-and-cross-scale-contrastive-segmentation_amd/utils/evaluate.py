"""Evaluation at the original label size (reference managers/HRNet_Manager.py post_process_output, the same in its OCRNet and
DeepLabv3 managers): for ADE20K and PASCAL-Context the reference cuts the ``fit_stride`` padding off the logits, resizes them
bilinearly to the image's original size and scores them against the label map that was never resized.

``evaluate_at_original`` does those steps for one image.  For CUDA fp32 logits it is one launch of libdcl_eval.so
(csrc/dcl_eval.hip) that reads the low-resolution map of an ``UpsampledLogits`` (or the dense logits) and leaves the arg-max map
and the confusion matrix: neither full-size map is formed.  Everything else takes the torch composition of the same steps."""
import torch
import torch.nn.functional as F

from ..debug import cfg as _dbg
from .metrics import _cols, out_of_range


def _hip_applies(z, label, C, h, w, Hp, Wp, rh, rw, H0, W0, cols):
    """CUDA fp32 [1, C, h, w] with the switch on and a shape dve_supported takes; a missing library is an error here."""
    if not (_dbg.eval_hip and z.is_cuda and label.is_cuda and z.dtype == torch.float32 and not torch.is_autocast_enabled()):
        return False
    from .. import _lib_eval as le
    return le.supported(C, h, w, Hp, Wp, rh, rw, H0, W0, cols)


@torch.no_grad()
def evaluate_at_original(output, label, crop, size, align_corners, dataset, label_lut=None, existing_matrix=None, return_ids=False):
    """Confusion matrix int32 [C, C] (rows = predicted class, columns = target class, plus ``existing_matrix``) of ONE image at its
    original size, with ``t_get_confusion_matrix``'s rule for the ignore column.

    ``output``: dense logits [1, C, Hp, Wp] or an ``UpsampledLogits`` (its own size and align_corners are the first resize);
    ``crop`` = (rh, rw): the rows and columns of the Hp x Wp map that hold the image (the rest is ``fit_stride`` padding);
    ``size`` = (H0, W0): the original size the crop is resized to, with ``align_corners``; ``label`` [H0, W0] or [1, H0, W0] at
    that size, through ``label_lut`` (uint8 [256]: raw id -> network id) when given.  Targets outside the class range go to
    ``utils.metrics.out_of_range(device)`` on the GPU and raise on the CPU.  With ``return_ids`` also the arg-max map uint8
    [1, H0, W0]."""
    lazy = hasattr(output, 'materialize')
    z = output.lowres if lazy else output
    assert z.dim() == 4 and z.shape[0] == 1, "one image per call: logits must be [1, C, H, W]"
    C, h, w = int(z.shape[1]), int(z.shape[2]), int(z.shape[3])
    Hp, Wp = (int(output.size[0]), int(output.size[1])) if lazy else (h, w)
    align_mid = bool(output.align_corners) if lazy else False
    rh, rw = int(crop[0]), int(crop[1])
    H0, W0 = int(size[0]), int(size[1])
    if rh < 1 or rw < 1 or rh > Hp or rw > Wp:
        raise ValueError(f"crop {(rh, rw)} does not lie inside the logits' size {(Hp, Wp)}")
    if C > 256:
        raise ValueError(f"{C} classes do not fit a uint8 map")
    if label.dim() == 3:
        assert label.shape[0] == 1, "one image per call"
        label = label[0]
    assert tuple(label.shape) == (H0, W0), f"label must be {[H0, W0]} (the original size), got {list(label.shape)}"
    cols = _cols(C, dataset, True)
    if label_lut is not None:
        label_lut = torch.as_tensor(label_lut)
        assert label_lut.dtype == torch.uint8 and tuple(label_lut.shape) == (256,), "label_lut must be uint8 [256]"
        label_lut = label_lut.to(z.device)
    label = label.to(z.device)

    if _hip_applies(z, label, C, h, w, Hp, Wp, rh, rw, H0, W0, cols):
        from .. import _lib_eval as le
        if label_lut is not None and label.dtype != torch.uint8:
            label, label_lut = label_lut[label.to(torch.int64)], None
        if label.dtype not in (torch.int64, torch.int32, torch.uint8):
            label = label.to(torch.int64)
        z, label = z.detach().contiguous(), label.contiguous()
        lut = label_lut.contiguous() if label_lut is not None else None
        cm = torch.zeros((C, cols), dtype=torch.int32, device=z.device)
        ids = torch.empty((1, H0, W0), dtype=torch.uint8, device=z.device) if return_ids else None
        le.check(le.lib().dve_evaluate(le.ptr(z), C, h, w, Hp, Wp, 1 if align_mid else 0, rh, rw, H0, W0, 1 if align_corners else 0,
                                       le.ptr(label), label.element_size(), le.ptr(lut), cols, le.ptr(cm),
                                       le.ptr(out_of_range(z.device)), le.ptr(ids), le.stream_ptr(z.device)), "dve_evaluate")
        le.calls["evaluate"] += 1
        cm = cm[:, :C]
    else:
        full = output.materialize() if lazy else output
        x = full.detach()[:, :, :rh, :rw]
        if (rh, rw) != (H0, W0):
            x = F.interpolate(x, size=(H0, W0), mode='bilinear', align_corners=bool(align_corners))
        idx = x.argmax(1)
        ids = idx.to(torch.uint8) if return_ids else None
        t = (label_lut[label.to(torch.int64)] if label_lut is not None else label).reshape(-1).to(torch.int64)
        p = idx.reshape(-1)
        bad = (t < 0) | (t >= cols)
        if z.is_cuda:                                   # counted, not synchronised on: the manager reads the counter once
            out_of_range(z.device).add_(bad.sum().to(torch.int32))
            p, t = p[~bad], t[~bad]
        elif bool(bad.any()):
            raise RuntimeError("Class values must be smaller than num_classes.")        # F.one_hot's error, as t_get_confusion_matrix
        cm = torch.bincount(p * cols + t, minlength=C * cols).view(C, cols)[:, :C].to(torch.int)
    if existing_matrix is not None:
        cm = cm + existing_matrix
    return (cm, ids) if return_ids else cm
