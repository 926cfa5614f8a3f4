"""Online hard example mining for the pixel-wise cross-entropy: the public HRNet ``OhemCrossEntropy`` (the loss of its Cityscapes
recipe: threshold 0.9, at least 131072 pixels kept per GPU), the name losses/LossWrapper.py dispatches on.

With logits ``z [N,C,H,W]`` at the label size, labels ``t``, class weights ``w`` (or none), ``ignore``, ``thresh``, ``min_kept``:

    valid_i = 0 <= t_i < C and t_i != ignore
    p_i = softmax(z_i)[t_i],   l_i = w[t_i] (lse_i - z_i[t_i])                 (valid pixels)
    n = #valid,  k = min(min_kept, n - 1),  v = sort(p)[k],  thr = max(v, thresh)
    kept_i = valid_i and p_i < thr   (strict),   m = #kept
    loss = sum_kept l_i / m          (a plain mean: the weights are in the numerator only)

The gradient treats ``thr`` and the mask as constants.  Under DDP the mining is per rank, as in the public recipe.

Two deviations from the public code:
  * n == 0 (only void pixels): it raises IndexError; here the loss is a zero tensor with zero gradient, as in LovaszSoftmax;
  * m == 0 (a single valid pixel at or above ``thresh``, or a tie group that starts at rank 0): it returns the NaN mean of nothing;
    here the sum is divided by max(m, 1): the loss is 0 with zero gradient.
Non-finite logits are outside the contract (a NaN p orders last and is never kept).

On a GPU the loss runs on kernels (csrc/dcl_ohem.hip, C ABI include/dcl_ohem.h) between the two entries of the fused up-sampling +
cross-entropy: ``dcl_upsample_ce_fwd`` gives the log-sum-exp and the arg-max map from the low-resolution logits, ``doh_target_prob``
the maps p and l, ``doh_select`` the exact k-th smallest p by a three-pass radix select, ``doh_reduce`` the masked mean and the
hard-target map (the label where kept, the ignore id elsewhere) that ``dcl_upsample_ce_bwd`` then takes as its target.  The
full-resolution logits are never written, nothing is sorted and nothing returns to the host; 20 bytes per pixel of maps.  That path is
taken for fp32 CUDA logits with 1 <= C <= 255, N H W < 2^31 and the shape limits of the two reused entries (``_lib_ohem.supported``),
unless ``DCL_OHEM_HIP=0`` (debug.cfg.ohem_hip); everything else, CPU tensors included, takes ``ohem_reference`` below."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..utils import DATASETS_INFO
from .TwoScaleLoss import CITYSCAPES_CLASS_WEIGHTS


def ohem_reference(z, t, w, ignore, thresh, min_kept, size=None, align_corners=False, dtype=None, kept=None):
    """The torch composition of the arithmetic above: ``(loss, thr, kept, p)`` with ``kept`` bool [N,H,W] and ``p`` [N,H,W] (NaN at
    invalid pixels).  ``size``: up-sample ``z`` first (F.interpolate, bilinear); ``dtype``: compute in it (float64: the tests'
    reference); a given ``kept`` overrides the selection.  No boolean indexing: the invalid pixels sort behind everything as +inf."""
    if dtype is not None:
        z = z.to(dtype)
    if size is not None:
        z = F.interpolate(z, size=tuple(size), mode='bilinear', align_corners=align_corners)
    C = z.shape[1]
    t = t.long()
    valid = (t >= 0) & (t < C) & (t != ignore)
    tc = torch.where(valid, t, torch.zeros_like(t))
    logp = F.log_softmax(z, dim=1).gather(1, tc.unsqueeze(1)).squeeze(1)           # z_t - lse
    l = -logp if w is None else -logp * w.to(device=z.device, dtype=z.dtype)[tc]
    pd = logp.detach().exp()
    n = valid.sum()
    k = torch.clamp(torch.clamp(n - 1, max=max(1, int(min_kept))), min=0)
    v = torch.sort(torch.where(valid, pd, torch.full_like(pd, float('inf'))).reshape(-1)).values.gather(0, k.reshape(1))[0]
    v = torch.where(n > 0, v, torch.zeros_like(v))
    thr = torch.clamp(v, min=float(thresh))
    if kept is None:
        kept = valid & (pd < thr)
    else:
        kept = kept.to(device=z.device).bool() & valid
    m = kept.sum()
    loss = torch.where(kept, l, torch.zeros_like(l)).sum() / torch.clamp(m, min=1).to(z.dtype)
    return loss, thr, kept, torch.where(valid, pd, torch.full_like(pd, float('nan')))


class _OhemHip(torch.autograd.Function):
    """forward: dcl_upsample_ce_fwd (lse, arg-max map) -> doh_target_prob -> doh_select -> doh_reduce; backward: dcl_upsample_ce_bwd
    on the hard-target map with grad_out / max(m, 1) formed on the device."""

    @staticmethod
    def forward(ctx, z, target, weight, ignore, H, W, align, thresh, min_kept, holder):
        from .. import _lib, _lib_ohem as oh
        L = _lib.lib()
        n, c, h, w = z.shape
        dev = z.device
        st = _lib.stream_ptr(dev)
        lse = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        pred = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
        partial = torch.empty((n * H, 2), dtype=torch.float32, device=dev)
        out2 = torch.empty(2, dtype=torch.float32, device=dev)                   # the plain CE of the call: discarded
        _lib.check(L.dcl_upsample_ce_fwd(_lib.ptr(z), n, c, h, w, H, W, 1 if align else 0, _lib.ptr(target), None, int(ignore),
                                         _lib.ptr(lse), _lib.ptr(pred), _lib.ptr(partial), _lib.ptr(out2), st), "dcl_upsample_ce_fwd")
        p = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        l = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        ws = torch.empty(oh.workspace_bytes(n, H), dtype=torch.uint8, device=dev)
        hard = torch.empty((n, H, W), dtype=torch.int64, device=dev)
        res = torch.empty(oh.RES_WORDS, dtype=torch.int32, device=dev)
        kept8 = torch.empty((n, H, W), dtype=torch.uint8, device=dev) if holder is not None and holder.get("want_kept") else None
        oh.target_prob(z, (H, W), align, target, weight, ignore, lse, p, l, ws, st)
        oh.select(p, min_kept, thresh, ws, st)
        oh.reduce(p, l, target, ignore, ws, hard, kept8, res, st)
        ctx.save_for_backward(z, hard, weight, lse, res)
        ctx.geom = (H, W, bool(align), int(ignore))
        if holder is not None:
            holder.update(pred=pred, p=p, l=l, lse=lse, hard=hard, kept=kept8, res=res)
        return res.view(torch.float32)[oh.RES_LOSS].clone()

    @staticmethod
    def backward(ctx, gout):
        from .. import _lib, _lib_ohem as oh
        L = _lib.lib()
        z, hard, weight, lse, res = ctx.saved_tensors
        H, W, align, ignore = ctx.geom
        n, c, h, w = z.shape
        gscale = (gout.reshape(1).to(torch.float32) / res.view(torch.float32)[oh.RES_DENOM:oh.RES_DENOM + 1]).contiguous()
        dz = torch.empty_like(z)
        _lib.check(L.dcl_upsample_ce_bwd(_lib.ptr(z), n, c, h, w, H, W, 1 if align else 0, _lib.ptr(hard), _lib.ptr(weight), ignore,
                                         _lib.ptr(lse), _lib.ptr(gscale), _lib.ptr(dz), _lib.stream_ptr(z.device)),
                   "dcl_upsample_ce_bwd")
        return dz, None, None, None, None, None, None, None, None, None


def hip_applies(z, target, size) -> bool:
    """Whether (z [N,C,h,w] resized to ``size``, target) takes the kernels: fp32 CUDA, the shape limits of include/dcl_ohem.h."""
    from ..debug import cfg
    if not (cfg.ohem_hip and torch.is_tensor(z) and z.is_cuda and target.is_cuda and z.dim() == 4 and z.dtype == torch.float32
            and not torch.is_autocast_enabled() and not target.is_floating_point()):
        return False
    from .. import _lib_ohem as oh
    n, c, h, w = z.shape
    return tuple(target.shape) == (n, int(size[0]), int(size[1])) and oh.supported(n, c, h, w, int(size[0]), int(size[1]))


def ohem_cross_entropy(z, target, weight, ignore, thresh, min_kept, size=None, align_corners=False, holder=None):
    """The loss of logits ``z`` (``size``: kept at low resolution, resized bilinearly to it) on the kernels where they apply, else
    ``ohem_reference``.  ``holder`` (a dict, optional) receives the maps of the kernel path (``pred``, ``p``, ``l``, ``lse``,
    ``hard``, ``res``; ``kept`` when it holds ``want_kept``) or ``path='torch'``."""
    out = (int(z.shape[2]), int(z.shape[3])) if size is None else (int(size[0]), int(size[1]))
    min_kept = max(1, int(min_kept))
    if hip_applies(z, target, out):
        if weight is not None:
            weight = weight.to(device=z.device, dtype=torch.float32).contiguous()
        if holder is not None:
            holder["path"] = "hip"
        return _OhemHip.apply(z.contiguous(), target.contiguous().long(), weight, int(ignore), out[0], out[1],
                              bool(align_corners) if size is not None else False, float(thresh), min_kept, holder)
    if holder is not None:
        holder["path"] = "torch"
    return ohem_reference(z, target, weight, ignore, thresh, min_kept, size=size, align_corners=align_corners)[0]


class OhemCrossEntropy(nn.Module):
    """``config``: the flat loss config as LossWrapper (or TwoScaleLoss, per head) passes it: ``dataset`` / ``experiment`` give the
    ignore id (LossWrapper's rule) and the class weights (Cityscapes: CITYSCAPES_CLASS_WEIGHTS, else none, as for CrossEntropyLoss
    there); ``ohem_thresh`` (0.7) and ``ohem_min_kept`` (100000) are the public defaults."""

    def __init__(self, config):
        super().__init__()
        self.dataset = config['dataset']
        self.experiment = config['experiment']
        names = DATASETS_INFO[self.dataset].CLASS_INFO[self.experiment][1]
        self.ignore_label = (len(names) - 1) if 255 in names else -1
        self.thresh = float(config.get('ohem_thresh', 0.7))
        self.min_kept = max(1, int(config.get('ohem_min_kept', 100000)))
        self.weight = torch.FloatTensor(CITYSCAPES_CLASS_WEIGHTS) if self.dataset == 'CITYSCAPES' else None
        self._weights = {}                          # device -> the weights there (one copy, made once)
        if self.weight is not None and 'device' in config:
            device = torch.device(config['device'])
            if device.type != 'cuda' or torch.cuda.is_available():
                self._weight_on(device)              # here, not in the first forward: a pageable copy blocks the host

    def _weight_on(self, device):
        if self.weight is None:
            return None
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if device not in self._weights:
            self._weights[device] = self.weight.to(device)
        return self._weights[device]

    def forward(self, prediction, target: torch.Tensor) -> torch.Tensor:
        w = self._weight_on(prediction.device)
        if hasattr(prediction, 'materialize'):      # models.ops_logits.UpsampledLogits: stays at low resolution
            return prediction.ohem_cross_entropy(target, w, self.ignore_label, self.thresh, self.min_kept)
        if prediction.dim() != 4 or tuple(prediction.shape[2:]) != tuple(target.shape[-2:]):
            raise ValueError(f"OhemCrossEntropy: logits {tuple(prediction.shape)} are not at the label size {tuple(target.shape)} "
                             "(up-sample them, or hand over an UpsampledLogits)")
        return ohem_cross_entropy(prediction, target, w, self.ignore_label, self.thresh, self.min_kept)
