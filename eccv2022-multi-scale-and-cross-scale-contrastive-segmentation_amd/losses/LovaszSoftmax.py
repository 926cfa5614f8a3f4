"""Lovasz-Softmax loss (Berman et al., CVPR 2018) with the reference's constructor and options
(losses/LovaszSoftmax.py:8-86): ``per_image``, ``classes_to_ignore`` (default: the dataset's ignore id),
``classes_to_consider`` in {'present', 'all', [ids]}.

On a GPU the loss runs on this project's kernels (csrc/dcl_lovasz.hip, C ABI include/dcl_lovasz.h): one key pass, a
segmented radix sort of all classes at once, an integer scan, and a one-pass backward -- no loop over classes, no host
synchronisation, bitwise reproducible.  The workspace is ``_lib_lovasz.workspace_bytes`` (about 16 bytes per logit; all
classes are sorted at once, there is no chunking).  That path is taken for CUDA tensors with C <= 256, N*C*H*W < 2^31,
floating-point logits (cast to fp32) and int64 / int32 / uint8 labels, unless ``DCL_LOVASZ_HIP=0`` (debug.cfg.lovasz_hip);
everything else, CPU tensors included, takes the PyTorch statement of the same loss below."""
import torch
import torch.nn as nn

from ..utils import DATASETS_INFO


def lovasz_grad(gt_sorted: torch.Tensor) -> torch.Tensor:
    """Gradient of the Lovasz extension of the Jaccard loss w.r.t. sorted errors (Alg. 1 of the paper)."""
    gts = gt_sorted.sum()
    inter = gts - gt_sorted.cumsum(0)
    union = gts + (1.0 - gt_sorted).cumsum(0)
    jac = 1.0 - inter / union
    if gt_sorted.numel() > 1:
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
    return jac


_LABEL_BYTES = {torch.int64: 8, torch.int32: 4, torch.uint8: 1}


class _LovaszHip(torch.autograd.Function):
    """forward: dlv_lovasz_fwd -> (loss, d loss / d softmax kept for the backward); backward: dlv_lovasz_bwd."""

    @staticmethod
    def forward(ctx, logits, target, per_image, ignore, present_only, consider):
        from .. import _lib_lovasz as lv
        n, c, h, w = logits.shape
        x = logits.detach()
        if x.dtype != torch.float32:
            x = x.float()
        x = x.contiguous()
        t = target.contiguous()
        nbytes = lv.workspace_bytes(n, c, h * w, per_image)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        coef = torch.empty_like(x)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        lv.check(lv.lib().dlv_lovasz_fwd(lv.ptr(x), lv.ptr(t), _LABEL_BYTES[t.dtype], n, c, h * w, int(per_image),
                                         int(ignore is not None), 0 if ignore is None else int(ignore), int(present_only),
                                         lv.ptr(consider), lv.ptr(ws), nbytes, lv.ptr(coef), lv.ptr(loss),
                                         lv.stream_ptr(x.device)), "dlv_lovasz_fwd")
        ctx.save_for_backward(x, coef)
        ctx.in_dtype = logits.dtype
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        from .. import _lib_lovasz as lv
        x, coef = ctx.saved_tensors
        n, c, h, w = x.shape
        up = grad_out.detach().to(torch.float32).contiguous()
        dx = torch.empty_like(x)
        lv.check(lv.lib().dlv_lovasz_bwd(lv.ptr(x), lv.ptr(coef), lv.ptr(up), n, c, h * w, lv.ptr(dx),
                                         lv.stream_ptr(x.device)), "dlv_lovasz_bwd")
        return (dx if ctx.in_dtype == torch.float32 else dx.to(ctx.in_dtype)), None, None, None, None, None


class LovaszSoftmax(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.eps = torch.as_tensor(1e-10)
        self.experiment = config['experiment']
        self.dataset = config['dataset']
        names = DATASETS_INFO[self.dataset].CLASS_INFO[self.experiment][1]
        default_ignore = len(names) - 1 if 255 in names else None
        self.per_image = config.get('per_image', False)
        self.classes_to_ignore = config.get('classes_to_ignore', default_ignore)
        self.classes_to_consider = config.get('classes_to_consider', 'present')
        self._consider = {}                        # (device, C) -> uint8 mask of a class list, built once

    def _flat(self, prob, lbl):
        c = prob.shape[1]
        prob = prob.permute(0, 2, 3, 1).reshape(-1, c)
        lbl = lbl.reshape(-1)
        if self.classes_to_ignore is None:
            return prob, lbl
        valid = lbl != self.classes_to_ignore
        return prob[valid], lbl[valid]

    def _loss_flat(self, prob, lbl):
        if prob.numel() == 0:
            return prob.sum() * 0.0                # only void pixels: zero loss, zero gradient
        c = prob.shape[1]
        classes = list(range(c)) if self.classes_to_consider in ('all', 'present') else self.classes_to_consider
        terms = []
        for k in classes:
            fg = (lbl == k).float()
            if self.classes_to_consider == 'present' and fg.sum() == 0:
                continue
            err = (fg - prob[:, k]).abs()
            err_sorted, perm = torch.sort(err, 0, descending=True)
            terms.append(torch.dot(err_sorted, lovasz_grad(fg[perm.detach()])))
        if not terms:
            return prob.sum() * 0.0                # no term: a zero TENSOR (the reference's int 0 breaks its own LossWrapper)
        return terms[0] if len(terms) == 1 else sum(terms[1:], terms[0]) / len(terms)

    def _hip_applies(self, prediction, target) -> bool:
        from ..debug import cfg
        if not (cfg.lovasz_hip and prediction.is_cuda and target.is_cuda and prediction.dim() == 4):
            return False
        n, c, h, w = prediction.shape
        return (prediction.is_floating_point() and prediction.dtype != torch.float64 and target.dtype in _LABEL_BYTES
                and tuple(target.shape) == (n, h, w) and 1 <= c <= 256 and n >= 1 and h * w >= 1 and n * c * h * w < 2 ** 31
                and (self.classes_to_ignore is None or isinstance(self.classes_to_ignore, int)))

    def _consider_mask(self, device, c):
        if self.classes_to_consider in ('all', 'present'):
            return None
        key = (device, c)
        if key not in self._consider:
            m = torch.zeros(c, dtype=torch.uint8)
            for k in self.classes_to_consider:
                m[k] = 1
            self._consider[key] = m.to(device)
        return self._consider[key]

    def forward(self, prediction: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if self._hip_applies(prediction, target):
            return _LovaszHip.apply(prediction, target, bool(self.per_image), self.classes_to_ignore,
                                    self.classes_to_consider == 'present',
                                    self._consider_mask(prediction.device, prediction.shape[1]))
        p = torch.softmax(prediction, dim=1)
        if self.per_image:
            per = [self._loss_flat(*self._flat(pi.unsqueeze(0), ti.unsqueeze(0))) for pi, ti in zip(p, target)]
            return per[0] if len(per) == 1 else sum(per[1:], per[0]) / len(per)
        return self._loss_flat(*self._flat(p, target))
