"""The training-time input augmentation of the reference (utils/config_parsers.py parse_transform_lists, utils/transforms.py,
utils/np_transforms.py FlipNP, torchvision's ColorJitter / Normalize) as ONE arithmetic, specified in DESIGN.md ("Input
augmentation") and include/dcl_aug.h: flip, resize, pad, crop, colour, normalise.

Three parts: ``AugmentPlanner`` draws a sample's ``Plan`` (every random quantity of the chain) on the host from a counter-based
stream, ``apply_plan_torch`` is the torch composition of the arithmetic (CPU tensors, unsupported plans, ``DCL_AUG_HIP=0``; the
oracle of the kernels), ``DeviceAugment`` turns lists of decoded uint8 tensors and plans into the batch, on libdcl_aug.so where
the plan is supported."""
import math
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np
import torch

from ..utils import DATASETS_INFO

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
PATIENCE = 10                                   # RandomCropImgLbl.patience
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ACCEPTED = ('flip', 'random_scale', 'RandomCropImgLbl', 'colorjitter', 'pseudo_colorjitter', 'resize_val', 'torchvision_normalise')
UNSUPPORTED = ('blur', 'pad', 'resize')


@dataclass
class Plan:
    """Every quantity that fixes the augmentation of one sample (``dau_plan`` of include/dcl_aug.h)."""
    H: int
    W: int
    rh: int
    rw: int
    Hc: int
    Wc: int
    pt: int
    pl: int
    h: int
    w: int
    flip: bool = False
    corners: List[Tuple[int, int]] = field(default_factory=lambda: [(0, 0)])
    perm: Tuple[int, ...] = ()
    b: float = 1.0
    c: float = 1.0
    s: float = 1.0
    delta: float = 0.0
    normalise: bool = True
    ignore: int = 255
    max_ratio: Optional[float] = None


def network_lut(dataset, experiment) -> torch.Tensor:
    """uint8 [256]: the reference's ``remap_mask(raw ids, CLASS_INFO[exp][0], to_network=True)`` as a table."""
    remap = DATASETS_INFO[dataset].CLASS_INFO[experiment][0]
    lut = np.full(256, 255, dtype=np.uint8)
    for key, vals in remap.items():
        for v in vals:
            if 0 <= v < 256:
                lut[v] = key
    lut[lut == 255] = len(remap) - 1
    return torch.from_numpy(lut)


def ignore_id(dataset, experiment) -> int:
    """The label of the padding (BaseTranform.ignore_class); -1 when the experiment has no ignore class."""
    names = DATASETS_INFO[dataset].CLASS_INFO[experiment][1]
    return len(names) - 1 if 255 in names else -1


class AugmentPlanner:
    """Parses the reference's transform list and draws plans.  The stream of sample ``index`` in ``epoch`` is
    ``numpy.random.default_rng((seed, epoch, index))``: it depends neither on the number of workers nor on the order of calls."""

    def __init__(self, transforms, transform_values, dataset, experiment, seed=0):
        tv = dict(transform_values or {})
        for t in transforms:
            if t in UNSUPPORTED:
                raise ValueError(f"transform {t} is not available on the device augmentation path (DESIGN.md, 'Input augmentation')")
            if t not in ACCEPTED:
                raise ValueError(f'transform {t} not recognized')
        self.transforms, self.values = list(transforms), tv
        self.dataset, self.experiment, self.seed = dataset, experiment, int(seed)
        self.ignore = ignore_id(dataset, experiment)
        if self.ignore < 0:
            raise ValueError(f'{dataset} experiment {experiment} has no ignore class to pad labels with')
        self.flip = 'flip' in transforms
        self.random_scale = 'random_scale' in transforms
        self.random_crop = 'RandomCropImgLbl' in transforms
        self.resize_val = 'resize_val' in transforms
        self.normalise = 'torchvision_normalise' in transforms
        self.crop_shape = tuple(tv['crop_shape']) if (self.random_scale or self.random_crop) else None
        self.max_ratio = tv.get('crop_class_max_ratio') or None
        self.scale_range = tuple(tv['scale_range']) if self.random_scale else (1.0, 1.0)
        self.aspect_range = tuple(tv.get('aspect_range', (0.9, 1.1)))
        self.p_random_scale = float(tv.get('p_random_scale', 1.0))
        # colour: (probability, (lo, hi) of b / c / s, hue half width); the later key of the list wins, as the chain would
        self.colour = None
        if 'colorjitter' in transforms:
            self.colour = (1.0, (2 / 3, 1.5), 0.05)
        if 'pseudo_colorjitter' in transforms:
            s = tv.get('colorjitter_strength', 2)
            self.colour = (float(tv.get('p_colorjitter', 0.7)), (1 - s * 0.25, 1 + s * 0.25), 0.02 * s)
        if self.resize_val:
            self.min_side, self.fit_stride = tv['min_side_length'], tv.get('fit_stride_val')

    def plan(self, H, W, epoch=0, index=0) -> Plan:
        rng = np.random.default_rng((self.seed, int(epoch), int(index)))
        # every quantity is drawn, in this order, whether or not it is used: a key of the list never shifts another's draw
        u_flip, u_scale = rng.random(), rng.random()
        scale, aspect = rng.uniform(*self.scale_range), rng.uniform(*self.aspect_range)
        u_pad = rng.random(2)
        u_corner = rng.random((PATIENCE, 2))
        u_colour = rng.random()
        lo, hi = self.colour[1] if self.colour else (1.0, 1.0)
        b, c, s = (float(v) for v in rng.uniform(lo, hi, 3))
        hw = self.colour[2] if self.colour else 0.0
        delta = float(rng.uniform(-hw, hw))
        perm = tuple(int(v) for v in rng.permutation(4))

        rh, rw = H, W
        resized = self.random_scale and u_scale < self.p_random_scale
        if self.resize_val:
            ratio = self.min_side / min(W, H)
            rw, rh = int(round(W * ratio)), int(round(H * ratio))
        elif resized:
            rw, rh = int(W * (math.sqrt(aspect) * scale)), int(H * (math.sqrt(1.0 / aspect) * scale))
        Hc, Wc, pt, pl = rh, rw, 0, 0
        if self.resize_val and self.fit_stride:
            Hc, Wc = -(-rh // self.fit_stride) * self.fit_stride, -(-rw // self.fit_stride) * self.fit_stride
        elif resized:                               # (the reference pads only inside the branch that resized)
            ch, cw = self.crop_shape
            Hc, Wc = max(rh, ch), max(rw, cw)
            pt, pl = min(int(u_pad[0] * (Hc - rh + 1)), Hc - rh), min(int(u_pad[1] * (Wc - rw + 1)), Wc - rw)
        if self.random_crop:
            h, w = self.crop_shape
            if h > Hc or w > Wc:
                raise ValueError(f'crop_shape {(h, w)} is larger than the image {(Hc, Wc)} (Required crop size is larger than input image size)')
            P = PATIENCE if self.max_ratio else 1
            corners = [(min(int(u_corner[p, 0] * (Hc - h + 1)), Hc - h), min(int(u_corner[p, 1] * (Wc - w + 1)), Wc - w))
                       for p in range(P)]
            if (Hc, Wc) == (h, w):
                corners = [(0, 0)]                  # torchvision's get_params returns the whole image without drawing
        else:
            h, w, corners = Hc, Wc, [(0, 0)]
        ops = perm if self.colour and u_colour < self.colour[0] else ()
        return Plan(H=H, W=W, rh=rh, rw=rw, Hc=Hc, Wc=Wc, pt=pt, pl=pl, h=h, w=w, flip=self.flip and u_flip < 0.5, corners=corners,
                    perm=ops, b=b, c=c, s=s, delta=delta, normalise=self.normalise, ignore=self.ignore,
                    max_ratio=self.max_ratio if self.random_crop else None)


# ---- the arithmetic, in torch ------------------------------------------------------------------------------------------------------
def resize_weights(S, D) -> np.ndarray:
    """float64 [D, S]: row o holds the normalised triangle-filter weights of output index o (csrc/dcl_aug_plan.h dau_tap_range /
    dau_tap_weight restated: the same double operations in the same order)."""
    scale = S / D
    sup = max(scale, 1.0)
    out = np.zeros((D, S), dtype=np.float64)
    for o in range(D):
        centre = (o + 0.5) * scale
        k0, k1 = max(int(centre - sup + 0.5), 0), min(int(centre + sup + 0.5), S)
        total = 0.0
        for k in range(k0, k1):
            total += max(1.0 - abs(k + 0.5 - centre) / sup, 0.0)
        for k in range(k0, k1):
            out[o, k] = max(1.0 - abs(k + 0.5 - centre) / sup, 0.0) / total
    return out


def nearest_index(S, D) -> np.ndarray:
    """int64 [D]: ((2 o + 1) S) // (2 D)."""
    o = np.arange(D, dtype=np.int64)
    return ((2 * o + 1) * S) // (2 * D)


def _weights_t(S, D, dtype, device):
    # through fp32 in either precision: the weights ARE fp32 numbers (include/dcl_aug.h), only the sums differ
    return torch.from_numpy(resize_weights(S, D).astype(np.float32)).to(device=device, dtype=dtype)


def resize_image(img, rh, rw, dtype=torch.float32):
    """[H, W, 3] (any real dtype) -> [rh, rw, 3] in ``dtype``: both axes without rounding in between."""
    H, W = img.shape[:2]
    x = img.to(dtype)
    if rh != H:
        x = torch.einsum('oh,hwc->owc', _weights_t(H, rh, dtype, img.device), x)
    if rw != W:
        x = torch.einsum('pw,owc->opc', _weights_t(W, rw, dtype, img.device), x)
    return x


def resize_label(lbl, rh, rw):
    H, W = lbl.shape
    iy = torch.from_numpy(nearest_index(H, rh)).to(lbl.device)
    ix = torch.from_numpy(nearest_index(W, rw)).to(lbl.device)
    return lbl[iy][:, ix]


def _luma(x):
    return (299 * x[..., 0] + 587 * x[..., 1] + 114 * x[..., 2]) / 1000


def brightness(x, b):
    return (x * b).clamp(0, 255)


def contrast(x, c, m=None):
    m = _luma(x).mean() if m is None else m
    return (m + c * (x - m)).clamp(0, 255)


def saturation(x, s):
    L = _luma(x)[..., None]
    return (L + s * (x - L)).clamp(0, 255)


def hue(x, delta):
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    maxc, minc = x.max(dim=-1).values, x.min(dim=-1).values
    eq = maxc == minc
    cr = maxc - minc
    one = torch.ones_like(maxc)
    s = cr / torch.where(eq, one, maxc)
    d = torch.where(eq, one, cr)
    rc, gc, bc = (maxc - r) / d, (maxc - g) / d, (maxc - b) / d
    h = torch.where(maxc == r, bc - gc, torch.where(maxc == g, 2 + rc - bc, 4 + gc - rc))
    h = h / 6 + 1
    h = h - torch.floor(h)
    h = h + delta
    h = h - torch.floor(h)
    h6 = h * 6
    fl = torch.floor(h6)
    f = h6 - fl
    i = fl.to(torch.int64) % 6
    p = (maxc * (1 - s)).clamp(0, 255)
    q = (maxc * (1 - f * s)).clamp(0, 255)
    t = (maxc * (1 - (1 - f) * s)).clamp(0, 255)
    table = torch.stack([torch.stack(v, dim=-1) for v in
                         ((maxc, t, p), (q, maxc, p), (p, maxc, t), (p, q, maxc), (t, p, maxc), (maxc, p, q))], dim=0)   # [6, ..., 3]
    return torch.gather(table, 0, i[None, ..., None].expand(1, *i.shape, 3))[0]


def candidate_verdict(window, ignore, max_ratio):
    """(acceptable, max_count, sum_count) of one candidate window of network labels."""
    cnt = torch.bincount(window.reshape(-1).to(torch.int64), minlength=256).cpu().numpy().astype(np.int64)
    cnt[ignore] = 0
    classes, mx, total = int((cnt > 0).sum()), int(cnt.max()), int(cnt.sum())
    ok = classes > 1 and float(mx) / float(total) < float(max_ratio)          # Python floats: the reference's float64 comparison
    return ok, mx, total


def choose_crop(lbl_canvas, plan: Plan) -> int:
    """Index of the chosen candidate: the first acceptable one, else the last."""
    P = len(plan.corners)
    if P == 1 or not plan.max_ratio:
        return P - 1
    for p, (i, j) in enumerate(plan.corners[:-1]):
        if candidate_verdict(lbl_canvas[i:i + plan.h, j:j + plan.w], plan.ignore, plan.max_ratio)[0]:
            return p
    return P - 1


def apply_plan_torch(img_u8, lbl_u8, plan: Plan, lut, dtype=torch.float32):
    """The composition: uint8 [H, W, 3] / uint8 [H, W] -> (``dtype`` [3, h, w], int64 [h, w], chosen candidate).  On the tensors'
    device; the crop choice reads the label counts back, which only this path may do."""
    assert tuple(img_u8.shape) == (plan.H, plan.W, 3) and tuple(lbl_u8.shape) == (plan.H, plan.W)
    img, lbl = (img_u8.flip(1), lbl_u8.flip(1)) if plan.flip else (img_u8, lbl_u8)
    x = resize_image(img, plan.rh, plan.rw, dtype)
    y = lut.to(lbl.device)[resize_label(lbl, plan.rh, plan.rw).to(torch.int64)]
    canvas = torch.zeros(plan.Hc, plan.Wc, 3, dtype=dtype, device=img.device)
    lcanvas = torch.full((plan.Hc, plan.Wc), plan.ignore, dtype=torch.uint8, device=img.device)
    canvas[plan.pt:plan.pt + plan.rh, plan.pl:plan.pl + plan.rw] = x
    lcanvas[plan.pt:plan.pt + plan.rh, plan.pl:plan.pl + plan.rw] = y
    chosen = choose_crop(lcanvas, plan)
    i, j = plan.corners[chosen]
    x, y = canvas[i:i + plan.h, j:j + plan.w], lcanvas[i:i + plan.h, j:j + plan.w]
    for op in plan.perm:
        if op == BRIGHTNESS:
            x = brightness(x, plan.b)
        elif op == CONTRAST:
            x = contrast(x, plan.c)
        elif op == SATURATION:
            x = saturation(x, plan.s)
        else:
            x = hue(x, plan.delta)
    x = x / 255
    if plan.normalise:
        x = (x - torch.tensor(MEAN, dtype=dtype, device=x.device)) / torch.tensor(STD, dtype=dtype, device=x.device)
    return x.permute(2, 0, 1).contiguous(), y.to(torch.int64).contiguous(), chosen


class DeviceAugment:
    """Lists of decoded tensors and plans -> the batch (float32 [B, 3, h, w], int64 [B, h, w]) on the tensors' device and the
    CURRENT stream.  Per sample: the kernels of libdcl_aug.so (three launches, no host synchronisation) when the tensors are on
    the GPU, the switch is on and ``dau_supported`` takes the plan; the composition otherwise."""

    def __init__(self, lut):
        self.lut = lut.to(torch.uint8).contiguous()
        self._luts = {}
        self.last_ws = None                         # [B, WS_INTS] int32 of the last batch that took the kernels (tests)
        self.last_paths = []                        # 'hip' / 'torch' per sample of the last batch

    def _lut_on(self, device):
        if device not in self._luts:
            self._luts[device] = self.lut.to(device)
        return self._luts[device]

    def _use_hip(self, img, lbl, plan):
        from ..debug import cfg as dbg
        if not (dbg.aug_hip and img.is_cuda and lbl.is_cuda):
            return None
        if not (img.dtype == torch.uint8 and lbl.dtype == torch.uint8 and img.is_contiguous() and lbl.is_contiguous()
                and tuple(img.shape) == (plan.H, plan.W, 3) and tuple(lbl.shape) == (plan.H, plan.W)):
            return None
        from .. import _lib_aug as la
        cp = la.c_plan(plan)
        return cp if la.supported(cp) else None

    def __call__(self, imgs, lbls, plans):
        assert len(imgs) == len(lbls) == len(plans) and len(imgs) > 0
        h, w = plans[0].h, plans[0].w
        assert all((p.h, p.w) == (h, w) for p in plans), 'every plan of a batch must have the same crop size'
        dev = imgs[0].device
        B = len(imgs)
        out = torch.empty(B, 3, h, w, dtype=torch.float32, device=dev)
        out_l = torch.empty(B, h, w, dtype=torch.int64, device=dev)
        lut = self._lut_on(dev)
        cps = [self._use_hip(i, l, p) for i, l, p in zip(imgs, lbls, plans)]
        self.last_paths = ['hip' if cp is not None else 'torch' for cp in cps]
        ws = None
        if any(cp is not None for cp in cps):
            from .. import _lib_aug as la
            ws = torch.zeros(B, la.WS_INTS, dtype=torch.int32, device=dev)
            st = la.stream_ptr(dev)
        for n, (img, lbl, plan, cp) in enumerate(zip(imgs, lbls, plans, cps)):
            if cp is None:
                x, y, _ = apply_plan_torch(img, lbl, plan, lut)
                out[n].copy_(x)
                out_l[n].copy_(y)
                continue
            if cp.P > 1:
                la.crop_select(lbl, lut, cp, ws[n], st)
            if CONTRAST in plan.perm:
                la.gray_mean(img, cp, ws[n], st)
            la.apply(img, lbl, lut, cp, ws[n], out[n], out_l[n], st)
        self.last_ws = ws
        return out, out_l

    def chosen(self, n, plan) -> int:
        """The candidate the kernels chose for sample n of the last batch (reads the verdicts back: tests and tools only)."""
        v = self.last_ws[n, :3 * len(plan.corners)].cpu().view(-1, 3)[:, 0].tolist()
        for p, ok in enumerate(v[:-1]):
            if ok:
                return p
        return len(v) - 1
