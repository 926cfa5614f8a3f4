"""The training-time input augmentation of the reference (utils/config_parsers.py parse_transform_lists, utils/transforms.py,
utils/np_transforms.py FlipNP, torchvision's ColorJitter / Normalize) as ONE arithmetic, specified in DESIGN.md ("Input
augmentation") and include/dcl_aug.h: flip, resize, pad, crop, colour, normalise.

Three parts: ``AugmentPlanner`` draws a sample's ``Plan`` (every random quantity of the chain) on the host from a counter-based
stream, ``apply_plan_torch`` is the torch composition of the arithmetic (CPU tensors, unsupported plans, ``DCL_AUG_HIP=0``; the
oracle of the kernels), ``DeviceAugment`` turns lists of decoded uint8 tensors and plans into the batch, on libdcl_aug.so where
the plan is supported.

``planner_for`` is what the manager calls: ``ChainPlanner`` adds the keys 'blur', 'pad' and 'resize' (BlurPIL, PadNP, Resize) and
experiments without an ignore class (CaDIS experiment 1).  What those keys do after the crop is the plan's ``chain``, which
``apply_plan_torch`` composes in torch and ``DeviceAugment`` runs on libdcl_blur.so (include/dcl_blur.h); a plan without a chain
takes the path above, untouched."""
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
    # what follows the crop on the image's planes, in the order of the config's list: ('pad', top, bottom), ('blur', R), ('colour',).
    # Empty: perm runs right after the crop (dau_apply).  Otherwise perm runs where the ('colour',) item stands, and only there.
    chain: tuple = ()

    @property
    def out_h(self) -> int:
        """Rows of the sample's slice of the batch: the crop's and those the chain's pads add."""
        return self.h + sum(it[1] + it[2] for it in self.chain if it[0] == 'pad')

    @property
    def out_w(self) -> int:
        return self.w


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
                raise ValueError(f"transform {t} is not available to AugmentPlanner: planner_for() returns the planner that takes it "
                                 "(DESIGN.md, 'Input augmentation')")
            if t not in ACCEPTED:
                raise ValueError(f'transform {t} not recognized')
        ignore = ignore_id(dataset, experiment)
        if ignore < 0:
            raise ValueError(f'{dataset} experiment {experiment} has no ignore class to pad labels with')
        self._setup(transforms, tv, dataset, experiment, seed, ignore)

    def _setup(self, transforms, tv, dataset, experiment, seed, ignore):
        """The keys of ACCEPTED (shared with ChainPlanner, which has taken its own keys out of the list)."""
        self.transforms, self.values = list(transforms), tv
        self.dataset, self.experiment, self.seed = dataset, experiment, int(seed)
        self.ignore = ignore
        self.resize = None                          # ChainPlanner's 'resize' key: (target (h, w) or None, min side or None)
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
        return self._draw(np.random.default_rng((self.seed, int(epoch), int(index))), H, W)

    def _draw(self, rng, H, W) -> Plan:
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
        if self.resize is not None and self.resize[0] is not None:
            rh, rw = self.resize[0]
        elif self.resize_val or self.resize is not None:
            ratio = self.min_side / min(W, H)
            rw, rh = int(round(W * ratio)), int(round(H * ratio))
        elif resized:
            rw, rh = int(W * (math.sqrt(aspect) * scale)), int(H * (math.sqrt(1.0 / aspect) * scale))
        Hc, Wc, pt, pl = rh, rw, 0, 0
        if (self.resize_val or self.resize is not None) and self.fit_stride:
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


BLUR_P, BLUR_KERNEL_LIMITS = 0.05, (3, 7)        # parse_transform_lists: BlurPIL(probability=.05, kernel_limits=(3, 7))
PAD_ROWS = (2, 2)                               # ... PadNP(ver=(2, 2), hor=(0, 0), padding_mode='reflect'): 540 rows -> 544
NO_IGNORE = 255                                 # Plan.ignore of an experiment without an ignore class: no lookup table produces it


class ChainPlanner(AugmentPlanner):
    """AugmentPlanner and the reference's remaining ``data.transforms`` keys: 'blur', 'pad' and 'resize'.  Its draws come after every
    draw of AugmentPlanner on the same stream, so a list within ACCEPTED gives AugmentPlanner's plans; what the new keys add is the
    plan's ``chain``.  An experiment without an ignore class is taken as long as nothing pads labels with it."""

    def __init__(self, transforms, transform_values, dataset, experiment, seed=0):
        tv = dict(transform_values or {})
        for t in transforms:
            if t not in ACCEPTED and t not in UNSUPPORTED:
                raise ValueError(f'transform {t} not recognized')
        ignore = ignore_id(dataset, experiment)
        self._setup([t for t in transforms if t in ACCEPTED], tv, dataset, experiment, seed, ignore if ignore >= 0 else NO_IGNORE)
        self.blur = 'blur' in transforms
        self.blur_p = float(tv.get('blur_p', BLUR_P))
        self.blur_limits = tuple(int(v) for v in tv.get('blur_kernel_limits', BLUR_KERNEL_LIMITS))
        if self.blur and not self.blur_limits[0] < self.blur_limits[1]:
            raise ValueError(f'blur: blur_kernel_limits {self.blur_limits} is an empty range')
        if 'pad' in transforms and dataset != 'CADIS':
            raise ValueError(f"transform pad is for CADIS only (PadNP(ver=(2, 2)) takes its 540 rows to 544), not for {dataset}")
        self.pad = PAD_ROWS if 'pad' in transforms and 'crop' not in transforms else None
        if 'resize' in transforms:
            target, self.fit_stride = tv.get('target_size'), tv.get('fit_stride')
            if target is None and tv.get('min_side_length') is None:
                raise ValueError("transform resize needs transform_values.target_size [h, w] or transform_values.min_side_length")
            self.resize = (tuple(int(v) for v in target) if target is not None else None, tv.get('min_side_length'))
            self.min_side = tv.get('min_side_length')
        if ignore < 0:
            for key, pads in (('random_scale', self.random_scale), ('resize', self.resize is not None and bool(self.fit_stride)),
                              ('resize_val', self.resize_val)):
                if pads:
                    raise ValueError(f'transform {key} pads labels with the ignore class, and {dataset} experiment {experiment} has none')
        # the image's steps after the crop, in the order of the list (the later colour key wins, as in AugmentPlanner)
        colour_key = 'pseudo_colorjitter' if 'pseudo_colorjitter' in transforms else 'colorjitter'
        self.order = [t for t in transforms if t in ('pad', 'blur', colour_key)]

    def plan(self, H, W, epoch=0, index=0) -> Plan:
        rng = np.random.default_rng((self.seed, int(epoch), int(index)))
        p = self._draw(rng, H, W)
        u_blur = rng.random()                       # drawn whether or not the list holds 'blur', after every draw of _draw
        R = int(rng.integers(*self.blur_limits))
        chain = []
        for t in self.order:
            if t == 'pad' and self.pad is not None:
                chain.append(('pad',) + self.pad)
            elif t == 'blur' and self.blur and u_blur < self.blur_p:
                chain.append(('blur', R))
            elif t not in ('pad', 'blur') and p.perm:
                chain.append(('colour',))
        if chain != [('colour',)]:                  # colour alone: AugmentPlanner's plan, three launches
            p.chain = tuple(chain)
        return p


def planner_for(transforms, transform_values, dataset, experiment, seed=0):
    """The planner of a transform list: AugmentPlanner for what it takes (the same plans as ever), else ChainPlanner."""
    if all(t in ACCEPTED for t in transforms) and ignore_id(dataset, experiment) >= 0:
        return AugmentPlanner(transforms, transform_values, dataset, experiment, seed)
    return ChainPlanner(transforms, transform_values, dataset, experiment, seed)


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


def box_of(radius):
    """(l, ww, fw) of PIL's GaussianBlur(radius): the extended box of its three passes an axis (csrc/dcl_blur_plan.h dbl_box_of
    restated: the same double operations in the same order, the two weights rounded to fp32 last)."""
    s2 = float(radius) * float(radius) / 3.0
    L = math.sqrt(12.0 * s2 + 1.0)
    l = math.floor((L - 1.0) / 2.0)
    a = (2.0 * l + 1.0) * (l * (l + 1.0) - 3.0 * s2) / (6.0 * (s2 - (l + 1.0) * (l + 1.0)))
    ww = 1.0 / (2.0 * (l + a) + 1.0)
    return int(l), float(np.float32(ww)), float(np.float32((1.0 - (2.0 * l + 1.0) * ww) / 2.0))


def box_pass(x, dim, l, ww, fw):
    """One extended-box pass along ``dim``: ww (sum of the 2 l + 1 inner taps, from -l upwards) + fw (the two outer taps), every
    index clamped to the axis."""
    n = x.shape[dim]
    idx = torch.arange(n, device=x.device)
    tap = lambda d: x.index_select(dim, (idx + d).clamp(0, n - 1))
    acc = torch.zeros_like(x)
    for d in range(-l, l + 1):
        acc = acc + tap(d)
    return ww * acc + fw * (tap(-l - 1) + tap(l + 1))


def gaussian_blur(x, radius):
    """[h, w, ...] -> the same: three passes along the rows (x), then three along the columns (y)."""
    l, ww, fw = box_of(radius)
    for dim in (1, 1, 1, 0, 0, 0):
        x = box_pass(x, dim, l, ww, fw)
    return x


def reflect_rows(x, top, bottom):
    """numpy.pad(mode='reflect') along the rows of [h, ...]."""
    h = x.shape[0]
    assert 0 <= top <= h - 1 and 0 <= bottom <= h - 1, f'reflect padding {(top, bottom)} needs more than {h} rows'
    r = torch.arange(-top, h + bottom, device=x.device).abs()
    r = torch.where(r > h - 1, 2 * (h - 1) - r, r)
    return x.index_select(0, r)


def colour_chain(x, plan):
    """plan.perm on [h, w, 3] values in [0, 255]."""
    for op in plan.perm:
        if op == BRIGHTNESS:
            x = brightness(x, plan.b)
        elif op == CONTRAST:
            x = contrast(x, plan.c)
        elif op == SATURATION:
            x = saturation(x, plan.s)
        else:
            x = hue(x, plan.delta)
    return x


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
    if not plan.chain:
        x = colour_chain(x, plan)
    else:                                           # the kernels' order: dau_apply leaves x / 255, dbl_from_unit takes it back
        x = x / 255 * 255
        for item in plan.chain:
            if item[0] == 'pad':
                x, y = reflect_rows(x, item[1], item[2]), reflect_rows(y, item[1], item[2])
            elif item[0] == 'blur':
                x = gaussian_blur(x, item[1])
            elif item[0] == 'colour':
                x = colour_chain(x, plan)
            else:
                raise ValueError(f'chain item {item} not recognized')
    x = x / 255
    if plan.normalise:
        x = (x - torch.tensor(MEAN, dtype=dtype, device=x.device)) / torch.tensor(STD, dtype=dtype, device=x.device)
    return x.permute(2, 0, 1).contiguous(), y.to(torch.int64).contiguous(), chosen


class DeviceAugment:
    """Lists of decoded tensors and plans -> the batch (float32 [B, 3, h, w], int64 [B, h, w]) on the tensors' device and the
    CURRENT stream.  Per sample: the kernels of libdcl_aug.so (three launches, no host synchronisation) when the tensors are on
    the GPU, the switch is on and ``dau_supported`` takes the plan; the composition otherwise.  A plan with a ``chain`` goes on
    from there on libdcl_blur.so (``_chain``) when its switch is on too and ``dbl_supported`` takes every blur of the chain."""

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
        if plan.chain:
            from dataclasses import replace
            from .. import _lib_blur as lb
            h = plan.h
            for item in plan.chain:
                if item[0] == 'pad':
                    if not (0 <= item[1] <= h - 1 and 0 <= item[2] <= h - 1):
                        return None
                    h += item[1] + item[2]
                elif item[0] == 'blur':
                    if not lb.supported(3, h, plan.w, item[1]):
                        return None
                elif item[0] != 'colour':
                    return None
            if not dbg.blur_hip or 3 * h * plan.w >= 2 ** 31:
                return None
            plan = replace(plan, perm=(), normalise=False)      # dau_apply's part: up to the crop, x / 255
        cp = la.c_plan(plan)
        return cp if la.supported(cp) else None

    def _chain(self, planes, lbl, plan, ws, out, out_l, st):
        """What follows dau_apply for a plan with a chain: ``planes`` (float32 [3, h, w] of x / 255) and ``lbl`` (int64 [h, w]) ->
        the sample's slices ``out`` / ``out_l``, every launch on the current stream."""
        from .. import _lib_blur as lb
        lb.from_unit(planes, planes, st)
        pads = sum(item[0] == 'pad' for item in plan.chain)
        for item in plan.chain:
            if item[0] == 'pad':
                pads -= 1
                ho = planes.shape[1] + item[1] + item[2]
                padded = torch.empty(3, ho, planes.shape[2], dtype=torch.float32, device=planes.device)
                lbl_p = out_l if pads == 0 else torch.empty(ho, planes.shape[2], dtype=torch.int64, device=planes.device)
                lb.pad_rows(planes, padded, lbl, lbl_p, item[1], item[2], st)
                planes, lbl = padded, lbl_p
            elif item[0] == 'blur':
                dst, scratch = torch.empty_like(planes), torch.empty_like(planes)
                lb.blur(planes, dst, scratch, item[1], st)
                planes = dst
            else:
                cp = lb.colour_plan(plan, planes.shape[1], planes.shape[2])
                if CONTRAST in plan.perm:
                    lb.gray_mean(planes, cp, ws, st)
                lb.colour(planes, cp, ws, st)
        lb.normalise(planes, out, plan.normalise, st)

    def __call__(self, imgs, lbls, plans):
        assert len(imgs) == len(lbls) == len(plans) and len(imgs) > 0
        h, w = plans[0].out_h, plans[0].out_w
        assert all((p.out_h, p.out_w) == (h, w) for p in plans), 'every plan of a batch must have the same crop size'
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
            if CONTRAST in plan.perm and not plan.chain:
                la.gray_mean(img, cp, ws[n], st)
            if plan.chain:
                planes = torch.empty(3, plan.h, plan.w, dtype=torch.float32, device=dev)
                padded = any(item[0] == 'pad' for item in plan.chain)
                y = torch.empty(plan.h, plan.w, dtype=torch.int64, device=dev) if padded else out_l[n]
                la.apply(img, lbl, lut, cp, ws[n], planes, y, st)
                self._chain(planes, y, plan, ws[n], out[n], out_l[n], st)
                continue
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
