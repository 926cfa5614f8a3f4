"""Shared by tests/test_eval_host.py, tests/test_eval_hip.py and tests/test_eval_footprint.py: the shapes, the inputs, the float64
evaluation of the two resizes and the rule that leaves near-ties out."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import _pred_cases as pred_cases

#        (C, h, w, a1, Hp, Wp, rh, rw, H0, W0, a2); h = 0: dense input [1, C, Hp, Wp]
CASES = [(150, 8, 12, 0, 32, 48, 29, 43, 37, 55, 0),      # up-sampling, odd width, tail of 3
         (19, 8, 16, 1, 32, 64, 32, 64, 21, 45, 1),       # nothing cropped, stage 2 down-samples
         (150, 0, 0, 0, 32, 32, 23, 32, 50, 70, 0),       # dense input, rows cropped only
         (256, 4, 6, 1, 16, 24, 13, 21, 16, 22, 0),       # class limit, mixed flags
         (1, 3, 5, 0, 12, 20, 9, 17, 11, 19, 0),          # one class
         (19, 5, 7, 0, 20, 28, 17, 23, 64, 96, 1),        # W0 multiple of the run: word stores
         (19, 0, 0, 0, 16, 24, 16, 24, 16, 24, 0),        # both stages the identity
         (2, 8, 8, 0, 32, 32, 1, 1, 5, 7, 0),             # a crop of one pixel
         (19, 8, 8, 0, 32, 32, 31, 30, 1, 1, 1)]          # an output of one pixel
DENSE = CASES[2]
IDENTITY = CASES[6]
MARGIN = 2 * pred_cases.MARGIN      # x max|z|: two resizes stack twice the roundings of one
MAX_LEFT_OUT = 0.01


def case_id(c):
    return "x".join(map(str, c))


def logits(case):
    C, h, w, _, Hp, Wp = case[:6]
    return torch.randn(1, C, h or Hp, w or Wp, generator=torch.Generator().manual_seed(1000 * C + Hp))


def compose(z, case):
    """The torch composition in z's precision: resize to Hp x Wp (a lazy case), slice, resize to H0 x W0"""
    C, h, w, a1, Hp, Wp, rh, rw, H0, W0, a2 = case
    full = F.interpolate(z, size=(Hp, Wp), mode="bilinear", align_corners=bool(a1)) if h else z
    x = full[:, :, :rh, :rw]
    return F.interpolate(x, size=(H0, W0), mode="bilinear", align_corners=bool(a2)) if (rh, rw) != (H0, W0) else x


def decided(full, zmax):
    """(arg-max [1, H0, W0] int64, mask of the pixels whose float64 top-two margin is at least MARGIN * max|z|)"""
    if full.shape[1] == 1:
        return torch.zeros(full[:, 0].shape, dtype=torch.int64), torch.ones(full[:, 0].shape, dtype=torch.bool)
    top = full.topk(2, dim=1)
    return full.argmax(1), (top.values[:, 0] - top.values[:, 1]) >= MARGIN * zmax


@functools.lru_cache(maxsize=None)
def reference(case):
    """(z fp32, arg-max of the float64 evaluation in torch on the CPU, mask of the decided pixels), computed once per case"""
    z = logits(case)
    ids, ok = decided(compose(z.double(), case), float(z.abs().max()))
    assert float((~ok).float().mean()) <= MAX_LEFT_OUT, (case, int((~ok).sum()))
    return z, ids, ok


def wrap(z, case):
    """What evaluate_at_original takes for the case: an UpsampledLogits, or the dense tensor"""
    from mscs_amd.models.ops_logits import UpsampledLogits
    return UpsampledLogits(z, (case[4], case[5]), bool(case[3])) if case[1] else z


def target(case, hi=None, seed=6):
    """int64 [H0, W0] of class ids in [0, hi) (default: C + 1, the ignore id included)"""
    C, H0, W0 = case[0], case[8], case[9]
    return torch.randint(0, hi or C + 1, (H0, W0), generator=torch.Generator().manual_seed(seed + H0))


def lut(seed=5):
    return torch.randint(0, 256, (256,), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def bincount_cm(ids, t, C, cols):
    """int64 [C, cols] of (prediction, target) pairs with 0 <= target < cols, and the count of the others"""
    ids, t = ids.reshape(-1).long().cpu(), t.reshape(-1).long().cpu()
    good = (t >= 0) & (t < cols)
    return torch.bincount(ids[good] * cols + t[good], minlength=C * cols).view(C, cols), int((~good).sum())


def taps_np(in_size, mid, crop, out, a1, a2, dst):
    """dve_plan_taps restated with _pred_cases.src_index: ((j0, j1), (m0, m1), (i x 4), (l x 4)); equal sizes are (q, q), (1, 0)"""
    def stage(n_in, n_out, align, d):
        if n_in == n_out:
            return d, d, np.float32(1), np.float32(0)
        return pred_cases.src_index(n_in, n_out, align, d)
    j0, j1, m0, m1 = stage(crop, out, a2, dst)
    first, second = stage(in_size, mid, a1, j0), stage(in_size, mid, a1, j1)
    return (j0, j1), (m0, m1), first[:2] + second[:2], first[2:] + second[2:]


def manager_cfg(tmp, cuda=False, dataset="ADE20K", **extra):
    cfg = {"name": "eval", "mode": "training", "manager": "HRNet", "cuda": cuda, "parallel": False, "gpu_device": [0], "seed": 3,
           "log_every_n_steps": 1000, "log_path": str(tmp), "run_id": "run0", "save_checkpoints": False,
           "graph": {"model": "HRNet", "backbone": "hrnet18", "sync_bn": False, "pretrained": False, "align_corners": True},
           "data": {"dataset": dataset, "experiment": 1, "batch_size": 2, "num_workers": 0, "synthetic_raw": True,
                    "synthetic_raw_size": [45, 70], "synthetic_length": 2, "synthetic_valid_length": 2,
                    "transforms": ["RandomCropImgLbl", "torchvision_normalise"], "transform_values": {"crop_shape": [32, 64]},
                    "transforms_val": ["resize_val", "torchvision_normalise"],
                    "transform_values_val": {"min_side_length": 64, "fit_stride_val": 32}},
           "loss": {"name": "LossWrapper", "losses": {"CrossEntropyLoss": 1}},
           "train": {"learning_rate": 0.01, "lr_fct": "polynomial", "optim": "SGD", "lr_batchwise": True, "epochs": 1}}
    cfg.update(extra)
    return cfg
