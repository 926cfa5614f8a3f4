"""Shared by tests/test_tta_host.py and tests/test_tta_hip.py: the G17 fixtures (tools/gen_golden_tta.py: the reference's
TTAWrapper / TTAWrapperCTS around a toy model, on the CPU), the toy model, and this package's wrapper built for a fixture."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from conftest import GOLDEN

CASES = [f"{c}_ac{a}" for c in "abcd" for a in (0, 1)]


class Toy(nn.Module):
    """Conv2d(3, K, 3, stride 4, padding 1) and a bilinear resize to the input size: logits at ceil(n / 4) like the models of the
    package.  ``lazy_eval_logits`` (only where ``lazy`` asks for the attribute) hands the low-resolution map out instead."""

    def __init__(self, K, align_corners, lazy=False):
        super().__init__()
        self.num_classes = K
        self.align_corners = align_corners
        self.conv = nn.Conv2d(3, K, 3, stride=4, padding=1)
        if lazy:
            self.lazy_eval_logits = False

    def forward(self, x):
        z = self.conv(x)
        if getattr(self, "lazy_eval_logits", False):
            from mscs_amd.models.ops_logits import UpsampledLogits
            return UpsampledLogits(z, x.shape[-2:], self.align_corners)
        return F.interpolate(z, size=x.shape[-2:], mode='bilinear', align_corners=self.align_corners)


def load(case):
    z = np.load(os.path.join(GOLDEN, f"G17_tta_{case}.npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["config"] = json.loads(str(d["config_json"]))
    return d


def toy(g, dev="cpu", dtype=torch.float32, lazy=False):
    c = g["config"]
    m = Toy(c["K"], c["align_corners"], lazy)
    with torch.no_grad():
        m.conv.weight.copy_(torch.from_numpy(g["weight"]))
        m.conv.bias.copy_(torch.from_numpy(g["bias"]))
    return m.to(dev).to(dtype).eval()


def wrapper(g, model, scales=None):
    """this package's wrapper with the fixture's arguments; ``scales`` (default: a copy of the fixture's list) is the list that is
    handed over -- and mutated"""
    from mscs_amd.models import TTAWrapper, TTAWrapperCTS
    c = g["config"]
    scales = list(c["scales"]) if scales is None else scales
    if c["wrapper"] == "plain":
        return TTAWrapper(model, scales)
    return TTAWrapperCTS(model, scales, c["flip"], c["strides"], c["crop"], base_size=c["base"], num_classes=c["K"])
