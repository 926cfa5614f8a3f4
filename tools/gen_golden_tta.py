#!/usr/bin/env python3
"""G17: test-time-augmentation fixtures from the REFERENCE models/TTA_wrapper.py and models/TTA_wrapper_CTS.py, run on the CPU
(build container only).

tests/golden/G17_tta_<case>_ac<0|1>.npz: the reference's wrapper around a toy model (defined here and again in
tests/_tta_golden.py: Conv2d(3, K, 3, stride 4, padding 1) followed by a bilinear resize to the input size, with ``num_classes`` and
``align_corners``).  ``config_json`` (wrapper, K, align_corners, the scale list as passed and as the wrapper left it, flip, crop,
strides, base_size), the convolution's ``weight`` and ``bias``, the input ``x`` and the wrapper's output ``out``.

Two stand-ins live here, on top of tools/ref_shim.py: ``cv2.resize`` made from F.interpolate(align_corners=False) (cv2 is not
installed; INTER_LINEAR on a float image is half-pixel bilinear without antialiasing by its definition, which is read, not run),
and a ``Tensor.cuda`` whose result says its device type is 'cuda' (TTAWrapperCTS.inference asserts it).  The reference's
``base_size`` and ``num_classes`` are attributes, set on the instance after construction.  The reference is imported at run time;
none of its text is here."""
import builtins
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: E402

ref_shim.install()
ref_shim.quiet()
import cv2  # noqa: E402  (ref_shim's inert stand-in)


def _resize(img, dsize, interpolation=None):
    w, h = dsize
    t = torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1)[None]
    return F.interpolate(t, size=(h, w), mode='bilinear', align_corners=False)[0].permute(1, 2, 0).contiguous().numpy()


class _OnCuda(torch.Tensor):
    @property
    def device(self):
        return types.SimpleNamespace(type='cuda')


cv2.resize = _resize
cv2.INTER_LINEAR = 1
torch.Tensor.cuda = lambda self, *a, **k: self.as_subclass(_OnCuda)

_print = builtins.print
builtins.print = lambda *a, **k: None
from models.TTA_wrapper import TTAWrapper  # noqa: E402  (the reference's)
from models.TTA_wrapper_CTS import TTAWrapperCTS  # noqa: E402

OUT = os.path.join(os.path.dirname(__file__), "..", "tests", "golden")

CASES = {
    "a": dict(wrapper="plain", shape=[1, 3, 30, 44], K=5, scales=[0.5, 0.75, 1.5]),
    "b": dict(wrapper="cts", shape=[1, 3, 20, 40], K=5, scales=[0.5, 1.5], crop=[16, 24], strides=[11, 16], base=48, flip=True),
    "c": dict(wrapper="cts", shape=[1, 3, 20, 40], K=5, scales=[1.0], crop=[32, 24], strides=None, base=48, flip=False),
    "d": dict(wrapper="plain", shape=[1, 3, 8, 9], K=1, scales=[2.0]),
}


class Toy(nn.Module):
    def __init__(self, K, align_corners):
        super().__init__()
        self.num_classes = K
        self.align_corners = align_corners
        self.conv = nn.Conv2d(3, K, 3, stride=4, padding=1)

    def forward(self, x):
        return F.interpolate(self.conv(x), size=x.shape[-2:], mode='bilinear', align_corners=self.align_corners)


def fixtures():
    for seed, (name, c) in enumerate(sorted(CASES.items())):
        for ac in (False, True):
            torch.manual_seed(1700 + 2 * seed + int(ac))
            model = Toy(c["K"], ac).eval()
            x = torch.randn(c["shape"])
            scales = list(c["scales"])
            with torch.no_grad():
                if c["wrapper"] == "plain":
                    w = TTAWrapper(model, scales)
                else:
                    w = TTAWrapperCTS(model, scales, c["flip"], c["strides"], c["crop"])
                    w.base_size = c["base"]
                    w.num_classes = c["K"]
                out = w(x)
            out = torch.Tensor(out.as_subclass(torch.Tensor))
            assert list(out.shape) == [1, c["K"]] + c["shape"][2:] and bool(torch.isfinite(out).all())
            cfg = dict(c, align_corners=ac, scales_after=scales)
            path = os.path.join(OUT, f"G17_tta_{name}_ac{int(ac)}.npz")
            np.savez_compressed(path, config_json=np.array(json.dumps(cfg)), weight=model.conv.weight.detach().numpy(),
                                bias=model.conv.bias.detach().numpy(), x=x.numpy(), out=out.numpy())
            _print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes, max|out| {float(out.abs().max()):.4f}")


if __name__ == "__main__":
    torch.set_num_threads(4)
    fixtures()
