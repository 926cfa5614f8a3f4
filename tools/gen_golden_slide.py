#!/usr/bin/env python3
"""G19: sliding-window test-time-augmentation fixtures from the REFERENCE models/TTA_wrapper_PC.py and models/TTAWrapperSlide.py, run
on the CPU (build container only).

tests/golden/G19_slide_<case>_ac<0|1>.npz: the reference's wrapper around the toy model of tools/gen_golden_tta.py (Conv2d(3, K, 3,
stride 4, padding 1) followed by a bilinear resize to the input size; defined again in tests/_tta_golden.py).  ``config_json``
(protocol, K, align_corners, the scale list as passed and as the wrapper left it, crop, base_size / img_scale, strides, flip), the
convolution's ``weight`` and ``bias``, the input ``x`` and the wrapper's output ``out``.

Stand-ins on top of tools/ref_shim.py (cv2 is not installed; what the functions do is read from their documentation, not run):
``cv2.resize`` made from F.interpolate(align_corners=False) (INTER_LINEAR on a float image is half-pixel bilinear without
antialiasing), ``cv2.copyMakeBorder`` with ``BORDER_CONSTANT`` as a constant border in the image's dtype, and a ``Tensor.cuda``
whose result says its device type is 'cuda' (both ``inference`` methods assert it).  The reference's ``crop_size``, ``base_size``,
``num_classes`` and ``img_scale`` are literals of its constructors: they are set on the instance after construction, and the view
list that TTAWrapperSlide derives from ``img_scale`` in its constructor is derived again from the fixture's value.  The reference is
imported at run time; none of its text is here."""
import builtins
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: E402

ref_shim.install()
ref_shim.quiet()
import cv2  # noqa: E402  (ref_shim's inert stand-in)

from gen_golden_tta import Toy, _OnCuda, _print, _resize  # noqa: E402  (it silences print; _print is the real one)


def _copy_make_border(img, top, bottom, left, right, border_type, value=0):
    assert border_type == cv2.BORDER_CONSTANT and top == 0 and left == 0
    h, w = img.shape[:2]
    out = np.empty((h + bottom, w + right) + img.shape[2:], dtype=img.dtype)
    out[...] = np.asarray(value, dtype=img.dtype)
    out[:h, :w] = img
    return out


cv2.resize = _resize
cv2.INTER_LINEAR = 1
cv2.BORDER_CONSTANT = 0
cv2.copyMakeBorder = _copy_make_border
torch.Tensor.cuda = lambda self, *a, **k: self.as_subclass(_OnCuda)

builtins.print = lambda *a, **k: None
from models.TTA_wrapper_PC import TTAWrapperPC  # noqa: E402  (the reference's)
from models.TTAWrapperSlide import TTAWrapperSlide  # noqa: E402

OUT = os.path.join(os.path.dirname(__file__), "..", "tests", "golden")

CASES = {
    "pa": dict(protocol="pc", shape=[1, 3, 22, 30], K=5, scales=[0.25, 0.5, 1.5], crop=[16, 24], base=40),
    "pb": dict(protocol="pc", shape=[1, 3, 30, 22], K=5, scales=[0.25, 0.5, 1.5], crop=[16, 24], base=40),
    "sa": dict(protocol="slide", shape=[1, 3, 20, 40], K=5, scales=[0.5, 1.5], crop=[16, 24], strides=[5, 11], flip=True,
               img_scale=[44, 28]),
    "sb": dict(protocol="slide", shape=[1, 3, 20, 40], K=5, scales=[0.5, 1.5], crop=[16, 24], strides=None, flip=False,
               img_scale=[44, 28]),
}


def fixtures():
    for seed, (name, c) in enumerate(sorted(CASES.items())):
        for ac in (False, True):
            torch.manual_seed(1900 + 2 * seed + int(ac))
            model = Toy(c["K"], ac).eval()
            x = torch.randn(c["shape"])
            scales = list(c["scales"])
            with torch.no_grad():
                if c["protocol"] == "pc":
                    w = TTAWrapperPC(model, scales)
                    w.crop_size = list(c["crop"])
                    w.base_size = c["base"]
                else:
                    w = TTAWrapperSlide(model, scales, c["flip"], c["strides"], list(c["crop"]))
                    flips = [True, False] if c["flip"] else [False]
                    w.image_scales = [((int(c["img_scale"][0] * s), int(c["img_scale"][1] * s)), s) for s in w.scales for _ in flips]
                    w.image_flips = [f for _ in w.scales for f in flips]
                w.num_classes = c["K"]
                out = w(x)
            out = torch.Tensor(out.as_subclass(torch.Tensor))
            assert list(out.shape) == [1, c["K"]] + c["shape"][2:] and bool(torch.isfinite(out).all())
            cfg = dict(c, align_corners=ac, scales_after=scales)
            path = os.path.join(OUT, f"G19_slide_{name}_ac{int(ac)}.npz")
            np.savez_compressed(path, config_json=np.array(json.dumps(cfg)), weight=model.conv.weight.detach().numpy(),
                                bias=model.conv.bias.detach().numpy(), x=x.numpy(), out=out.numpy())
            _print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes, max|out| {float(out.abs().max()):.4f}")


if __name__ == "__main__":
    torch.set_num_threads(4)
    fixtures()
