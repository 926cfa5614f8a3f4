"""Shared by tests/test_slide_host.py, tests/test_slide_hip.py and tests/test_slide_footprint.py: the G19 fixtures
(tools/gen_golden_slide.py: the reference's TTAWrapperPC / TTAWrapperSlide around the toy model of tests/_tta_golden.py, on the
CPU), this package's wrapper built for a fixture, the window grids of the fixture geometries, and the error bound of
tests/test_tta_hip.py."""
import json
import os

import numpy as np
import torch

from conftest import GOLDEN

from _tta_golden import toy  # noqa: F401  (the same toy model: Conv2d(3, K, 3, stride 4, padding 1) and a resize)

CASES = [f"{c}_ac{a}" for c in ("pa", "pb", "sa", "sb") for a in (0, 1)]
EPS = float(np.finfo(np.float32).eps)
PAD = [-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225]

# Window grids of the fixture geometries, computed by hand from the reference's loops:
#   name: (resized image (nh, nw), window (wh, ww), row starts, column starts)
# PASCAL-Context (crop (16, 24), strides (10, 16), no shift-back, partial windows padded); the canvas is the un-padded image
# ADE20K slide (img_scale (44, 28), crop (16, 24), strides (5, 11), last window shifted back, a short axis gives a short window)
GRIDS = {
    "pa_1.0": ((29, 40), (16, 24), [0, 10, 20], [0, 16]),                       # 3 x 2, partial last row
    "pa_1.5": ((44, 60), (16, 24), [0, 10, 20, 30], [0, 16, 32, 48]),           # 4 x 4, partial last row and column
    "pb_0.5": ((20, 15), (16, 24), [0, 10], [0]),                               # padded on one axis only: 2 x 1
    "pb_1.5": ((60, 44), (16, 24), [0, 10, 20, 30, 40, 50], [0, 16, 32]),       # 6 x 3
    "sa_0.5": ((22, 14), (16, 14), [0, 5, 6], [0]),                             # three short windows, cover up to 3
    "sa_1.0": ((44, 28), (16, 24), [0, 5, 10, 15, 20, 25, 28], [0, 4]),         # 7 x 2
    "sa_1.5": ((66, 42), (16, 24), [0, 5, 10, 15, 20, 25, 30, 35, 40, 45, 50], [0, 11, 18]),   # 11 x 3, cover up to 4 x 3
    "odd": ((23, 31), (7, 10), [0, 5, 11, 16], [0, 9, 15, 21]),                 # nw % 4 != 0, odd column starts, ww % 4 != 0
}


def load(case):
    z = np.load(os.path.join(GOLDEN, f"G19_slide_{case}.npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["config"] = json.loads(str(d["config_json"]))
    return d


def wrapper(g, model, scales=None, window_batch=None):
    """this package's wrapper with the fixture's arguments; ``scales`` (default: a copy of the fixture's list) is the list that is
    handed over -- and mutated"""
    from mscs_amd.models import TTAWrapperPC, TTAWrapperSlide
    c = g["config"]
    scales = list(c["scales"]) if scales is None else scales
    if c["protocol"] == "pc":
        w = TTAWrapperPC(model, scales, num_classes=c["K"], crop_size=tuple(c["crop"]), base_size=c["base"])
    else:
        w = TTAWrapperSlide(model, scales, c["flip"], c["strides"], c["crop"], num_classes=c["K"], img_scale=tuple(c["img_scale"]))
    if window_batch is not None:
        w.tta_window_batch = window_batch
    return w


def views(g):
    """model views of a fixture: PASCAL-Context one per scale, the ADE20K protocol two per scale with ``flip``"""
    c = g["config"]
    return len(c["scales_after"]) * (2 if c["protocol"] == "slide" and c["flip"] else 1)


def logits(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=gen, dtype=torch.float64) * 3).clamp_(-8, 8).float()


def bound(got, eager, ref, relative=False, what="", record=None):
    """tests/test_tta_hip.py::_bound: got / eager are fp32 results of the kernel and of the torch composition, ref is float64;
    e_kernel <= max(4 * e_eager, 16 * eps32 * max|ref|), or the same on errors divided by |ref| (floor 16 * eps32)"""
    got, eager, ref = got.detach().double().cpu(), eager.detach().double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    scale = ref.abs() if relative else torch.ones(())
    e_kernel = float(((got - ref).abs() / scale).max())
    e_eager = float(((eager - ref).abs() / scale).max())
    floor = 16 * EPS * (1.0 if relative else float(ref.abs().max()))
    print(f"{what}: e_kernel {e_kernel:.3e} e_eager {e_eager:.3e} floor {floor:.3e}")
    if record is not None:
        record[what] = {"e_kernel": e_kernel, "e_eager": e_eager, "floor": floor, "relative": bool(relative)}
    assert e_kernel <= max(4 * e_eager, floor), (what, e_kernel, e_eager, floor)
