"""Footprint of the input-augmentation entries at the C ABI (include/dcl_aug.h): dau_crop_select / dau_gray_mean / dau_apply on
guarded buffers (tests/_footprint.py): every band intact, both outputs fully written, finite and independent of what lies outside
the inputs, and the values those of the Python entry point on torch-allocated buffers."""
import numpy as np
import pytest
import torch

from _footprint import run_both

import _aug_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def leave_no_state():
    """The modules that run after this one find the random streams and the device memory pool as this one found them."""
    state = cases.save_state()
    yield
    cases.restore_state(state)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_aug
    _lib_aug.lib()
    return torch.device("cuda:0")


def _plans():
    from mscs_amd.datasets.augment import Plan
    col = dict(perm=(2, 0, 1, 3), b=1.2, c=0.8, s=1.3, delta=-0.04, ignore=cases.IGNORE)
    return [
        ("1x1 -> 1x1", Plan(H=1, W=1, rh=1, rw=1, Hc=1, Wc=1, pt=0, pl=0, h=1, w=1, corners=[(0, 0)], **col)),
        ("2x3 -> 5x7", Plan(H=2, W=3, rh=5, rw=7, Hc=5, Wc=7, pt=0, pl=0, h=5, w=7, flip=True, corners=[(0, 0)], **col)),
        # 37 x 53 shrunk by 8 (the most taps) to 5 x 7 inside a 16 x 24 canvas: maximal padding, ten candidates, the image in the
        # far corner so that the first candidates see padding only
        ("37x53 -> 16x24 padded", Plan(H=37, W=53, rh=5, rw=7, Hc=16, Wc=24, pt=11, pl=17, h=16, w=24, flip=True,
                                       corners=[(0, 0)], **col)),
        ("37x53 -> 8x12 of a padded 16x24", Plan(H=37, W=53, rh=5, rw=7, Hc=16, Wc=24, pt=11, pl=17, h=8, w=12, flip=False,
                                                 corners=[(0, 0), (3, 5), (8, 12), (8, 0), (0, 12), (4, 4), (8, 11), (7, 12), (1, 1),
                                                          (8, 12)], max_ratio=0.75, **col)),
    ]


@pytest.mark.parametrize("case", _plans(), ids=lambda c: c[0])
def test_aug_entries_footprint(dev, case):
    from mscs_amd import _lib_aug as la
    from mscs_amd.datasets import augment as A
    name, plan = case
    cp = la.c_plan(plan)
    assert la.supported(cp)
    rng = np.random.default_rng(plan.H * 100 + plan.W)
    img = torch.from_numpy(rng.integers(0, 256, (plan.H, plan.W, 3), dtype=np.uint8)).to(dev)
    lbl = torch.from_numpy(rng.integers(0, 20, (plan.H, plan.W), dtype=np.uint8)).to(dev)
    lut = cases.identity_lut().to(dev)
    st = la.stream_ptr(dev)

    def body(ar):
        gi, gl, gt = ar.inp(img, "img"), ar.inp(lbl, "lbl"), ar.inp(lut, "lut")
        ws = ar.zeros(la.WS_INTS, torch.int32, "ws")
        out = ar.out((3, plan.h, plan.w), torch.float32, "out_img")
        out_l = ar.out((plan.h, plan.w), torch.int64, "out_lbl")
        if len(plan.corners) > 1:
            la.crop_select(gl, gt, cp, ws, st)
        la.gray_mean(gi, cp, ws, st)
        la.apply(gi, gl, gt, cp, ws, out, out_l, st)
        return {"img": out, "lbl": out_l, "verdicts": ws[:3 * len(plan.corners)] if len(plan.corners) > 1 else ws[la.WS_MEAN:la.WS_MEAN + 1]}
    got = run_both(dev, body, ("aug", name))

    # the values are those of the Python entry point on torch-allocated buffers, and the composition's
    aug = A.DeviceAugment(cases.identity_lut())
    x, y = aug([img], [lbl], [plan])
    assert aug.last_paths == ["hip"] and torch.equal(got["img"], x[0]) and torch.equal(got["lbl"], y[0])
    ex, ey, chosen = A.apply_plan_torch(img.cpu(), lbl.cpu(), plan, cases.identity_lut(), torch.float64)
    assert torch.equal(got["lbl"].cpu(), ey)
    if len(plan.corners) > 1:
        assert aug.chosen(0, plan) == chosen
    # and close to the float64 composition.  A worst-case fp32 round-off bound for ANY supported plan (this is not the accuracy test):
    # at most 17 x 17 = 289 filter terms and some 20 operations of the colour chain, each rounding a value of at most 255 by 2^-24
    # relative, then / 255 / 0.224: (289 + 20) * 2^-24 / 0.224 = 8.2e-5.  A wrong tap or operation moves a pixel by 1 / 255 / 0.229
    # = 1.7e-2 or more.
    assert float((got["img"].cpu().double() - ex).abs().max()) <= 1e-4
