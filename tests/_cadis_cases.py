"""Shared by tests/test_cadis_host.py and tests/test_blur_hip.py: the eight plans with a chain of the kernel comparison, structured
uint8 images for the blur, and the rows of the CaDIS frame-table excerpt."""
import numpy as np
import torch

from mscs_amd.datasets.augment import BRIGHTNESS as B, CONTRAST as C, HUE as U, SATURATION as S, NO_IGNORE, Plan

from _aug_cases import COL, IGNORE, identity_lut, restore_state, save_state, source  # noqa: F401  (one copy; re-exported)


def _plan(H, W, rh, rw, h, w, corners=None, Hc=None, Wc=None, **kw):
    Hc, Wc = Hc or max(rh, h), Wc or max(rw, w)
    if corners is None:
        corners = [((Hc - h) // 2, (Wc - w) // 3)]
    kw.setdefault("ignore", IGNORE)
    return Plan(H=H, W=W, rh=rh, rw=rw, Hc=Hc, Wc=Wc, pt=0, pl=0, h=h, w=w, corners=corners, **kw)


def eight_chain_plans():
    """[(name, (H, W), plan)]; sources 37 x 53 and 33 x 65."""
    a, b = (37, 53), (33, 65)
    ten = [(y, x) for y, x in ((0, 0), (3, 5), (21, 29), (10, 10), (1, 28), (20, 0), (7, 19), (15, 3), (2, 2), (12, 25))]
    return [
        ("pad blur colour", a, _plan(*a, 37, 53, 32, 48, perm=(C, B, S, U), chain=(("pad", 2, 2), ("blur", 3), ("colour",)), **COL)),
        ("colour blur", b, _plan(*b, int(33 * 2.2), int(65 * 1.8), 32, 48, perm=(B, U, C, S), chain=(("colour",), ("blur", 4)), **COL)),
        ("blur flipped", a, _plan(*a, 37, 53, 32, 48, flip=True, chain=(("blur", 5),), **COL)),
        ("pad only", b, _plan(*b, 33, 65, 33, 65, normalise=False, chain=(("pad", 2, 2),), **COL)),
        # Resize(target_size=[40, 61], fit_stride=32): the canvas grows bottom and right to 64 x 64
        ("resize fit_stride", a, _plan(*a, 40, 61, 64, 64, Hc=64, Wc=64, corners=[(0, 0)], perm=(S, C), chain=(("colour",), ("blur", 3)), **COL)),
        ("no ignore ten candidates", a, _plan(*a, 37, 53, 16, 24, corners=ten, max_ratio=0.75, ignore=NO_IGNORE, perm=(U, B),
                                              chain=(("pad", 0, 3), ("colour",)), **COL)),
        ("colour through the chain", b, _plan(*b, 17, 30, 16, 24, perm=(U, S, B, C), chain=(("colour",),), **COL)),
        ("blur 6 on 16 x 24", a, _plan(*a, int(37 * 0.45), int(53 * 0.55), 16, 24, flip=True, chain=(("blur", 6),), **COL)),
    ]


def structured(H, W, C=3, seed=0):
    """uint8 [H, W, C]: an impulse row, an impulse column, lit corners, the right half noise."""
    rng = np.random.default_rng((seed, H, W))
    img = np.zeros((H, W, C), dtype=np.uint8)
    img[H // 2] = 255
    img[:, W // 3] = 255
    img[0, 0] = img[0, -1] = img[-1, 0] = img[-1, -1] = 255
    img[:, W // 2:] = rng.integers(0, 256, (H, W - W // 2, C))
    return img
