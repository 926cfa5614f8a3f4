#!/usr/bin/env python3
"""CaDIS input-path fixtures from the REFERENCE utils/repeat_factor_sampling.py, utils/transforms.py and utils/np_transforms.py,
run on the CPU (build container only; needs pandas, which the product does not).  They are named tests/golden/cadis_*, without a
G<n> prefix: a name that starts with G2 would join the loss fixtures that tests/test_oracle.py and others collect by prefix.

tests/golden/cadis_frames_v1_v5.csv: the rows of videos 1 and 5 (split 0: train / validation) of the reference's data/data.csv, every
column, in the table's order.

tests/golden/cadis_rfs_exp<2|3>.npz, from RepeatFactorSampler(dataframe = that excerpt, split=0, experiment, repeat_thresh=0.15):
``class_ids`` / ``class_factors`` (float64), ``image_factors`` (float32, one per frame of video 1 that is not blacklisted),
``epoch0`` / ``epoch1`` (the index lists of two successive epochs of ONE sampler at world size 1) and ``w2_rank0`` / ``w2_rank1``
(epoch 0 of a fresh sampler per rank at world size 2).

tests/golden/cadis_transforms.npz, on the seeded 37 x 53 source of tests/_aug_cases.source (seed 7): the outputs of
Resize(target_size=[64, 96], fit_stride=32), of PadNP(ver=(2, 2), hor=(0, 0), 'reflect') and of BlurPIL(probability=1,
kernel_limits=(3, 7)) under numpy seeds 0 .. 5, each with the radius it drew.

Stand-ins on top of tools/ref_shim.py: this torch's ``Sampler.__init__`` refuses the ``data_source`` argument that the reference's
sampler passes to it, so the constructor is relaxed here to take and drop it; the world size and rank, which the reference's module
reads from torch.distributed through three helpers, are given by replacing those helpers in its namespace.  The reference is
imported at run time; none of its text is here."""
import builtins
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: E402

ref_shim.install()
ref_shim.quiet()
torch.utils.data.Sampler.__init__ = lambda self, *a, **k: None

_print = builtins.print
builtins.print = lambda *a, **k: None
import pandas as pd  # noqa: E402
from utils.np_transforms import PadNP  # noqa: E402  (the reference's)
import utils.repeat_factor_sampling as ref_rfs  # noqa: E402
from utils.transforms import BlurPIL, Resize  # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)


def excerpt():
    import csv
    with open(os.path.join(ref_shim.REFERENCE_ROOT, "data", "data.csv"), newline="") as f:
        rows = list(csv.reader(f))
    vid = rows[0].index("vid_num")
    path = os.path.join(OUT, "cadis_frames_v1_v5.csv")
    with open(path, "w", newline="") as f:
        csv.writer(f, lineterminator="\n").writerows([rows[0]] + [r for r in rows[1:] if r[vid] in ("1", "5")])
    return path


def sampler(df, experiment, world=1, rank=0):
    ref_rfs.get_world_size, ref_rfs.get_rank, ref_rfs.is_distributed = (lambda: world), (lambda: rank), (lambda: world > 1)
    return ref_rfs.RepeatFactorSampler(data_source=None, dataframe=df.copy(), repeat_thresh=0.15, experiment=experiment, split=0)


def samplers(path):
    df = pd.read_csv(path)
    for experiment in (2, 3):
        s = sampler(df, experiment)
        ids = sorted(s.class_repeat_factors)
        out = dict(class_ids=np.asarray(ids, dtype=np.int64),
                   class_factors=np.asarray([s.class_repeat_factors[c] for c in ids], dtype=np.float64),
                   image_factors=s.repeat_factors.numpy())
        for epoch in (0, 1):
            s.set_epoch(epoch)
            out[f"epoch{epoch}"] = np.asarray(list(iter(s)), dtype=np.int64)
        for rank in (0, 1):                         # (the module-level rank is read again while iterating: one rank at a time)
            r = sampler(df, experiment, world=2, rank=rank)
            r.set_epoch(0)
            out[f"w2_rank{rank}"] = np.asarray(list(iter(r)), dtype=np.int64)
        np.savez_compressed(os.path.join(OUT, f"cadis_rfs_exp{experiment}.npz"), **out)
        f = out["image_factors"]
        _print(f"experiment {experiment}: {len(f)} frames, {int((f > 1).sum())} with a factor above 1, max {f.max():.3f}, "
               f"{len(out['epoch0'])} / {len(out['epoch1'])} indices in epochs 0 / 1, {len(out['w2_rank0'])} + {len(out['w2_rank1'])} "
               "at world size 2")


def transforms():
    from _aug_cases import source
    img, lbl = (t.numpy() for t in source(37, 53, 7))
    out = dict(img=img, lbl=lbl)
    out["resize_img"], out["resize_lbl"] = Resize("CADIS", 2, target_size=[64, 96], fit_stride=32)((img, lbl))
    pad = PadNP(ver=(2, 2), hor=(0, 0), padding_mode="reflect")
    out["pad_img"], out["pad_lbl"] = pad(img), pad(lbl)
    blur = BlurPIL("CADIS", 2, probability=1, kernel_limits=(3, 7))
    radii = []
    for seed in range(6):
        np.random.seed(seed)
        np.random.random()
        radii.append(np.random.randint(3, 7))
        np.random.seed(seed)
        out[f"blur{seed}"] = blur(img)
    out["blur_radii"] = np.asarray(radii, dtype=np.int64)
    np.savez_compressed(os.path.join(OUT, "cadis_transforms.npz"), **out)
    _print("Resize ->", out["resize_img"].shape, out["resize_lbl"].shape, " PadNP ->", out["pad_img"].shape, " blur radii", radii)


if __name__ == "__main__":
    path = excerpt()
    _print(path, os.path.getsize(path), "bytes")
    samplers(path)
    transforms()
