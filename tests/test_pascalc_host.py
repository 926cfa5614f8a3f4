"""PASCAL-Context through the managers on the CPU: the raw reader (datasets/raw.py PascalC) on a folder written here, the label
lookup of experiment 1, and an HRNet-18 manager on that folder with ``resize_val``: ``validate()`` scores at the original label
sizes and ``infer()`` with ``tta`` runs TTAWrapperPC and saves at each image's original size.  On the code before the reader the
manager tests fail with NotImplementedError (no reader for dataset PASCALC)."""
import math
import os

import numpy as np
import pytest
import torch

import mscs_amd  # noqa: F401
from mscs_amd.utils import set_verbosity

SIZES = {"2008_000003": (37, 50), "2008_000009": (48, 33), "2009_000012": (40, 40)}     # stem -> (H, W): three different sizes


def _write(root, split, sizes=SIZES):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    os.makedirs(os.path.join(root, split, "image"))
    os.makedirs(os.path.join(root, split, "label"))
    labels = {}
    for i, (stem, (h, w)) in enumerate(sorted(sizes.items())):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, split, "image", stem + ".jpg"))
        lbl = np.repeat(np.repeat(rng.integers(1, 60, (-(-h // 8), -(-w // 8)), dtype=np.uint8), 8, 0), 8, 1)[:h, :w].copy()
        if i == 0:
            lbl[:5, :7] = 0                                                          # raw 0: the ignore class of experiment 1
        Image.fromarray(lbl, mode="L").save(os.path.join(root, split, "label", stem + ".png"))
        labels[stem] = lbl
    return labels


@pytest.fixture()
def quiet():
    import random
    state = (torch.get_rng_state(), np.random.get_state(), random.getstate())
    threads = torch.get_num_threads()
    torch.set_num_threads(4)
    set_verbosity(40)
    yield
    torch.set_num_threads(threads)
    torch.set_rng_state(state[0])
    np.random.set_state(state[1])
    random.setstate(state[2])


def test_reader_pairs_files_and_returns_raw_ids(tmp_path):
    from mscs_amd.datasets import PascalC
    from mscs_amd.datasets.raw import PascalC as same
    assert PascalC is same and (PascalC.dataset, PascalC.experiment) == ("PASCALC", 1)
    labels = _write(str(tmp_path), "val")
    ds = PascalC(str(tmp_path), "val")
    assert len(ds) == 3 and [os.path.basename(p) for p in ds.images] == [s + ".jpg" for s in sorted(SIZES)]
    seen_zero = False
    for i, stem in enumerate(sorted(SIZES)):
        img, lbl, meta = ds[i]
        assert img.dtype == torch.uint8 and tuple(img.shape) == SIZES[stem] + (3,)
        assert lbl.dtype == torch.uint8 and tuple(lbl.shape) == SIZES[stem]
        assert np.array_equal(lbl.numpy(), labels[stem])                             # decode only: raw ids
        assert meta["index"] == i and meta["img_filename"].endswith(stem + ".jpg") and meta["target_filename"].endswith(stem + ".png")
        assert "plan" not in meta
        seen_zero = seen_zero or bool((lbl == 0).any())
    assert seen_zero
    with pytest.raises(AssertionError, match="split"):
        PascalC(str(tmp_path), "test")
    # an image without a label, and a label without an image
    os.rename(tmp_path / "val" / "label" / "2009_000012.png", tmp_path / "val" / "label" / "2009_000013.png")
    with pytest.raises((FileNotFoundError, AssertionError)):
        PascalC(str(tmp_path), "val")
    os.remove(tmp_path / "val" / "image" / "2009_000012.jpg")
    with pytest.raises((FileNotFoundError, AssertionError)):
        PascalC(str(tmp_path), "val")


def test_network_lut_of_experiment_1():
    from mscs_amd.datasets import network_lut
    lut = network_lut("PASCALC", 1)
    assert int(lut[0]) == 59
    assert lut[1:60].tolist() == list(range(59))


def _cfg(root, tmp, **extra):
    cfg = {"name": "pc", "mode": "training", "manager": "HRNet", "cuda": False, "parallel": False, "gpu_device": [0], "seed": 3,
           "log_every_n_steps": 1000, "log_path": str(tmp), "run_id": "run0", "save_checkpoints": False, "data_path": str(root),
           "graph": {"model": "HRNet", "backbone": "hrnet18", "sync_bn": False, "pretrained": False, "align_corners": True},
           "data": {"dataset": "PASCALC", "experiment": 1, "batch_size": 1, "num_workers": 0, "split": ["train", "val"],
                    "transforms": ["RandomCropImgLbl", "torchvision_normalise"], "transform_values": {"crop_shape": [32, 32]},
                    "transforms_val": ["resize_val", "torchvision_normalise"],
                    "transform_values_val": {"min_side_length": 64, "fit_stride_val": 32}},
           "loss": {"name": "LossWrapper", "losses": {"CrossEntropyLoss": 1}},
           "train": {"learning_rate": 0.01, "lr_fct": "polynomial", "optim": "SGD", "lr_batchwise": True, "epochs": 1}}
    cfg.update(extra)
    return cfg


@pytest.mark.timeout(600)
def test_manager_validates_and_infers_at_the_original_sizes(tmp_path, quiet, monkeypatch):
    """(raises NotImplementedError without the feature: no reader for dataset PASCALC)"""
    Image = pytest.importorskip("PIL.Image")
    from mscs_amd.managers import HRNetManager
    from mscs_amd.models import TTAWrapperPC
    from mscs_amd.utils import evaluate as ev
    root = tmp_path / "data"
    _write(str(root), "train")
    _write(str(root), "val")
    m = HRNetManager(_cfg(root, tmp_path / "train"), autostart=False)
    m.setup()
    assert m._bare_model().num_classes == 59
    seen = []
    real = ev.evaluate_at_original

    def spy(*a, **k):
        seen.append((tuple(a[3]), a[5]))
        return real(*a, **k)
    monkeypatch.setattr(ev, "evaluate_at_original", spy)
    miou = m.validate()
    assert math.isfinite(miou) and 0.0 <= miou <= 1.0
    assert seen == [(SIZES[s], "PASCALC") for s in sorted(SIZES)]                    # scored at the original sizes
    path = m.save_checkpoint(path=str(tmp_path / "chk.pt"))

    mi = HRNetManager(_cfg(root, tmp_path / "infer", mode="inference", load_checkpoint=path, tta=True, tta_scales=[0.5],
                           save_outputs=True), autostart=False)
    mi.setup()
    calls = []
    forward = TTAWrapperPC.forward
    monkeypatch.setattr(TTAWrapperPC, "forward", lambda self, x, *a, **k: (calls.append(tuple(x.shape[-2:])), forward(self, x, *a, **k))[1])
    del seen[:]
    mious = mi.infer()
    assert len(calls) == 3 and len(seen) == 3, "infer() did not run TTAWrapperPC on every image"
    assert math.isfinite(float(mious["mean_iou"])) and list(mious["per_class_iou"].shape) == [59]
    assert mi.model.return_features is False and mi.model.lazy_eval_logits is False
    base = tmp_path / "infer" / "run0" / "outputs" / "val"
    assert sorted(os.listdir(base)) == ["debug", "submit"]
    for stem, (h, w) in SIZES.items():
        submit, debug = Image.open(base / "submit" / f"{stem}.png"), Image.open(base / "debug" / f"{stem}.png")
        assert submit.mode == "L" and debug.mode == "RGB" and submit.size == debug.size == (w, h)
