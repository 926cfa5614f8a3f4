"""Time of the on-device input augmentation (libdcl_aug.so) against the torch composition on the GPU and against the reference's PIL
pipeline on one CPU core, and of the manager's training step on the raw input path against the same step on ``data.synthetic``, in
one process on one GPU.

    python tools/aug_time.py [--warmup 3] [--iters 10] [--no-step] [--steps 10] [--out profiles/aug_time.json]

Batch rows: 12 images of 1024 x 2048 -> crops of 512 x 1024 (the Cityscapes config) and 16 images of ADE20K-like sizes -> crops of
512 x 512, plans drawn by the planner from the reference's shipped transform lists; images resident on the GPU, HIP-event medians
over whole batches (3 launches per image).  PIL row: flip, resize (BILINEAR / NEAREST), pad, the crop search with its label
histograms, the four colour operations, normalise, per image on one thread, host clock (only where PIL is installed).  Step rows:
``BaseManager`` training steps (upload + augmentation on the input stream, forward, loss, backward, optimiser) over pre-fetched pinned
batches, ``synthetic_raw`` against ``synthetic``, alternating blocks, host clock around a device synchronise.  Not a test: nothing
is asserted about the ratios."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mscs_amd  # noqa: E402,F401
from mscs_amd import _lib_aug as la  # noqa: E402
from mscs_amd.datasets import augment as A  # noqa: E402
from mscs_amd.debug import cfg as dbg  # noqa: E402

TRAIN = ["flip", "random_scale", "RandomCropImgLbl", "colorjitter", "torchvision_normalise"]
# max |fp32 composition - float64 composition| over the eight plans of tests/_aug_cases.py, on the CPU, and the kernels' bound
COMPOSITION_FP32_ERR = 3.944450296500257e-06
ADE_SIZES = [(512, 683), (683, 512), (256, 341), (600, 800), (480, 640), (375, 500), (768, 1024), (512, 512)]


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def make_batch(dataset, sizes, crop, seed):
    planner = A.AugmentPlanner(TRAIN, {"crop_shape": list(crop), "crop_class_max_ratio": 0.75, "scale_range": [0.5, 2]}, dataset, 1, seed)
    from mscs_amd.datasets import SyntheticRaw
    imgs, lbls, plans = [], [], []
    for n, (H, W) in enumerate(sizes):
        img, lbl, meta = SyntheticRaw(len(sizes), (H, W), dataset, 1, planner, seed=seed)[n]
        imgs.append(img)
        lbls.append(lbl)
        plans.append(meta["plan"])
    return imgs, lbls, plans


def batch_rows(dev, name, dataset, sizes, crop, warmup, iters):
    imgs, lbls, plans = make_batch(dataset, sizes, crop, seed=1)
    aug = A.DeviceAugment(A.network_lut(dataset, 1))
    gi, gl = [t.to(dev) for t in imgs], [t.to(dev) for t in lbls]
    row = {"batch": name, "images": len(sizes), "crop": list(crop), "candidates": [len(p.corners) for p in plans],
           "resized": [[p.rh, p.rw] for p in plans]}
    old = dbg.aug_hip
    try:
        dbg.aug_hip = True
        x, y = aug(gi, gl, plans)
        assert aug.last_paths == ["hip"] * len(sizes), aug.last_paths
        row["kernels"] = timed(lambda: aug(gi, gl, plans), warmup, iters)
        dbg.aug_hip = False
        ex, ey = aug(gi, gl, plans)
        row["torch_composition_gpu"] = timed(lambda: aug(gi, gl, plans), 1, max(3, iters // 3))
    finally:
        dbg.aug_hip = old
    row["labels_equal"] = bool(torch.equal(y, ey))
    row["max_abs_diff_kernels_vs_composition_fp32"] = float((x - ex).abs().max())
    row["kernels_per_image_ms"] = row["kernels"]["median_ms"] / len(sizes)
    return row


def pil_pipeline(img, lbl, plan, lut):
    """The reference's CPU work for one sample with the plan's draws: FlipNP, RandomResize (+ pad), RandomCropImgLbl with its
    histograms, ColorJitter on the PIL image, ToTensor + Normalize."""
    from PIL import Image, ImageEnhance
    lbl = lut[lbl]
    if plan.flip:
        img, lbl = np.flip(img, axis=1), np.flip(lbl, axis=1)
    pi, pl_ = Image.fromarray(np.ascontiguousarray(img)), Image.fromarray(np.ascontiguousarray(lbl))
    if (plan.rh, plan.rw) != (plan.H, plan.W):
        pi, pl_ = pi.resize((plan.rw, plan.rh), Image.BILINEAR), pl_.resize((plan.rw, plan.rh), Image.NEAREST)
    ai, al = np.array(pi), np.array(pl_)
    if (plan.Hc, plan.Wc) != (plan.rh, plan.rw):
        pad = ((plan.pt, plan.Hc - plan.rh - plan.pt), (plan.pl, plan.Wc - plan.rw - plan.pl))
        ai = np.pad(ai, pad + ((0, 0),), mode="constant", constant_values=0)
        al = np.pad(al, pad, constant_values=plan.ignore)
    chosen = len(plan.corners) - 1
    for p, (i, j) in enumerate(plan.corners):
        classes, cnt = np.unique(al[i:i + plan.h, j:j + plan.w], return_counts=True)
        cnt = cnt[classes != plan.ignore]
        if len(cnt) > 1 and np.max(cnt) / np.sum(cnt) < (plan.max_ratio or 0):
            chosen = p
            break
    i, j = plan.corners[chosen]
    pi = Image.fromarray(np.ascontiguousarray(ai[i:i + plan.h, j:j + plan.w]))
    al = al[i:i + plan.h, j:j + plan.w]
    for op in plan.perm:
        if op == A.BRIGHTNESS:
            pi = ImageEnhance.Brightness(pi).enhance(plan.b)
        elif op == A.CONTRAST:
            pi = ImageEnhance.Contrast(pi).enhance(plan.c)
        elif op == A.SATURATION:
            pi = ImageEnhance.Color(pi).enhance(plan.s)
        else:
            h, s, v = pi.convert("HSV").split()
            nh = np.array(h, dtype=np.uint8)
            with np.errstate(over="ignore"):
                nh += np.uint8(int(plan.delta * 255) % 256)
            pi = Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")
    x = np.asarray(pi, dtype=np.float32).transpose(2, 0, 1) / 255.0
    if plan.normalise:
        x = (x - np.asarray(A.MEAN, dtype=np.float32)[:, None, None]) / np.asarray(A.STD, dtype=np.float32)[:, None, None]
    return np.ascontiguousarray(x), al.astype(np.int64)


def pil_row(name, dataset, sizes, crop):
    try:
        import PIL  # noqa: F401
    except ImportError:
        return {"batch": name, "pil": "not installed"}
    imgs, lbls, plans = make_batch(dataset, sizes, crop, seed=1)
    lut = A.network_lut(dataset, 1).numpy()
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    ms = []
    try:
        for img, lbl, plan in zip(imgs, lbls, plans):
            t0 = time.perf_counter()
            pil_pipeline(img.numpy(), lbl.numpy(), plan, lut)
            ms.append((time.perf_counter() - t0) * 1e3)
    finally:
        torch.set_num_threads(threads)
    return {"batch": name, "pil_one_core_per_image_ms": {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)},
            "images_per_s_one_core": 1e3 / statistics.median(ms)}


def step_config(raw):
    data = {"dataset": "CITYSCAPES", "experiment": 1, "batch_size": 12, "num_workers": 0, "synthetic": True,
            "synthetic_length": 48, "synthetic_mode": "blocky", "transform_values": {"crop_shape": [512, 1024]}}
    if raw:
        data.update({"synthetic_raw": True, "synthetic_raw_size": [1024, 2048], "transforms": TRAIN,
                     "transform_values": {"crop_shape": [512, 1024], "crop_class_max_ratio": 0.75, "scale_range": [0.5, 2]}})
    return {"name": "aug_time", "mode": "training", "manager": "HRNet", "cuda": True, "seed": 0, "parallel": False,
            "gpu_device": [0], "save_checkpoints": False,
            "graph": {"model": "HRNet", "backbone": "hrnet48", "sync_bn": True, "out_stride": 4, "pretrained": False,
                      "align_corners": True,
                      "ms_projector": {"mlp": [[1, -1, 1]], "scales": 3, "d": 256, "use_bn": True, "before_context": True}},
            "data": data,
            "loss": {"name": "LossWrapper", "losses": {"CrossEntropyLoss": 1, "DenseContrastiveLossV2_ms": 0.1},
                     "dataset": "CITYSCAPES", "experiment": 1, "temperature": 0.1, "scales": 3, "weights": [1.0, 0.7, 0.4],
                     "cross_scale_contrast": True, "min_views_per_class": 5, "max_views_per_class": 2500,
                     "max_features_total": 10000, "label_scaling_mode": "nn"},
            "train": {"learning_rate": 0.01, "lr_fct": "polynomial", "optim": "SGD", "lr_batchwise": True, "epochs": 484,
                      "momentum": 0.9, "weight_decay": 0.0005}}


def step_rows(dev, warmup, steps):
    from mscs_amd.managers import HRNetManager
    from mscs_amd.utils import set_verbosity
    set_verbosity(40)
    runs = {}
    for key in ("synthetic", "synthetic_raw"):
        mgr = HRNetManager(step_config(key == "synthetic_raw"), autostart=False)
        mgr.setup()
        mgr.model.train()
        batches = []
        for n, b in enumerate(mgr.data_loaders["train_loader"]):        # pre-fetched (the loader pins them): the datasets' own
            batches.append(b)                                          # pixel generation is not what is compared
            if n == 3:
                break

        def block(k, mgr=mgr, batches=batches):
            t0 = time.perf_counter()
            for i in range(k):
                img, lbl, ready = mgr._upload(*batches[i % len(batches)][:3])
                mgr.optimiser.zero_grad(set_to_none=True)
                ret = mgr.forward_step(img, lbl, label_ready=ready)
                ret["loss"].backward()
                mgr.optimiser.step()
                mgr.scheduler.step()
                mgr.step_metrics(1, ret, lbl, 0.0)
            torch.cuda.synchronize()
            mgr.flush_logging()
            assert bool(torch.isfinite(ret["loss"]))
            return (time.perf_counter() - t0) * 1e3 / k
        block(warmup)
        runs[key] = block
    out = {k: [] for k in runs}
    for _ in range(3):                                                  # alternating blocks
        for k, block in runs.items():
            out[k].append(block(steps))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "blocks_of": steps} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aug_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/aug_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    la.lib()
    batches = [("cityscapes 12 x (1024 x 2048) -> 512 x 1024", "CITYSCAPES", [(1024, 2048)] * 12, (512, 1024)),
               ("ade20k 16 x mixed sizes -> 512 x 512", "ADE20K", ADE_SIZES * 2, (512, 512))]
    res = {"device": torch.cuda.get_device_name(0), "method": "HIP-event medians over whole batches; host clock for PIL and the step",
           "accuracy": {"fp32_composition_vs_float64_max_abs_err_cpu": COMPOSITION_FP32_ERR,
                        "kernel_bound_4x": 4 * COMPOSITION_FP32_ERR,
                        "note": "eight plans of tests/_aug_cases.py; the kernels' own figure is printed by tests/test_aug_hip.py"},
           "batches": [batch_rows(dev, *b, a.warmup, a.iters) for b in batches],
           "pil": [pil_row(b[0], b[1], b[2], b[3]) for b in batches]}
    if not a.no_step:
        res["training_step_hrnet48_batch12"] = step_rows(dev, a.warmup, a.steps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
