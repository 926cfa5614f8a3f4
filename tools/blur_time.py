"""Time of the blur / pad / colour kernels of libdcl_blur.so against the torch composition, in one process on one GPU.

    python tools/blur_time.py [--warmup 3] [--iters 10] [--out profiles/blur_time.json]

Rows, HIP-event medians of ``--iters`` runs, images resident on the GPU:
  blur      dbl_blur alone on 3 x 512 x 1024, R = 3 .. 6, against ``augment.gaussian_blur`` on the same tensor; GB/s of the
            algorithmic traffic (two kernels x (read + write) x 6.29 MB) next to the card's 8 TB/s
  cadis     DeviceAugment on 8 images of 540 x 960 with ['pad', 'flip', 'blur', 'colorjitter', 'torchvision_normalise'], blur_p 1
            and 0.05, DCL_BLUR_HIP on and off
  cityscapes  DeviceAugment on 12 images of 1024 x 2048 -> 512 x 1024 with and without the 'blur' key at the default probability
Not a test: nothing is asserted about the ratios."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mscs_amd  # noqa: E402,F401
from mscs_amd import _lib_blur as lb  # noqa: E402
from mscs_amd.datasets import SyntheticRaw  # noqa: E402
from mscs_amd.datasets import augment as A  # noqa: E402
from mscs_amd.debug import cfg as dbg  # noqa: E402

PEAK_GBS = 8000.0
CTS = ["flip", "random_scale", "RandomCropImgLbl", "colorjitter", "torchvision_normalise"]
CTS_VALUES = {"crop_shape": [512, 1024], "crop_class_max_ratio": 0.75, "scale_range": [0.5, 2]}
CADIS = ["pad", "flip", "blur", "colorjitter", "torchvision_normalise"]


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


def blur_rows(dev, warmup, iters):
    src = torch.rand(3, 512, 1024, device=dev) * 255
    dst, scratch = torch.empty_like(src), torch.empty_like(src)
    hwc = src.permute(1, 2, 0).contiguous()
    st = lb.stream_ptr(dev)
    rows = []
    for R in (3, 4, 5, 6):
        k = timed(lambda: lb.blur(src, dst, scratch, R, st), warmup, iters)
        t = timed(lambda: A.gaussian_blur(hwc, R), warmup, iters)
        nbytes = 2 * 2 * src.numel() * 4
        rows.append({"radius": R, "taps_a_pass": 2 * A.box_of(R)[0] + 3, "kernels": k, "torch_composition_gpu": t,
                     "algorithmic_gb_per_s": nbytes / (k["median_ms"] * 1e-3) / 1e9,
                     "share_of_8_tb_per_s": nbytes / (k["median_ms"] * 1e-3) / 1e9 / PEAK_GBS,
                     "max_abs_diff": float((dst.permute(1, 2, 0) - A.gaussian_blur(hwc, R)).abs().max())})
    return rows


def batch_row(dev, name, dataset, experiment, transforms, values, sizes, warmup, iters):
    planner = A.planner_for(transforms, values, dataset, experiment, 1)
    items = [SyntheticRaw(len(sizes), s, dataset, experiment, planner, seed=1)[n] for n, s in enumerate(sizes)]
    imgs, lbls, plans = [i[0].to(dev) for i in items], [i[1].to(dev) for i in items], [i[2]["plan"] for i in items]
    aug = A.DeviceAugment(A.network_lut(dataset, experiment))
    row = {"batch": name, "images": len(sizes), "with_a_chain": sum(bool(p.chain) for p in plans),
           "blurred": sum(any(c[0] == "blur" for c in p.chain) for p in plans)}
    old = dbg.blur_hip
    try:
        for key, on in (("DCL_BLUR_HIP=1", True), ("DCL_BLUR_HIP=0", False)):
            dbg.blur_hip = on
            aug(imgs, lbls, plans)
            row[key] = dict(timed(lambda: aug(imgs, lbls, plans), warmup if on else 1, iters), paths=sorted(set(aug.last_paths)))
    finally:
        dbg.blur_hip = old
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blur_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/blur_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    lb.lib()
    cadis = [(540, 960)] * 8
    cts = [(1024, 2048)] * 12
    res = {"device": torch.cuda.get_device_name(0), "method": f"HIP-event medians of {a.iters} runs, one process",
           "blur_3x512x1024": blur_rows(dev, a.warmup, a.iters),
           "batches": [
               batch_row(dev, "cadis 8 x (540 x 960), blur_p 1", "CADIS", 2, CADIS, {"blur_p": 1}, cadis, a.warmup, a.iters),
               batch_row(dev, "cadis 8 x (540 x 960), blur_p 0.05", "CADIS", 2, CADIS, {}, cadis, a.warmup, a.iters),
               batch_row(dev, "cityscapes 12 x (1024 x 2048) -> 512 x 1024, no blur key", "CITYSCAPES", 1, CTS, CTS_VALUES, cts,
                         a.warmup, a.iters),
               batch_row(dev, "cityscapes 12 x (1024 x 2048) -> 512 x 1024, blur key at p 0.05", "CITYSCAPES", 1,
                         CTS[:3] + ["blur"] + CTS[3:], CTS_VALUES, cts, a.warmup, a.iters)]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
