"""Forward + backward time of the Lovasz-Softmax loss: the HIP kernels against the PyTorch path (DCL_LOVASZ_HIP=0), in one
process on one GPU, HIP-event medians.

    python tools/lovasz_time.py [--warmup 5] [--iters 20] [--torch-iters 20] [--out FILE]

Shapes: 12 x 19 x 512 x 1024 (Cityscapes crop, iid labels 0..19, 19 = ignore) and 16 x 150 x 512 x 512 (ADE20K, iid labels
0..150).  Also prints the bytes each stage of the HIP path moves (from the shapes) and the share of 8 TB/s that the measured
time of the whole forward + backward amounts to."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mscs_amd  # noqa: E402,F401
from mscs_amd import _lib_lovasz as lv  # noqa: E402
from mscs_amd.debug import cfg as dbg  # noqa: E402
from mscs_amd.losses import LovaszSoftmax  # noqa: E402

PEAK = 8.0e12


def stage_bytes(n, c, hw, per_image):
    """bytes each stage reads + writes, from the shapes (T elements, tiles of lv.TILE)"""
    t = n * c * hw
    s, l = (n * c, hw) if per_image else (c, n * hw)
    tiles = s * ((l + lv.TILE - 1) // lv.TILE)
    hist = 4 * 256 * tiles
    return [
        ("keys: logits read 3x, labels, key + payload written", 3 * 4 * t + 8 * n * hw + 8 * t),
        ("sort: 4 x (keys read, histograms written)", 4 * (4 * t + hist)),
        ("sort: 4 x (histograms scanned in place)", 4 * 2 * hist),
        ("sort: 4 x (key + payload read and written, histograms read)", 4 * (16 * t + hist)),
        ("scan: payload read for the tile counts", 4 * t),
        ("term + coefficients: key + payload read, coefficient scattered", 8 * t + 4 * t),
        ("backward: logits read 3x, coefficients read 2x, gradient written", 3 * 4 * t + 2 * 4 * t + 4 * t),
    ]


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
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--torch-iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.warmup >= 5 and a.iters >= 20 and a.torch_iters >= 20, "at least 5 warm-up and 20 timed iterations"
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    lines = [f"Lovasz-Softmax forward + backward, {torch.cuda.get_device_name(0)}, HIP-event medians "
             f"({a.warmup} warm-up, {a.iters} timed; PyTorch path {a.torch_iters} timed), ms"]
    for n, c, h, w, per_image in [(12, 19, 512, 1024, False), (12, 19, 512, 1024, True), (16, 150, 512, 512, False)]:
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(n, c, h, w, device=dev, generator=g).requires_grad_(True)
        lab = torch.randint(0, c + 1, (n, h, w), device=dev, generator=g)
        m = LovaszSoftmax({"dataset": "CITYSCAPES", "experiment": 1, "classes_to_ignore": c, "per_image": per_image})

        def step():
            x.grad = None
            m(x, lab).backward()
        res = {}
        for hip in (True, False):
            dbg.lovasz_hip = hip
            res[hip] = timed(step, a.warmup, a.iters if hip else a.torch_iters)
            loss = m(x, lab).item()
            res[hip] += (loss,)
        dbg.lovasz_hip = True
        sb = stage_bytes(n, c, h * w, per_image)
        total = sum(b for _, b in sb)
        lines.append(f"\n{n} x {c} x {h} x {w}{' per_image' if per_image else ''}: workspace "
                     f"{lv.workspace_bytes(n, c, h * w, per_image) / 1e9:.3f} GB")
        for hip in (True, False):
            med, lo, hi, loss = res[hip]
            lines.append(f"  {'HIP kernels ' if hip else 'PyTorch path'}  median {med:9.3f}  min {lo:9.3f}  max {hi:9.3f}  loss {loss:.7f}")
        lines.append(f"  PyTorch / HIP = {res[False][0] / res[True][0]:.1f}x")
        for what, b in sb:
            lines.append(f"    {b / 1e9:7.3f} GB  {what}")
        lines.append(f"    {total / 1e9:7.3f} GB in all: {total / PEAK * 1e3:.3f} ms at 8 TB/s = "
                     f"{100 * total / PEAK * 1e3 / res[True][0]:.1f} % of the measured HIP time")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
