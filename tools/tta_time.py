"""Time and peak memory of the test-time-augmentation merge: the HIP kernels (libdcl_tta.so) against the torch composition of the
same commit, on random low-resolution logits (no model: its forward is the same on both sides), HIP-event medians on one GPU.

    python tools/tta_time.py [--warmup 3] [--iters 10] [--configs cts,ade] [--out profiles/tta_time.json] [--timeout 240]

cts: the Cityscapes evaluation shape through TTAWrapperCTS's merge: K = 19, image 1024 x 2048, scales [0.75, 1.25, 1.5, 1.75, 2]
     (+ the appended 1.0), crop 512 x 1024 with non-overlapping strides, flip; per scale the window accumulations and the canvas
     merge.  Logits at a quarter of the crop, align_corners on.
ade: the ADE20K shape through TTAWrapper's merge: K = 150, image 512 x 512, the same scales, both orientations.
One step = the merge of every view of one image.  Every config runs in a child process of its own under its own time limit; the
first one that fails or runs out of time ends the run.  Peak memory is what a step allocates beyond its inputs and its
accumulator.  Not a test: nothing is asserted about the ratios."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALES = [0.75, 1.25, 1.5, 1.75, 2, 1.0]


def timed(fn, warmup, iters, dev):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "peak_mib": (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20}


def _both(row, step, warmup, iters, dev):
    import torch
    outs = {}
    for name, hip in (("hip", True), ("eager", False)):
        outs[name] = step(hip).clone()
        torch.cuda.synchronize()
    ref = outs["eager"].abs().max()
    row["max_abs_diff_over_max"] = float((outs["hip"] - outs["eager"]).abs().max() / ref)
    del outs
    # alternate the two sides so that a drift of the machine hits both
    row["hip"] = timed(lambda: step(True), warmup, iters, dev)
    row["eager"] = timed(lambda: step(False), warmup, iters, dev)
    row["hip_again"] = timed(lambda: step(True), warmup, iters, dev)
    row["eager_over_hip"] = row["eager"]["median_ms"] / row["hip"]["median_ms"]
    return row


def cts(dev, warmup, iters):
    import torch
    from mscs_amd.models import ops_tta
    K, H, W, crop, base = 19, 1024, 2048, (512, 1024), 2048
    g = torch.Generator(device=dev).manual_seed(0)
    plans, zs = [], {}
    for s in SCALES:
        nh, nw = ops_tta.cts_size(H, W, base, s)
        if s < 1.0:
            rows, cols = [(0, nh)], [(0, nw)]
        else:
            rows, cols = ops_tta.windows_1d(nh, crop[0], crop[0]), ops_tta.windows_1d(nw, crop[1], crop[1])
        rc, cc = ops_tta.counts_1d(nh, rows).to(dev), ops_tta.counts_1d(nw, cols).to(dev)
        plans.append((nh, nw, rows, cols, rc, cc))
        for h0, h1 in rows:
            for w0, w1 in cols:
                key = (-(-(h1 - h0) // 4), -(-(w1 - w0) // 4))
                if key not in zs:
                    zs[key] = (torch.randn(K, *key, device=dev, generator=g) * 2, torch.randn(K, *key, device=dev, generator=g) * 2)
    final = torch.zeros(K, H, W, device=dev)

    def step(hip):
        accum = ops_tta.window_accum if hip else ops_tta.window_accum_eager
        merge = ops_tta.canvas_merge if hip else ops_tta.canvas_merge_eager
        final.zero_()
        for nh, nw, rows, cols, rc, cc in plans:
            canvas = torch.zeros(K, nh, nw, device=dev)
            for h0, h1 in rows:
                for w0, w1 in cols:
                    z, zf = zs[(-(-(h1 - h0) // 4), -(-(w1 - w0) // 4))]
                    accum(z, zf, (h1 - h0, w1 - w0), True, canvas, h0, w0, h1 - h0, w1 - w0)
            merge(canvas, rc, cc, final, True)
        return final
    windows = sum(len(p[2]) * len(p[3]) for p in plans)
    row = {"config": "cts", "K": K, "H": H, "W": W, "crop": list(crop), "scales": SCALES, "windows": windows,
           "largest_canvas_mib": max(K * p[0] * p[1] for p in plans) * 4 / 2 ** 20}
    return _both(row, step, warmup, iters, dev)


def ade(dev, warmup, iters):
    import torch
    from mscs_amd.models import ops_tta
    K, H, W = 150, 512, 512
    g = torch.Generator(device=dev).manual_seed(0)
    views = []
    for s in SCALES:
        hm, wm = int(s * H), int(s * W)
        views.append((torch.randn(K, -(-hm // 4), -(-wm // 4), device=dev, generator=g) * 2, (hm, wm)))
    acc = torch.zeros(K, H, W, device=dev)

    def step(hip):
        merge = ops_tta.merge if hip else ops_tta.merge_eager
        acc.zero_()
        for f in (0, 1):
            for z, size in views:
                merge(z, size, True, f == 0, acc, True)
        return acc
    row = {"config": "ade", "K": K, "H": H, "W": W, "scales": SCALES, "views": 2 * len(views),
           "largest_view_mib": max(K * v[1][0] * v[1][1] for v in views) * 4 / 2 ** 20}
    return _both(row, step, warmup, iters, dev)


def child(a):
    import torch
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_tta as lt
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    lt.lib()
    with torch.no_grad():
        row = {"cts": cts, "ade": ade}[a.child](dev, a.warmup, a.iters)
    row["device"] = torch.cuda.get_device_name(0)
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--configs", default="cts,ade")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta_time.json"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds, per config")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert a.warmup >= 3 and a.iters >= 10, "at least 3 warm-up and 10 timed iterations"
    if a.child:
        return child(a)
    rows, device = [], None
    for c in a.configs.split(","):
        # a fresh process per config, ended at its own time limit; a failure ends the run: nothing more is started on the GPU
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", c, "--warmup", str(a.warmup), "--iters", str(a.iters)],
                           capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"config {c} failed with status {r.returncode}: stopping")
        row = json.loads([l for l in r.stdout.splitlines() if l.startswith("ROW ")][-1][4:])
        device = row.pop("device")
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"device": device, "what": "merge of the test-time-augmentation views of one image, kernels (hip) against the torch "
           "composition (eager) on random low-resolution logits; HIP-event medians (ms) with min / max, peak MiB beyond inputs and "
           "accumulator; hip_again = the kernels timed once more after the composition", "warmup": a.warmup, "iters": a.iters,
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
