"""Time and peak memory of ``predict_maps`` with both tables: the HIP kernel (libdcl_pred.so) against the torch composition of the
same commit (materialize / argmax / two table look-ups), on random logits, HIP-event medians on one GPU.

    python tools/pred_time.py [--warmup 3] [--iters 10] [--configs cts,ade,cts_dense,ade_dense] [--out profiles/pred_time.json]

cts:       C = 19, logits 256 x 512 resized to 1024 x 2048 (align_corners on), as an UpsampledLogits
ade:       C = 150, logits 128 x 128 resized to 512 x 512
cts_dense, ade_dense: the same two outputs from dense full-size logits (the identity level: what a TTA wrapper hands over)
Every config runs in a child process of its own under its own time limit; the first one that fails or runs out of time ends the
run.  Peak memory is what a call allocates beyond its input.  Not a test: nothing is asserted about the ratios."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"cts": (19, 256, 512, 1024, 2048, False), "ade": (150, 128, 128, 512, 512, False),
           "cts_dense": (19, 256, 512, 1024, 2048, True), "ade_dense": (150, 128, 128, 512, 512, True)}


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


def child(a):
    import torch
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_pred as lp
    from mscs_amd.debug import cfg as dbg
    from mscs_amd.models.ops_logits import UpsampledLogits
    from mscs_amd.utils import class_palette, predict_maps, submission_lut
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    lp.lib()
    C, h, w, H, W, dense = CONFIGS[a.child]
    g = torch.Generator(device=dev).manual_seed(0)
    z = torch.randn(1, C, h, w, device=dev, generator=g) * 2
    dataset = "CITYSCAPES" if C == 19 else "ADE20K"
    lut, pal = submission_lut(dataset, 1).to(dev), class_palette(dataset, 1).to(dev)
    if dense:
        z = torch.nn.functional.interpolate(z, size=(H, W), mode="bilinear", align_corners=True).contiguous()

    def step(hip):
        dbg.pred_hip = hip
        out = z if dense else UpsampledLogits(z, (H, W), True)      # (a fresh object: nothing materialised is kept between calls)
        return predict_maps(out, lut, pal)
    with torch.no_grad():
        outs = {name: step(hip) for name, hip in (("hip", True), ("eager", False))}
        torch.cuda.synchronize()
        row = {"config": a.child, "C": C, "h": h, "w": w, "H": H, "W": W, "dense": dense,
               "ids_differ": int((outs["hip"][0] != outs["eager"][0]).sum()),
               "full_logits_mib": C * H * W * 4 / 2 ** 20, "outputs_mib": 5 * H * W / 2 ** 20}
        del outs
        # alternate the two sides so that a drift of the machine hits both
        row["hip"] = timed(lambda: step(True), a.warmup, a.iters, dev)
        row["eager"] = timed(lambda: step(False), a.warmup, a.iters, dev)
        row["hip_again"] = timed(lambda: step(True), a.warmup, a.iters, dev)
    row["eager_over_hip"] = row["eager"]["median_ms"] / row["hip"]["median_ms"]
    row["device"] = torch.cuda.get_device_name(0)
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--configs", default="cts,ade,cts_dense,ade_dense")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pred_time.json"))
    ap.add_argument("--timeout", type=int, default=120, help="seconds, per config")
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
    res = {"device": device, "what": "predict_maps with both tables on one image, kernel (hip) against the torch composition (eager) "
           "on random logits; HIP-event medians (ms) with min / max, peak MiB beyond the input; hip_again = the kernel timed once "
           "more after the composition; ids_differ = pixels whose class differs between the two (near-ties)", "warmup": a.warmup,
           "iters": a.iters, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
