"""Time and peak memory of ``evaluate_at_original`` (utils/evaluate.py): the HIP kernel (libdcl_eval.so) against the torch
composition of the same commit (materialize / slice / F.interpolate / argmax / bincount), in the same process, on random logits
and blocky raw ADE20K labels through the network table, HIP-event medians on one GPU.

    python tools/eval_time.py [--warmup 3] [--iters 10] [--configs ade,ade_large,ade_dense] [--out profiles/eval_time.json]

ade:        C = 150, logits 128 x 176 resized to 512 x 704 as an UpsampledLogits, crop 512 x 683, original size 375 x 500
ade_large:  the same map, original size 1536 x 2048
ade_dense:  ade from dense 512 x 704 logits (the stage-1 identity: what a TTA wrapper hands over)
Every config runs in a child process of its own under its own time limit; the first one that fails or runs out of time ends the
run.  Peak memory is what a call allocates beyond its inputs.  Not a test: nothing is asserted about the ratios."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

#                  C,   h,   w,   Hp,  Wp,  rh,  rw,  H0,   W0,   dense
CONFIGS = {"ade": (150, 128, 176, 512, 704, 512, 683, 375, 500, False),
           "ade_large": (150, 128, 176, 512, 704, 512, 683, 1536, 2048, False),
           "ade_dense": (150, 128, 176, 512, 704, 512, 683, 375, 500, True)}


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
    import numpy as np
    import torch
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_eval as le
    from mscs_amd.datasets import network_lut
    from mscs_amd.debug import cfg as dbg
    from mscs_amd.models.ops_logits import UpsampledLogits
    from mscs_amd.utils import evaluate_at_original
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    le.lib()
    C, h, w, Hp, Wp, rh, rw, H0, W0, dense = CONFIGS[a.child]
    g = torch.Generator(device=dev).manual_seed(0)
    z = torch.randn(1, C, h, w, device=dev, generator=g) * 2
    lut = network_lut("ADE20K", 1)
    raw_ids = np.nonzero(lut.numpy() < C)[0].astype(np.uint8)
    rng = np.random.default_rng(0)
    small = raw_ids[rng.integers(0, len(raw_ids), (-(-H0 // 32), -(-W0 // 32)))]
    label = torch.from_numpy(np.repeat(np.repeat(small, 32, 0), 32, 1)[:H0, :W0].copy()).to(dev)
    lut = lut.to(dev)
    if dense:
        z = torch.nn.functional.interpolate(z, size=(Hp, Wp), mode="bilinear", align_corners=False).contiguous()

    def step(hip):
        dbg.eval_hip = hip
        out = z if dense else UpsampledLogits(z, (Hp, Wp), False)      # (a fresh object: nothing materialised is kept between calls)
        return evaluate_at_original(out, label, (rh, rw), (H0, W0), False, "ADE20K", label_lut=lut, return_ids=True)
    with torch.no_grad():
        outs = {name: step(hip) for name, hip in (("hip", True), ("eager", False))}
        torch.cuda.synchronize()
        differ = outs["hip"][1] != outs["eager"][1]
        row = {"config": a.child, "C": C, "h": h, "w": w, "Hp": Hp, "Wp": Wp, "rh": rh, "rw": rw, "H0": H0, "W0": W0, "dense": dense,
               "ids_differ": int(differ.sum()), "cm_cells_differ": int((outs["hip"][0] != outs["eager"][0]).sum()),
               "mid_logits_mib": C * Hp * Wp * 4 / 2 ** 20, "out_logits_mib": C * H0 * W0 * 4 / 2 ** 20,
               "outputs_mib": (H0 * W0 + 4 * C * (C + 1)) / 2 ** 20}
        del outs, differ
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
    ap.add_argument("--configs", default="ade,ade_large,ade_dense")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_time.json"))
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
    res = {"device": device, "what": "evaluate_at_original with return_ids on one ADE20K image, kernel (hip) against the torch "
           "composition (eager) in the same process, random logits and blocky raw labels through the network table; HIP-event medians "
           "(ms) with min / max, peak MiB beyond the inputs; hip_again = the kernel timed once more after the composition; ids_differ "
           "= pixels whose class differs between the two (near-ties)", "warmup": a.warmup, "iters": a.iters, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
