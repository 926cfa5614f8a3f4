"""Time and peak memory of OhemCrossEntropy on low-resolution logits: the kernels (libdcl_ohem.so between the two entries of the fused
up-sampling + cross-entropy) against the torch composition of the same commit (``ohem_reference``: up-sample, log-softmax, sort), and
against plain ``UpsampledLogits.cross_entropy`` -- what mining costs over the loss without it.  Forward + backward and forward alone,
random logits, HIP-event medians on one GPU, all in one process per shape.

    python tools/ohem_time.py [--warmup 3] [--iters 10] [--configs cts,ade] [--out profiles/ohem_time.json]

cts: Cityscapes, 12 x 19 x 128 x 256 -> 512 x 1024, class weights, thresh 0.9, min_kept 131072 (the public HRNet recipe)
ade: ADE20K,     16 x 150 x 128 x 128 -> 512 x 512, no weights, thresh 0.7, min_kept 100000 (the public defaults)
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

# name -> (dataset, N, C, h, w, H, W, align_corners, thresh, min_kept)
CONFIGS = {"cts": ("CITYSCAPES", 12, 19, 128, 256, 512, 1024, True, 0.9, 131072),
           "ade": ("ADE20K", 16, 150, 128, 128, 512, 512, False, 0.7, 100000)}


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
    from mscs_amd import _lib_ohem as oh
    from mscs_amd.debug import cfg as dbg
    from mscs_amd.losses.OhemCrossEntropy import OhemCrossEntropy
    from mscs_amd.models.ops_logits import UpsampledLogits
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    oh.lib()
    dataset, N, C, h, w, H, W, align, thresh, mk = CONFIGS[a.child]
    g = torch.Generator(device=dev).manual_seed(0)
    z = (3.0 * torch.randn(N, C, h, w, device=dev, generator=g)).requires_grad_(True)
    t = torch.randint(0, C, (N, H, W), device=dev, generator=g)
    t[torch.rand(N, H, W, device=dev, generator=g) < 0.1] = C
    fn = OhemCrossEntropy({"dataset": dataset, "experiment": 1, "device": dev, "ohem_thresh": thresh, "ohem_min_kept": mk})
    assert fn.ignore_label == C
    wt = fn._weight_on(dev)

    def step(kind, backward):
        z.grad = None
        lazy = UpsampledLogits(z, (H, W), align)                 # (a fresh object: nothing materialised is kept between calls)
        if kind == "plain_ce":
            loss = lazy.cross_entropy(t, weight=wt, ignore_index=C)
        else:
            dbg.ohem_hip = kind == "hip"
            loss = fn(lazy, t)
        if backward:
            loss.backward()
        return loss.detach()
    row = {"config": a.child, "N": N, "C": C, "h": h, "w": w, "H": H, "W": W, "thresh": thresh, "min_kept": mk,
           "full_logits_mib": N * C * H * W * 4 / 2 ** 20, "maps_mib": 20 * N * H * W / 2 ** 20}
    lh, le = step("hip", True), step("composition", True)
    torch.cuda.synchronize()
    row["loss_hip"], row["loss_composition"] = float(lh), float(le)
    # alternate the sides so that a drift of the machine hits all of them
    for backward, tag in ((True, "fwd_bwd"), (False, "fwd")):
        for kind in ("hip", "composition", "plain_ce", "hip"):
            key = f"{kind}_{tag}" + ("_again" if f"{kind}_{tag}" in row else "")
            row[key] = timed(lambda: step(kind, backward), a.warmup, a.iters, dev)
        row[f"composition_over_hip_{tag}"] = row[f"composition_{tag}"]["median_ms"] / row[f"hip_{tag}"]["median_ms"]
        row[f"hip_over_plain_ce_{tag}"] = row[f"hip_{tag}"]["median_ms"] / row[f"plain_ce_{tag}"]["median_ms"]
    row["device"] = torch.cuda.get_device_name(0)
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--configs", default="cts,ade")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ohem_time.json"))
    ap.add_argument("--timeout", type=int, default=150, help="seconds, per config")
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
    res = {"device": device, "what": "OhemCrossEntropy on an UpsampledLogits: kernels (hip) against the torch composition of the same "
           "commit (composition) and against plain UpsampledLogits.cross_entropy (plain_ce); forward + backward (fwd_bwd) and forward "
           "alone (fwd); HIP-event medians (ms) with min / max, peak MiB beyond the inputs; hip_*_again = the kernels timed once more "
           "after the others", "warmup": a.warmup, "iters": a.iters, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
