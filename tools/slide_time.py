"""Time and peak memory of the sliding-window test-time augmentation with equal-size windows: the fused path (libdcl_slide.so,
models/ops_slide.py, TTAWrapperPC / TTAWrapperSlide) against the per-window torch composition of the same commit, which is the
reference's structure.  HIP-event medians on one GPU, both sides in the same process, alternating.

    python tools/slide_time.py [--warmup 3] [--iters 10] [--configs pc_merge,slide_merge,pc_forward,slide_forward]
                               [--out profiles/slide_time.json] [--timeout 420]

(a) merge only, logits given (random quarter-resolution logits of every window and its mirror; no model):
    pc_merge      PASCAL-Context: K = 59, image 375 x 500, crop 512, base 520, scales [0.5, 0.75, 1.0, 1.5, 2.0]
    slide_merge   ADE20K slide: K = 150, image 512 x 683, crop 512, strides (341, 341), scales [0.5, 1.0, 1.5], flip
    One step = crop batch + canvas + sum over the scales for every view of one image.  The crop batches are timed as a row of
    their own (``crops``) and are part of neither side's ``merge`` time.
(b) the whole ``forward`` of the wrapper around HRNet-W48 at the same shapes, the fused path for ``tta_window_batch`` in
    {1, 4, 8, 16} against the composition (one model call per window and orientation):
    pc_forward, slide_forward

Launches per view are recorded next to the times: the fused path's from the binding modules' counters and the model calls, the
composition's counted from its operations (per window: two resizes, flip, add, scale, exp, the canvas ``+=`` and the count ``+=``;
per view: the zero fills, the division, the resize and the final ``+=``).  Every config runs in a child process of its own under
its own time limit; the first one that fails or runs out of time ends the run.  Peak memory is what a step allocates beyond its
inputs, the model and its accumulator.  Not a test: nothing is asserted about the ratios."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PC = dict(K=59, H=375, W=500, crop=(512, 512), base=520, scales=[0.5, 0.75, 1.0, 1.5, 2.0])
SLIDE = dict(K=150, H=512, W=683, crop=(512, 512), strides=(341, 341), img_scale=(2048, 512), scales=[0.5, 1.0, 1.5], flip=True)
WINDOW_BATCHES = (1, 4, 8, 16)


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


def pc_views(c):
    """[(size, window, row starts, column starts, mirror)] of the PASCAL-Context protocol"""
    from mscs_amd.models import ops_slide
    strides = ops_slide.pc_strides(c["crop"])
    out = []
    for s in c["scales"]:
        nh, nw = ops_slide.cts_size(c["H"], c["W"], c["base"], s)
        rows = ops_slide.pc_windows_1d(max(nh, c["crop"][0]), c["crop"][0], strides[0])
        cols = ops_slide.pc_windows_1d(max(nw, c["crop"][1]), c["crop"][1], strides[1])
        out.append(((nh, nw), tuple(c["crop"]), [r[0] for r in rows], [q[0] for q in cols], True))
    return out


def slide_views(c):
    from mscs_amd.models import ops_slide
    out = []
    for s in c["scales"]:
        nh, nw = int(c["img_scale"][0] * s), int(c["img_scale"][1] * s)
        rows = ops_slide.windows_1d(nh, c["crop"][0], c["strides"][0])
        cols = ops_slide.windows_1d(nw, c["crop"][1], c["strides"][1])
        win = (rows[0][1] - rows[0][0], cols[0][1] - cols[0][0])
        for mirror in ((True, False) if c["flip"] else (False,)):
            out.append(((nh, nw), win, [r[0] for r in rows], [q[0] for q in cols], mirror))
    return out


def merge_only(c, views, pad, dev, warmup, iters):
    import torch
    from mscs_amd.models import ops_slide, ops_tta
    K, H, W = c["K"], c["H"], c["W"]
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(3, H, W, device=dev, generator=g)
    zs = []
    for size, win, rows_lo, cols_lo, mirror in views:
        N = len(rows_lo) * len(cols_lo)
        shape = (N, K, -(-win[0] // 4), -(-win[1] // 4))
        zs.append((torch.randn(shape, device=dev, generator=g) * 2, torch.randn(shape, device=dev, generator=g) * 2 if mirror else None))
    final = torch.zeros(K, H, W, device=dev)

    def step(hip):
        final.zero_()
        for (size, win, rows_lo, cols_lo, mirror), (z, zf) in zip(views, zs):
            if hip:
                canvas = ops_slide.gather(z, zf, win, True, rows_lo, cols_lo, torch.empty((K,) + size, device=dev))
                ops_tta.merge(canvas, size, False, False, final, True)
            else:
                canvas = ops_slide.gather_eager(z, zf, win, True, rows_lo, cols_lo, torch.empty((K,) + size, device=dev))
                ops_tta.merge_eager(canvas, size, False, False, final, True)
        return final

    def crop_step(hip):
        fn = ops_slide.crops if hip else ops_slide.crops_eager
        return [fn(x, size, rows_lo, cols_lo, win, pad, mirror) for size, win, rows_lo, cols_lo, mirror in views][-1]

    windows = [len(v[2]) * len(v[3]) for v in views]
    row = {"K": K, "H": H, "W": W, "scales": c["scales"], "views": len(views), "windows_per_view": windows,
           "launches_per_view": {"hip": {"gather": 1, "merge": 1, "crops": 1},
                                 "eager": [(8 if v[4] else 5) * n + 5 for v, n in zip(views, windows)]},
           "largest_canvas_mib": max(K * v[0][0] * v[0][1] for v in views) * 4 / 2 ** 20}
    outs = {name: step(hip).clone() for name, hip in (("hip", True), ("eager", False))}
    row["max_rel_diff"] = float(((outs["hip"] - outs["eager"]).abs() / outs["eager"].abs()).max())
    a, b = crop_step(True), crop_step(False)
    row["crops_max_abs_diff"] = float((a - b).abs().max())
    del outs, a, b
    # alternate the two sides so that a drift of the machine hits both
    row["merge"] = {"hip": timed(lambda: step(True), warmup, iters, dev), "eager": timed(lambda: step(False), warmup, iters, dev),
                    "hip_again": timed(lambda: step(True), warmup, iters, dev)}
    row["merge"]["eager_over_hip"] = row["merge"]["eager"]["median_ms"] / row["merge"]["hip"]["median_ms"]
    row["crops"] = {"hip": timed(lambda: crop_step(True), warmup, iters, dev), "eager": timed(lambda: crop_step(False), warmup, iters, dev)}
    row["crops"]["eager_over_hip"] = row["crops"]["eager"]["median_ms"] / row["crops"]["hip"]["median_ms"]
    return row


def forward(c, make, dataset, dev, warmup, iters):
    import torch
    from mscs_amd import _lib_slide as ls
    from mscs_amd import _lib_tta as lt
    from mscs_amd.debug import cfg as dbg
    from mscs_amd.models import HRNet
    torch.manual_seed(0)
    graph = {"dataset": dataset, "backbone": "hrnet48", "pretrained": False, "align_corners": True}
    model = HRNet(config=graph, experiment=1).to(dev).eval()
    assert model.num_classes == c["K"]
    x = torch.randn(1, 3, c["H"], c["W"], device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    model_calls = [0]
    model.register_forward_pre_hook(lambda m, a: model_calls.__setitem__(0, model_calls[0] + 1))

    def run(hip, wb):
        dbg.slide_hip = hip
        w = make(model)
        w.tta_window_batch = wb
        return w(x)

    row = {"K": c["K"], "H": c["H"], "W": c["W"], "scales": c["scales"], "model": "HRNet-W48"}
    ref = run(False, 8).clone()
    row["composition_model_calls"] = model_calls[0]
    row["rows"] = {}
    order = [("hip", wb) for wb in WINDOW_BATCHES]
    for name, wb in order[:2] + [("eager", 8)] + order[2:]:
        model_calls[0] = 0
        before = dict(ls.calls), lt.calls["merge"]
        out = run(name == "hip", wb)
        entry = {"model_calls": model_calls[0],
                 "launches": {"crops": ls.calls["crops"] - before[0]["crops"], "gather": ls.calls["gather"] - before[0]["gather"],
                              "merge": lt.calls["merge"] - before[1]},
                 "max_rel_diff_to_composition": float(((out - ref).abs() / ref.abs()).max())}
        del out
        entry.update(timed(lambda: run(name == "hip", wb), warmup, iters, dev))
        row["rows"][f"{name}_wb{wb}" if name == "hip" else "eager"] = entry
    best = min((k for k in row["rows"] if k != "eager"), key=lambda k: row["rows"][k]["median_ms"])
    row["fastest_fused"] = best
    row["eager_over_fastest_fused"] = row["rows"]["eager"]["median_ms"] / row["rows"][best]["median_ms"]
    return row


def child(a):
    import torch
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_slide as ls
    from mscs_amd.models import TTAWrapperPC, TTAWrapperSlide
    from mscs_amd.utils import set_verbosity
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    ls.lib()
    set_verbosity(40)
    pad = [-m / s for m, s in zip(TTAWrapperPC.MEAN, TTAWrapperPC.STD)]
    with torch.no_grad():
        if a.child == "pc_merge":
            row = merge_only(PC, pc_views(PC), pad, dev, a.warmup, a.iters)
        elif a.child == "slide_merge":
            row = merge_only(SLIDE, slide_views(SLIDE), [0.0] * 3, dev, a.warmup, a.iters)
        elif a.child == "pc_forward":
            row = forward(PC, lambda m: TTAWrapperPC(m, list(PC["scales"]), num_classes=PC["K"], crop_size=PC["crop"], base_size=PC["base"]),
                          "PASCALC", dev, a.warmup, a.iters)
        else:
            row = forward(SLIDE, lambda m: TTAWrapperSlide(m, list(SLIDE["scales"]), SLIDE["flip"], SLIDE["strides"], SLIDE["crop"],
                                                           num_classes=SLIDE["K"], img_scale=SLIDE["img_scale"]),
                          "ADE20K", dev, a.warmup, a.iters)
    row["config"] = a.child
    row["device"] = torch.cuda.get_device_name(0)
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--configs", default="pc_merge,slide_merge,pc_forward,slide_forward")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slide_time.json"))
    ap.add_argument("--timeout", type=int, default=420, help="seconds, per config")
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
    res = {"device": device, "what": "sliding-window test-time augmentation with equal-size windows of one image: the fused path (hip) "
           "against the per-window torch composition (eager); HIP-event medians (ms) with min / max, peak MiB beyond inputs, model and "
           "accumulator; hip_again = the kernels timed once more after the composition", "warmup": a.warmup, "iters": a.iters,
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
