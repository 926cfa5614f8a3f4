"""Time of the dilated 3x3 convolution kernels (libdcl_dconv.so) against the eager path (ATen's convolution, i.e. the vendor
library) at the sizes DeepLabv3 runs them, in one process on one GPU, HIP-event medians.

    python tools/dconv_time.py [--warmup 3] [--iters 10] [--batch 16] [--no-step] [--out profiles/dconv_time.json]

Operator rows (ADE20K crops of 512 x 512, batch 16, ResNet-50): the ASPP branches 2048 -> 256 at dilations 12 / 24 / 36 on the 32 x 32
map of ``out_stride`` 16 and on the 64 x 64 map of ``out_stride`` 8; layer4's 512 -> 512 at dilation 2 (32 x 32) and 2 / 4 (64 x 64);
layer3's 256 -> 256 at dilation 2 (64 x 64).  Forward, data gradient and weight gradient are timed separately, the kernels through the
C entries on packed weights (the pack is timed on its own: it runs once per optimizer step), the eager path through
aten::convolution / aten::convolution_backward with one output selected.  Step rows: a whole DeepLabv3 training step (forward, CE,
backward) with the switch on and off.  Not a test: nothing is asserted about the ratios."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import mscs_amd  # noqa: E402,F401
from mscs_amd import _lib_dconv as ld  # noqa: E402
from mscs_amd.debug import cfg as dbg  # noqa: E402

SHAPES = [("aspp, out_stride 16", 2048, 256, 32, 32, (12, 24, 36)), ("aspp, out_stride 8", 2048, 256, 64, 64, (12, 24, 36)),
          ("layer4, out_stride 16", 512, 512, 32, 32, (2,)), ("layer4, out_stride 8", 512, 512, 64, 64, (2, 4)),
          ("layer3, out_stride 8", 256, 256, 64, 64, (2,))]


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


def operator(dev, n, ci, co, h, w, d, warmup, iters):
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(n, ci, h, w, device=dev, generator=g)
    wt = torch.randn(co, ci, 3, 3, device=dev, generator=g) / (3.0 * ci ** 0.5)
    gy = torch.randn(n, co, h, w, device=dev, generator=g)
    L, st = ld.lib(), ld.stream_ptr(dev)
    wamax = torch.empty(1, device=dev)
    wp = torch.empty(ld.packed_bytes(co, ci, False), dtype=torch.uint8, device=dev)
    wpt = torch.empty(ld.packed_bytes(co, ci, True), dtype=torch.uint8, device=dev)
    nbytes = [ld.workspace_bytes(op, n, ci, co, h, w, d) for op in (ld.FWD, ld.DGRAD, ld.WGRAD)]
    ws = torch.empty(max(nbytes), dtype=torch.uint8, device=dev)
    y, gx, gw = torch.empty_like(gy), torch.empty_like(x), torch.empty_like(wt)
    p = lambda t: t.data_ptr()
    hip = {
        "pack": lambda: ld.check(L.ddc_pack(p(wt), co, ci, p(wamax), p(wp), p(wpt), st), "ddc_pack"),
        "fwd": lambda: ld.check(L.ddc_fwd(p(x), p(wp), p(wamax), None, n, ci, co, h, w, d, p(ws), nbytes[0], p(y), st), "ddc_fwd"),
        "dgrad": lambda: ld.check(L.ddc_dgrad(p(gy), p(wpt), p(wamax), n, ci, co, h, w, d, p(ws), nbytes[1], p(gx), st), "ddc_dgrad"),
        "wgrad": lambda: ld.check(L.ddc_wgrad(p(x), p(gy), n, ci, co, h, w, d, p(ws), nbytes[2], p(gw), st), "ddc_wgrad"),
    }
    back = lambda mask: torch.ops.aten.convolution_backward(gy, x, wt, None, [1, 1], [d, d], [d, d], False, [0, 0], 1, mask)
    eager = {"fwd": lambda: F.conv2d(x, wt, None, 1, d, d), "dgrad": lambda: back([True, False, False]),
             "wgrad": lambda: back([False, True, False])}
    row = {"N": n, "Ci": ci, "Co": co, "H": h, "W": w, "d": d, "live_taps": bin(ld.live_taps(h, w, d)).count("1"),
           "wgrad_slabs": ld.wgrad_slabs(n, ci, co, h, w, d), "pack_hip": timed(hip["pack"], warmup, iters)}
    for k in ("fwd", "dgrad", "wgrad"):
        a, b = timed(hip[k], warmup, iters), timed(eager[k], warmup, iters)
        row[k] = {"hip": a, "eager": b, "eager_over_hip": b["median_ms"] / a["median_ms"]}
    # the two paths computed the same thing (a timing of a wrong result is worthless): the first image of both against the float64
    # convolution of the same fp32 inputs, max|. - fp64| / max|fp64|
    ref = F.conv2d(x[:1].double(), wt.double(), None, 1, d, d)
    den = float(ref.abs().max())
    row["fwd_hip_vs_fp64"] = float((y[:1].double() - ref).abs().max()) / den
    row["fwd_eager_vs_fp64"] = float((F.conv2d(x[:1], wt, None, 1, d, d).double() - ref).abs().max()) / den
    return row


def step(dev, out_stride, batch, warmup, iters):
    from mscs_amd.models import DeepLabv3
    from mscs_amd.utils import set_verbosity
    set_verbosity(40)
    res = {"out_stride": out_stride, "batch": batch, "image": [512, 512], "backbone": "resnet50", "dataset": "ADE20K"}
    g = torch.Generator().manual_seed(0)
    img = torch.randn(batch, 3, 512, 512, generator=g).to(dev)
    lbl = torch.randint(0, 150, (batch, 512, 512), generator=g).to(dev)
    for name, on in (("hip", True), ("eager", False)):
        dbg.dconv_hip = on
        torch.manual_seed(0)
        model = DeepLabv3({"dataset": "ADE20K", "backbone": "resnet50", "pretrained": False, "out_stride": out_stride}, 1).to(dev).train()

        def one():
            model.zero_grad(set_to_none=True)
            F.cross_entropy(model(img), lbl).backward()
        res[name] = timed(one, warmup, iters)
        del model
        torch.cuda.empty_cache()
    dbg.dconv_hip = True
    res["eager_over_hip"] = res["eager"]["median_ms"] / res["hip"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dconv_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "iters": args.iters,
           "what": "dilated 3x3 convolution, HIP-event medians (ms): libdcl_dconv.so against aten::convolution(_backward)",
           "rows": [], "steps": []}
    for what, ci, co, h, w, ds in SHAPES:
        for d in ds:
            row = dict(where=what, **operator(dev, args.batch, ci, co, h, w, d, args.warmup, args.iters))
            out["rows"].append(row)
            print(json.dumps(row), flush=True)
    if not args.no_step:
        for out_stride in (16, 8):
            s = step(dev, out_stride, args.batch, args.warmup, max(3, args.iters // 2))
            s["iters"] = max(3, args.iters // 2)
            out["steps"].append(s)
            print(json.dumps(s), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
