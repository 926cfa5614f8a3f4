#!/usr/bin/env python3
"""Per-launch A/B of the fused convolution backward (libdcl_convbwd.so) against the separate launches, at the C ABI.

    python tools/probes/conv_bwd_ab.py [--out profiles/convbwd_per_launch.csv] [--rounds 30] [--reps 10]

For the two BasicBlock shapes the launch is for (12 x 192 x 32 x 64 and 12 x 384 x 16 x 32, plain and with the PRE map), three variants
on the same buffers and stream:
    separate    dcl_conv3x3_f16x3 (data gradient, addend) + dcl_wgrad3x3[_pre]_f16x3 (weight gradient + slab reduction)
    fused256    dcb_conv3x3_bwd_f16x3 with wg_target = 256 (the separate entry's weight-gradient plan behind the tiles)
    fused       dcb_conv3x3_bwd_f16x3 with the automatic plan (weight gradient planned for the CUs the tiles leave free)
The variants ALTERNATE inside every round (separate, fused256, fused, separate, ...), each timed with a HIP event pair around
``reps`` back-to-back calls; the CSV has median and minimum per call over the rounds.  Nothing else runs on the device: these are
stand-alone times, the step's A/B (bench.py with DCL_FUSE_CONV_BWD=0/1) decides."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import mscs_amd  # noqa: E402,F401
from mscs_amd import _lib, _lib_convbwd as cb  # noqa: E402
from mscs_amd.models import ops_conv  # noqa: E402

SHAPES = [(12, 192, 32, 64), (12, 384, 16, 32)]


def p(t):
    return None if t is None else t.data_ptr()


def variants(dev, n, c, h, w, pre):
    L, B, st = _lib.lib(), cb.lib(), _lib.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(c + int(pre))
    x = torch.randn(n, c, h, w, device=dev, generator=g) * 2.5
    if not pre:
        x.relu_()
    wt = torch.randn(c, c, 3, 3, device=dev, generator=g) / (3.0 * c ** 0.5)
    gy = torch.randn(n, c, h, w, device=dev, generator=g) * 3e-5
    addend = torch.randn(n, c, h, w, device=dev, generator=g) * 1e-4
    sc = torch.rand(c, device=dev, generator=g) + 0.5 if pre else None
    sh = torch.randn(c, device=dev, generator=g) * 0.5 if pre else None
    op = torch.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)) if pre else x
    xa, ga, wa = op.abs().max().reshape(1), gy.abs().max().reshape(1), wt.abs().max().reshape(1)
    wpt = ops_conv.conv3x3_pack(wt, wa, transposed=True)
    gx, dw = torch.empty_like(x), torch.empty(c, c, 3, 3, device=dev)
    slabs = max(L.dcl_wgrad3x3_splits(n, c, c, h, w, 1), cb.wgrad_splits(n, c, c, h, w, 0, 0, 256), cb.wgrad_splits(n, c, c, h, w))
    part = torch.empty(slabs * 9 * c * c, device=dev)
    keep = (x, wt, gy, addend, sc, sh, xa, ga, wa, wpt, gx, dw, part)

    def separate():
        _lib.check(L.dcl_conv3x3_f16x3(p(gy), n, c, h, w, p(wpt), c, p(ga), 1, p(wa), p(addend), None, p(gx), 1, 1, h, w, 0, 0, st), "dgrad")
        if pre:
            _lib.check(L.dcl_wgrad3x3_pre_f16x3(p(x), p(gy), n, c, c, h, w, p(xa), 1, p(ga), 1, p(sc), p(sh), 1, p(part), p(dw), st), "wgrad")
        else:
            _lib.check(L.dcl_wgrad3x3_f16x3(p(x), p(gy), n, c, c, h, w, p(xa), 1, p(ga), 1, 1, p(part), p(dw), st), "wgrad")

    def fused(target):
        def run():
            cb.check(B.dcb_conv3x3_bwd_f16x3(p(gy), p(wpt), p(x), n, c, c, h, w, p(ga), 1, p(wa), p(xa), 1, p(addend), p(sc), p(sh),
                                             0, 0, target, p(gx), p(part), p(dw), st), "fused")
        return run
    return [("separate", separate), ("fused256", fused(256)), ("fused", fused(0))], keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convbwd_per_launch.csv"))
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = ["shape,pre,variant,plan,median_us,min_us,rounds,reps"]
    for n, c, h, w in SHAPES:
        for pre in (False, True):
            vs, keep = variants(dev, n, c, h, w, pre)
            plan = cb.plan(n, c, c, h, w)
            for _, fn in vs:                # warm-up: code objects loaded, caches in their steady state
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name, _ in vs}
            for _ in range(a.rounds):
                for name, fn in vs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.reps):
                        fn()
                    e1.record()
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1) * 1e3 / a.reps)
            for name, _ in vs:
                desc = {"separate": "dgrad 96 wgs; wgrad own plan", "fused256": f"tiles {plan['nd8']} + wgrad for 256",
                        "fused": f"tiles {plan['nd8']} + wgrad {plan['wgrad_grid']} wgs / {plan['slabs']} slabs"}[name]
                rows.append(f"{n}x{c}x{h}x{w},{int(pre)},{name},{desc},{statistics.median(times[name]):.1f},{min(times[name]):.1f},"
                            f"{a.rounds},{a.reps}")
                print(rows[-1], flush=True)
            del keep
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
