"""Forward + backward time of the global self-attention core: the HIP kernels (libdcl_attn.so) against the eager composition
that materialises the N x N scores, in one process on one GPU, HIP-event medians.

    python tools/attn_time.py [--warmup 5] [--iters 20] [--out profiles/attn_time.json]

Shapes: B = 2, C = 256, heads in {1, 4}, N in {2048, 8192}; the HIP path alone at N = 32768 (the benchmark's 1/4-resolution map,
where the eager path would need 4 GiB per image and head).  Records both times, their ratio, and the share of the split-f16
matrix-core roofline (2.5 PFLOP/s / 3) the HIP path reaches on the algorithmic work, 14 B heads N^2 D FLOP: two products
forward, five backward (the scores recomputed a second time in the backward are not counted).  Not a test: nothing is asserted
about the ratio."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mscs_amd  # noqa: E402,F401
from mscs_amd import _lib_attn as la  # noqa: E402
from mscs_amd.models.ops_attn import _Attention, attention_eager  # noqa: E402

ROOF = 2.5e15 / 3


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_time.json"))
    a = ap.parse_args()
    assert a.warmup >= 3 and a.iters >= 10, "at least 3 warm-up and 10 timed iterations"
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    la.lib()
    rows = []
    B, C = 2, 256
    for heads in (1, 4):
        for N, with_eager in ((2048, True), (8192, True), (32768, False)):
            D = C // heads
            g = torch.Generator(device=dev).manual_seed(0)
            qkv = torch.randn(B, N, 3 * C, device=dev, generator=g).requires_grad_(True)
            dout = torch.randn(B, N, C, device=dev, generator=g)
            scale = D ** -0.5

            def step(fn):
                qkv.grad = None
                fn(qkv, heads, scale).backward(dout)
            row = {"B": B, "N": N, "heads": heads, "D": D, "hip": timed(lambda: step(_Attention.apply), a.warmup, a.iters)}
            flop = 14.0 * B * heads * N * N * D
            row["hip"]["algorithmic_tflops"] = flop / (row["hip"]["median_ms"] * 1e-3) / 1e12
            row["hip"]["frac_of_f16x3_roofline"] = flop / (row["hip"]["median_ms"] * 1e-3) / ROOF
            if with_eager:
                row["eager"] = timed(lambda: step(attention_eager), a.warmup, a.iters)
                row["eager_over_hip"] = row["eager"]["median_ms"] / row["hip"]["median_ms"]
            rows.append(row)
            print(json.dumps(row))
    res = {"device": torch.cuda.get_device_name(0), "what": "attention core forward + backward, HIP-event medians, ms",
           "warmup": a.warmup, "iters": a.iters, "roofline_flops": ROOF, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
