"""Forward + backward time and peak memory of the OCR context core: the HIP kernels (libdcl_ocr.so) against the eager
composition, in one process on one GPU, HIP-event medians.

    python tools/ocr_time.py [--warmup 3] [--iters 10] [--configs 1,2,3] [--out profiles/ocr_time.json]

Config 1: B = 16, N = 128 x 128, C = 512, Ck = 256, K = 150 (the shipped ADE20K config: batch 16 of 512 x 512).
Config 2: B = 12, N = 128 x 256, C = 512, Ck = 256, K = 19 (Cityscapes crops).
Config 3: OCRNet(hrnet48) as a whole, forward + backward at batch 16 of 512 x 512, the switch on and off.
For configs 1 and 2 the gather and the object attention are timed separately; peak memory is what the step allocates beyond its
inputs.  Not a test: nothing is asserted about the ratios."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mscs_amd  # noqa: E402,F401
from mscs_amd import _lib_ocr as la  # noqa: E402
from mscs_amd.debug import cfg as dbg  # noqa: E402
from mscs_amd.models import ops_ocr  # noqa: E402


def timed(fn, warmup, iters, dev):
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


def cores(dev, B, h, w, C, Ck, K, warmup, iters):
    g = torch.Generator(device=dev).manual_seed(0)
    N = h * w
    x = torch.randn(B, C, h, w, device=dev, generator=g).requires_grad_(True)
    logits = torch.randn(B, K, h, w, device=dev, generator=g).requires_grad_(True)
    dctx = torch.randn(B, C, K, 1, device=dev, generator=g)
    q = torch.randn(B, Ck, N, device=dev, generator=g).requires_grad_(True)
    key = torch.randn(B, Ck, K, device=dev, generator=g).requires_grad_(True)
    val = torch.randn(B, Ck, K, device=dev, generator=g).requires_grad_(True)
    dout = torch.randn(B, Ck, N, device=dev, generator=g)

    def gather_step():
        x.grad = logits.grad = None
        ops_ocr.gather(x, logits, 1).backward(dctx)

    def attn_step():
        q.grad = key.grad = val.grad = None
        ops_ocr.object_attention(q, key, val).backward(dout)
    row = {"B": B, "H": h, "W": w, "N": N, "C": C, "Ck": Ck, "K": K,
           "x_mib": x.numel() * 4 / 2 ** 20, "scores_mib": B * N * K * 4 / 2 ** 20}
    for name, step in (("gather", gather_step), ("attention", attn_step)):
        row[name] = {}
        for hip in (True, False):
            dbg.ocr_hip = hip
            row[name]["hip" if hip else "eager"] = timed(step, warmup, iters, dev)
        dbg.ocr_hip = True
        row[name]["eager_over_hip"] = row[name]["eager"]["median_ms"] / row[name]["hip"]["median_ms"]
    return row


def whole_model(dev, warmup, iters):
    from mscs_amd.models import OCRNet
    from mscs_amd.utils import set_verbosity
    set_verbosity(40)
    with open(os.path.join(ROOT, "tests", "golden", "reference_configs", "hrnetocr_contrastive_ADE20K.json")) as f:
        graph = json.load(f)["graph"]
    graph.update(pretrained=False, dataset="ADE20K")
    torch.manual_seed(0)
    model = OCRNet(config=graph, experiment=1).to(dev).train()
    img = torch.randn(16, 3, 512, 512, device=dev)
    row = {"model": "OCRNet(hrnet48)", "B": 16, "H": 512, "W": 512}

    def step():
        model.zero_grad(set_to_none=True)
        interm, out, feats = model(img)
        (out.mean() + 0.4 * interm.mean() + sum(f.mean() for f in feats)).backward()
    for hip in (True, False):
        dbg.ocr_hip = hip
        row["hip" if hip else "eager"] = timed(step, warmup, iters, dev)
    dbg.ocr_hip = True
    row["eager_over_hip"] = row["eager"]["median_ms"] / row["hip"]["median_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--configs", default="1,2,3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ocr_time.json"))
    a = ap.parse_args()
    assert a.warmup >= 3 and a.iters >= 10, "at least 3 warm-up and 10 timed iterations"
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    la.lib()
    rows = []
    for c in (int(v) for v in a.configs.split(",")):
        if c == 1:
            row = cores(dev, 16, 128, 128, 512, 256, 150, a.warmup, a.iters)
        elif c == 2:
            row = cores(dev, 12, 128, 256, 512, 256, 19, a.warmup, a.iters)
        else:
            row = whole_model(dev, a.warmup, a.iters)
        row["config"] = c
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "what": "OCR context core forward + backward, HIP-event medians (ms), peak MiB "
           "beyond the inputs", "warmup": a.warmup, "iters": a.iters, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
