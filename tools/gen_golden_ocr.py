#!/usr/bin/env python3
"""G15: OCR fixtures from the REFERENCE models/OCR.py, run on the CPU (build container only).

tests/golden/G15_ocr_<case>.npz, training mode: the reference's SpatialGatherModule followed by its SpatialOCR_Module at small
widths.  ``config_json`` (in / key / out channels, K, B, H, W), the inputs ``x0`` (features) and ``x1`` (logits), every state_dict
tensor of the SpatialOCR_Module before the forward, flattened one after the other into ``w_flat`` with ``w_index_json`` =
[[key, shape], ...] in state_dict order, the outputs ``out0`` (the module's result) and ``ctx`` (the gather's), a stored random
cotangent ``cot0``, and the gradients ``gx0``, ``gx1`` and, packed the same way as ``g_flat`` / ``g_index_json``, of every
parameter, of <out0, cot0>.  (One array per tensor costs about 350 bytes of container each.)  Norm weights and biases are perturbed away from 1 and 0.  Weights, inputs and the cotangent are
rounded to 2 mantissa bits before the forward (exactly representable, a third of the bytes once compressed); outputs and
gradients are stored rounded to the nearest multiple of 2^-22 (1.2e-7 at most from the computed value, an eighth of the atol the
tests compare with; 2^(e - 24) for a tensor that reaches 2^e >= 4, where the tests' rtol term is 4e-5 or more): exact floats whose
low bits are zero.  With
both, every file stays under 100 KB; as computed, case b's gradients and outputs alone are 93 KB of incompressible fp32.

tests/golden/G15_ocrnet_hrnet48_keys.json: the ordered state_dict keys and shapes of the reference's OCRNet(hrnet48) built from
its shipped ADE20K config (``pretrained`` off), names and shapes only; the config itself is copied to
tests/golden/reference_configs/.  The reference is imported at run time; none of its text is here."""
import builtins
import json
import os
import shutil
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: E402

ref_shim.install()
ref_shim.quiet()
_print = builtins.print
builtins.print = lambda *a, **k: None
from models.OCR import OCRNet, SpatialGatherModule, SpatialOCR_Module  # noqa: E402  (the reference's)

OUT = os.path.join(os.path.dirname(__file__), "..", "tests", "golden")
SHIPPED = os.path.join(ref_shim.REFERENCE_ROOT, "configs", "ADE20K", "hrnetocr_contrastive_ADE20K.json")

CASES = {
    "a": dict(cin=32, key=16, out=32, K=5, B=2, H=5, W=7),
    "b": dict(cin=48, key=32, out=64, K=19, B=1, H=8, W=8),
    "c": dict(cin=16, key=16, out=16, K=1, B=2, H=3, W=3),
}


def coarse(t):
    """t with the low 21 bits of every float cleared"""
    return (t.detach().contiguous().view(torch.int32) & ~0x1FFFFF).view(torch.float32)


def stored(t):
    """t rounded to the nearest multiple of 2^-22 (2^(e - 24) for a tensor whose largest magnitude reaches 2^e >= 4: half an ulp of
    that maximum), as a float32 numpy array"""
    import math
    t = t.detach().contiguous().to(torch.float32)
    e = max(2, math.floor(math.log2(max(float(t.abs().max()), 1.0))) + 1)
    return (torch.round(t.double() * 2.0 ** (24 - e)) / 2.0 ** (24 - e)).to(torch.float32).numpy()


def pack(tensors, f=lambda v: v.detach().to(torch.float32).numpy()):
    flat = np.concatenate([f(v).reshape(-1) for v in tensors.values()])
    return flat, np.array(json.dumps([[k, list(v.shape)] for k, v in tensors.items()]))


def fixtures():
    for seed, (name, c) in enumerate(sorted(CASES.items())):
        torch.manual_seed(1500 + seed)
        gather = SpatialGatherModule(c["K"]).train()
        model = SpatialOCR_Module(in_channels=c["cin"], key_channels=c["key"], out_channels=c["out"], scale=1, dropout=0.0).train()
        with torch.no_grad():
            for key, p in model.named_parameters():
                if p.dim() == 1:
                    p.add_(0.2 * torch.randn_like(p))
                p.copy_(coarse(p))
        rec = {"config_json": np.array(json.dumps(c))}
        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        rec["w_flat"], rec["w_index_json"] = pack(state)
        feats = coarse(torch.randn(c["B"], c["cin"], c["H"], c["W"])).requires_grad_(True)
        logits = coarse(3.0 * torch.randn(c["B"], c["K"], c["H"], c["W"])).requires_grad_(True)
        ctx = gather(feats, logits)
        out = model(feats, ctx)
        cot = coarse(torch.randn(out.shape)) / 1024     # small gradients: fewer significant bits on the storage grid (1e-6 is still 7e-6 of their maximum)
        (out * cot).sum().backward()
        rec.update(x0=feats.detach().numpy(), x1=logits.detach().numpy(), out0=stored(out), ctx=stored(ctx), cot0=cot.numpy(),
                   gx0=stored(feats.grad), gx1=stored(logits.grad))
        rec["g_flat"], rec["g_index_json"] = pack({key: p.grad for key, p in model.named_parameters()}, stored)
        path = os.path.join(OUT, f"G15_ocr_{name}.npz")
        np.savez_compressed(path, **rec)
        _print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes, {len(state)} state tensors")


def keys():
    cfg = json.load(open(SHIPPED))
    graph = cfg["graph"]
    graph["pretrained"] = False
    graph["dataset"] = cfg["data"]["dataset"]
    model = OCRNet(config=graph, experiment=cfg["data"]["experiment"])
    entries = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    path = os.path.join(OUT, "G15_ocrnet_hrnet48_keys.json")
    with open(path, "w") as f:
        json.dump(entries, f, separators=(",", ":"))
        f.write("\n")
    _print(f"{os.path.basename(path)}: {len(entries)} entries, {os.path.getsize(path)} bytes")
    shutil.copyfile(SHIPPED, os.path.join(OUT, "reference_configs", os.path.basename(SHIPPED)))


if __name__ == "__main__":
    torch.set_num_threads(4)        # the CPU kernels' summation order depends on it; tests/test_ocr_host.py runs the comparison at 4 as well
    fixtures()
    keys()
