#!/usr/bin/env python3
"""G14: Projector(trans=True) fixtures from the REFERENCE Projector / SelfAttention, run on the CPU (build container only).

One tests/golden/G14_projector_trans_<case>.npz per case, training mode: ``config_json``, the inputs ``x{i}``, every
state_dict tensor before the forward as ``w:<key>`` and the key order as ``keys``, the outputs ``out{i}``, stored random
cotangents ``cot{i}``, and the gradients ``gx{i}`` (inputs) and ``g:<name>`` (every parameter) of sum_i <out_i, cot_i>.
The reference is imported at run time; none of its text is here."""
import builtins
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: E402

ref_shim.install()
ref_shim.quiet()
_print = builtins.print
builtins.print = lambda *a, **k: None
from models.Projector import Projector  # noqa: E402  (the reference's)

OUT = os.path.join(os.path.dirname(__file__), "..", "tests", "golden")

CASES = {
    "a": dict(cfg={"c_in": 32, "mlp": [[1, -1, 1], [1, 64, 1]], "use_bn": True, "trans": True, "heads": 2, "d": 32},
              shapes=[(2, 32, 5, 7)]),
    "b": dict(cfg={"c_in": [16, 32], "mlp": [], "trans": True, "heads": 1, "d": 16}, shapes=[(2, 16, 8, 8), (2, 32, 4, 4)]),
    "c": dict(cfg={"c_in": 48, "mlp": [], "trans": True, "heads": 3, "d": 24}, shapes=[(1, 48, 3, 3)]),
}


def main():
    for seed, (name, case) in enumerate(sorted(CASES.items())):
        torch.manual_seed(1400 + seed)
        cfg = json.loads(json.dumps(case["cfg"]))
        model = Projector(cfg).train()
        with torch.no_grad():
            for key, p in model.named_parameters():       # norm weights / biases away from 1 / 0, so that their gradients say something
                if p.dim() == 1:
                    p.add_(0.2 * torch.randn_like(p))
        rec = {"config_json": np.array(json.dumps(case["cfg"]))}
        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        rec["keys"] = np.array(list(state.keys()))
        for k, v in state.items():
            rec["w:" + k] = v.numpy()
        xs = [torch.randn(s).requires_grad_(True) for s in case["shapes"]]
        outs = model(xs if isinstance(cfg["c_in"], list) else xs[0])
        outs = outs if isinstance(outs, (list, tuple)) else [outs]
        cots = [torch.randn(o.shape) for o in outs]
        sum((o * c).sum() for o, c in zip(outs, cots)).backward()
        for i, (x, o, c) in enumerate(zip(xs, outs, cots)):
            rec[f"x{i}"] = x.detach().numpy()
            rec[f"out{i}"] = o.detach().contiguous().numpy()
            rec[f"cot{i}"] = c.numpy()
            rec[f"gx{i}"] = x.grad.numpy()
        for key, p in model.named_parameters():
            rec["g:" + key] = p.grad.numpy()
        path = os.path.join(OUT, f"G14_projector_trans_{name}.npz")
        np.savez_compressed(path, **rec)
        _print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes, keys {list(state.keys())}")


if __name__ == "__main__":
    main()
