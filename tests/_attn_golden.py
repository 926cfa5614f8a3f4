"""Shared by tests/test_attn_host.py and tests/test_attn_hip.py: the G14 fixtures (tools/gen_golden_attn.py: the reference's
Projector(trans=True) on the CPU, training mode) and one forward + backward of this package's Projector on them."""
import json
import os

import numpy as np
import torch

from conftest import GOLDEN

CASES = ("a", "b", "c")


def load(case):
    z = np.load(os.path.join(GOLDEN, f"G14_projector_trans_{case}.npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["config"] = json.loads(str(d["config_json"]))
    d["n"] = len([k for k in d if k.startswith("out")])
    return d


def build(g, dev="cpu"):
    """This package's Projector with the fixture's weights, in training mode."""
    from mscs_amd.models.Projector import Projector
    m = Projector(json.loads(json.dumps(g["config"])))
    m.load_state_dict({k: torch.from_numpy(g["w:" + k]) for k in g["keys"].tolist()}, strict=True)
    return m.to(dev).train()


def run(m, g, dev="cpu", finish=lambda o: o):
    """(outputs, input gradients, {name: parameter gradient}) of sum_i <finish(out_i), cot_i>, everything on the CPU as float64."""
    xs = [torch.from_numpy(g[f"x{i}"]).to(dev).requires_grad_(True) for i in range(g["n"])]
    m.zero_grad(set_to_none=True)
    outs = m(xs if m.is_ms else xs[0])
    outs = [finish(o) for o in (outs if isinstance(outs, (list, tuple)) else [outs])]
    sum((o * torch.from_numpy(g[f"cot{i}"]).to(dev)).sum() for i, o in enumerate(outs)).backward()
    f = lambda t: t.detach().double().cpu()
    return [f(o) for o in outs], [f(x.grad) for x in xs], {k: f(p.grad) for k, p in m.named_parameters()}


def distances(got, g):
    """{name: max|got - golden| / max|golden|} over the outputs, the input gradients and every parameter gradient"""
    outs, gxs, gps = got
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    d = {}
    for i in range(g["n"]):
        d[f"out{i}"] = rel(outs[i], torch.from_numpy(g[f"out{i}"]).double())
        d[f"gx{i}"] = rel(gxs[i], torch.from_numpy(g[f"gx{i}"]).double())
    for k, v in gps.items():
        d["g:" + k] = rel(v, torch.from_numpy(g["g:" + k]).double())
    return d
