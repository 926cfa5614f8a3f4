"""Shared by tests/test_ocr_host.py and tests/test_ocr_hip.py: the G15 fixtures (tools/gen_golden_ocr.py: the reference's
SpatialGatherModule + SpatialOCR_Module on the CPU, training mode) and one forward + backward of this package's modules on them."""
import json
import os

import numpy as np
import torch

from conftest import GOLDEN

CASES = ("a", "b", "c")


def _unpack(flat, index):
    out, at = {}, 0
    for key, shape in index:
        n = int(np.prod(shape)) if shape else 1
        out[key] = flat[at:at + n].reshape(shape)
        at += n
    assert at == flat.size
    return out


def load(case):
    z = np.load(os.path.join(GOLDEN, f"G15_ocr_{case}.npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["config"] = json.loads(str(d["config_json"]))
    d["w"] = _unpack(d["w_flat"], json.loads(str(d["w_index_json"])))
    d["g"] = _unpack(d["g_flat"], json.loads(str(d["g_index_json"])))
    return d


def build(g, dev="cpu", dtype=torch.float32, train=True):
    """(gather, module): this package's SpatialGatherModule and SpatialOCR_Module with the fixture's weights, training mode."""
    from mscs_amd.models.OCR import SpatialGatherModule, SpatialOCR_Module
    c = g["config"]
    m = SpatialOCR_Module(in_channels=c["cin"], key_channels=c["key"], out_channels=c["out"], scale=1, dropout=0.0)
    own = m.state_dict()
    assert list(own) == list(g["w"]), "state_dict keys / order differ from the reference"
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)).to(own[k].dtype) for k, v in g["w"].items()}, strict=True)
    return SpatialGatherModule(c["K"]).to(dev).train(train), m.to(dev).to(dtype).train(train)


def run(mods, g, dev="cpu", dtype=torch.float32):
    """(out, ctx, [gx0, gx1], {name: parameter gradient}) of <out, cot0>, on the CPU as float64."""
    gather, m = mods
    x0 = torch.from_numpy(g["x0"]).to(dev).to(dtype).requires_grad_(True)
    x1 = torch.from_numpy(g["x1"]).to(dev).to(dtype).requires_grad_(True)
    m.zero_grad(set_to_none=True)
    ctx = gather(x0, x1)
    out = m(x0, ctx)
    (out * torch.from_numpy(g["cot0"]).to(dev).to(dtype)).sum().backward()
    f = lambda t: t.detach().double().cpu()
    return f(out), f(ctx), [f(x0.grad), f(x1.grad)], {k: f(p.grad) for k, p in m.named_parameters()}


def golden(g):
    """the fixture's record in the shape of run()'s result"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    return t(g["out0"]), t(g["ctx"]), [t(g["gx0"]), t(g["gx1"])], {k: t(v) for k, v in g["g"].items()}


def distances(got, want):
    """{name: max|got - want| / max|want|} over the output, the class representations, the input gradients and every
    parameter gradient; both in the shape of run()'s result"""
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    d = {"out0": rel(got[0], want[0]), "ctx": rel(got[1], want[1]), "gx0": rel(got[2][0], want[2][0]), "gx1": rel(got[2][1], want[2][1])}
    for k, v in got[3].items():
        d["g:" + k] = rel(v, want[3][k])
    return d
