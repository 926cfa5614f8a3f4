#!/usr/bin/env python3
"""G16: DeepLabv3 fixtures from the REFERENCE models/DeepLabv3.py, run on the CPU (build container only).

tests/golden/G16_aspp_<case>.npz, training mode: the reference's ASPP at small widths, ``mult = 1`` (dilations 6 / 12 / 18).
``config_json`` (cin, caspp, mult, B, H, W), the input ``x0``, every state_dict tensor before the forward flattened one after the
other into ``w_flat`` with ``w_index_json`` = [[key, shape], ...] in state_dict order, the output ``out0``, a stored random
cotangent ``cot0``, the input gradient ``gx0`` and, packed the same way as ``g_flat`` / ``g_index_json``, the gradient of every
parameter of <out0, cot0>.  Packing and rounding are those of tools/gen_golden_ocr.py: weights, inputs and the cotangent keep 2
mantissa bits, outputs and gradients are stored on a grid of 2^-22 (2^(e - 24) for a tensor that reaches 2^e >= 4).
  a  B 2, 32 -> 16, 13 x 17   dilation 6 partly live, 12 reaches one row / five columns, 18 is centre-only
  b  B 2, 48 -> 32, 20 x 20   all three dilations live
  c  B 2, 16 -> 16,  5 x  5   all three centre-only

tests/golden/G16_deeplabv3_wiring.npz, eval mode: the reference's DeepLabv3 class with this package's resnet50 in place of
torchvision's and a stand-in for torchvision's IntermediateLayerGetter (below), ``out_stride`` 16, ``ms_projector`` over layer1 /
layer3 / layer4, B 2, 3 x 33 x 49.  The state is not stored: it is the closed form ``formula_tensor`` of tests/_aspp_golden.py
applied to the reference's own ordered state_dict keys and shapes (``keys_json``); ``head_json`` is the part outside the backbone.
``logits`` and the three projected maps ``feat0..2`` are stored on the same grid.  The reference is imported at run time; none of
its text is here."""
import builtins
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402
from gen_golden_ocr import coarse, pack, stored  # noqa: E402  (installs the shim; the packing and rounding scheme)

ref_shim.install()
ref_shim.quiet()
_print = lambda s: sys.stdout.write(s + "\n")      # (gen_golden_ocr has silenced print already)
builtins.print = lambda *a, **k: None
import models  # noqa: E402,F401  (the reference's package; its __init__ rebinds the name DeepLabv3 to the class)
refmod = sys.modules["models.DeepLabv3"]

sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import mscs_amd  # noqa: E402,F401
from mscs_amd.models import resnet50  # noqa: E402
import _aspp_golden as ag  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden")

CASES = {
    "a": dict(cin=32, caspp=16, mult=1, B=2, H=13, W=17),
    "b": dict(cin=48, caspp=32, mult=1, B=2, H=20, W=20),
    "c": dict(cin=16, caspp=16, mult=1, B=2, H=5, W=5),
}


class LayerGetter(torch.nn.ModuleDict):
    """What the reference asks of torchvision's IntermediateLayerGetter: the model's children under their names, run in order, the
    outputs of the layers named in ``return_layers`` collected under the given keys."""

    def __init__(self, model, return_layers):
        super().__init__(OrderedDict(model.named_children()))
        self.return_layers = dict(return_layers)

    def forward(self, x):
        out = OrderedDict()
        for name, m in self.items():
            x = m(x)
            if name in self.return_layers:
                out[self.return_layers[name]] = x
        return out


def aspp_fixtures():
    for seed, (name, c) in enumerate(sorted(CASES.items())):
        torch.manual_seed(1600 + seed)
        model = refmod.ASPP(c_in=c["cin"], c_aspp=c["caspp"], mult=c["mult"]).train()
        with torch.no_grad():
            for key, p in model.named_parameters():
                if p.dim() == 1:
                    p.add_(0.2 * torch.randn_like(p))
                p.copy_(coarse(p))
        rec = {"config_json": np.array(json.dumps(c))}
        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        rec["w_flat"], rec["w_index_json"] = pack(state)
        x = coarse(torch.randn(c["B"], c["cin"], c["H"], c["W"])).requires_grad_(True)
        out = model(x)
        cot = coarse(torch.randn(out.shape)) / 1024
        (out * cot).sum().backward()
        rec.update(x0=x.detach().numpy(), out0=stored(out), cot0=cot.numpy(), gx0=stored(x.grad))
        rec["g_flat"], rec["g_index_json"] = pack({key: p.grad for key, p in model.named_parameters()}, stored)
        path = os.path.join(OUT, f"G16_aspp_{name}.npz")
        np.savez_compressed(path, **rec)
        _print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes, {len(state)} state tensors, "
               f"eps {model.aspp1_bn.eps} momentum {model.aspp1_bn.momentum}")


def wiring_fixture():
    c = dict(dataset="CITYSCAPES", experiment=1, backbone="resnet50", out_stride=16, d=16, B=2, H=33, W=49)
    graph = {"dataset": c["dataset"], "backbone": c["backbone"], "pretrained": False, "out_stride": c["out_stride"],
             "ms_projector": {"mlp": [[1, -1, 1]], "feats": ["layer1", "layer3", "layer4"], "d": c["d"], "use_bn": True,
                              "before_context": True}}
    c["graph"] = json.loads(json.dumps(graph))
    refmod.resnet50 = lambda pretrained=False, **kw: resnet50(pretrained=pretrained, **kw)
    refmod.IntermediateLayerGetter = LayerGetter
    model = refmod.DeepLabv3(graph, c["experiment"])
    keys = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    model.load_state_dict({k: ag.formula_tensor(k, tuple(s)) for k, s in keys}, strict=True)
    model.eval()
    with torch.no_grad():
        logits, feats = model(ag.wiring_input(c))
    assert len(feats) == 3
    rec = {"config_json": np.array(json.dumps(c)), "keys_json": np.array(json.dumps(keys, separators=(",", ":"))),
           "head_json": np.array(json.dumps([e for e in keys if not e[0].startswith("backbone.")], separators=(",", ":"))),
           "logits": stored(logits)}
    for i, f in enumerate(feats):
        rec[f"feat{i}"] = stored(f)
    np.savez_compressed(ag.WIRING, **rec)
    _print(f"{os.path.basename(ag.WIRING)}: {os.path.getsize(ag.WIRING)} bytes, {len(keys)} keys, max|logits| "
           f"{float(logits.abs().max()):.3g}, max|feat| {[round(float(f.abs().max()), 3) for f in feats]}")


if __name__ == "__main__":
    torch.set_num_threads(4)        # the CPU kernels' summation order depends on it; the tests run the comparison at 4 as well
    aspp_fixtures()
    wiring_fixture()
