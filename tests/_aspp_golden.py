"""Shared by tests/test_dconv_host.py and tests/test_dconv_hip.py (and read by tools/gen_golden_aspp.py): the G16 fixtures (the
reference's ASPP on the CPU, training mode; the reference's DeepLabv3 wired to this package's resnet50, eval mode), one forward +
backward of this package's ASPP on them, and the closed-form state the wiring fixture is evaluated at."""
import json
import os
import zlib

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("a", "b", "c")
WIRING = os.path.join(GOLDEN, "G16_deeplabv3_wiring.npz")


def _unpack(flat, index):
    out, at = {}, 0
    for key, shape in index:
        n = int(np.prod(shape)) if shape else 1
        out[key] = flat[at:at + n].reshape(shape)
        at += n
    assert at == flat.size
    return out


def load(case):
    z = np.load(os.path.join(GOLDEN, f"G16_aspp_{case}.npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["config"] = json.loads(str(d["config_json"]))
    d["w"] = _unpack(d["w_flat"], json.loads(str(d["w_index_json"])))
    d["g"] = _unpack(d["g_flat"], json.loads(str(d["g_index_json"])))
    return d


def build(g, dev="cpu", dtype=torch.float32, train=True, norm=torch.nn.BatchNorm2d):
    """This package's ASPP with the fixture's state (loaded strictly), kernels selected as DeepLabv3 selects them."""
    from mscs_amd.models.DeepLabv3 import ASPP
    from mscs_amd.models.ops import use_direct_conv1x1
    from mscs_amd.models.ops_dconv import use_dilated_conv3x3
    c = g["config"]
    m = ASPP(c_in=c["cin"], c_aspp=c["caspp"], norm=norm, mult=c["mult"], align_corners=True)
    own = m.state_dict()
    assert list(own) == list(g["w"]), "state_dict keys / order differ from the reference"
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)).to(own[k].dtype) for k, v in g["w"].items()}, strict=True)
    use_dilated_conv3x3(m)
    use_direct_conv1x1(m)
    return m.to(dev).to(dtype).train(train)


def run(m, g, dev="cpu", dtype=torch.float32):
    """(out, gx0, {name: parameter gradient}) of <out, cot0>, on the CPU as float64."""
    x0 = torch.from_numpy(g["x0"]).to(dev).to(dtype).requires_grad_(True)
    m.zero_grad(set_to_none=True)
    out = m(x0)
    (out * torch.from_numpy(g["cot0"]).to(dev).to(dtype)).sum().backward()
    f = lambda t: t.detach().double().cpu()
    return f(out), f(x0.grad), {k: f(p.grad) for k, p in m.named_parameters()}


def golden(g):
    """the fixture's record in the shape of run()'s result"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    return t(g["out0"]), t(g["gx0"]), {k: t(v) for k, v in g["g"].items()}


def distances(got, want):
    """{name: max|got - want| / max|want|} over the output, the input gradient and every parameter gradient"""
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    d = {"out0": rel(got[0], want[0]), "gx0": rel(got[1], want[1])}
    for k, v in got[2].items():
        d["g:" + k] = rel(v, want[2][k])
    return d


def formula_tensor(key, shape):
    """The wiring fixture's value of state_dict entry ``key``: ten hashed bits per element, centred, times a power of two -- exact
    in float32 and the same on every machine, so 25 M backbone weights need not be stored."""
    if key.endswith("num_batches_tracked"):
        return torch.zeros(shape, dtype=torch.int64)
    n = int(np.prod(shape)) if shape else 1
    h = (np.arange(n, dtype=np.uint64) + np.uint64(zlib.crc32(key.encode()))) * np.uint64(2654435761) % np.uint64(1 << 32)
    h = (h ^ (h >> np.uint64(15))) * np.uint64(2246822519) % np.uint64(1 << 32)
    u = ((h >> np.uint64(22)).astype(np.float64) + 0.5) / 1024.0 - 0.5          # uniform on a grid in (-0.5, 0.5)
    if len(shape) == 4:
        fan_in, k = int(np.prod(shape[1:])), 0
        while fan_in > 24 * 4 ** k:              # amplitude 2^-k: variance 4^-k / 12 <= 2 / fan_in
            k += 1
        v = u * 2.0 ** -k
    elif key.endswith(("running_var", "weight")):
        v = 1.0 + 0.25 * u
    else:
        v = 0.25 * u
    return torch.from_numpy(v.astype(np.float32).reshape(shape))


def wiring():
    z = np.load(WIRING, allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["config"] = json.loads(str(d["config_json"]))
    d["keys"] = json.loads(str(d["keys_json"]))
    d["head"] = json.loads(str(d["head_json"]))
    return d


def wiring_input(c):
    return formula_tensor("input", (c["B"], 3, c["H"], c["W"])) * 4
