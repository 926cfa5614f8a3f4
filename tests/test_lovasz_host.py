"""Host half of the Lovasz-Softmax library: it is built next to the main one, exports and binds exactly what its header declares,
sizes its workspace by the documented formula, and leaves CPU tensors on the PyTorch path."""
import ctypes
import json
import os
import re

import numpy as np
import torch

from conftest import GOLDEN, ROOT

import mscs_amd  # noqa: F401
from mscs_amd import _lib


def _header():
    return open(os.path.join(ROOT, "include", "dcl_lovasz.h")).read()


def test_second_library_is_built_by_the_same_target():
    from mscs_amd import _lib_lovasz as lv
    _lib.build()
    assert os.path.exists(lv.LIB_PATH) and os.path.basename(lv.LIB_PATH) == "libdcl_lovasz.so"
    assert os.path.dirname(lv.LIB_PATH) == os.path.dirname(_lib.LIB_PATH)


def test_header_exports_and_bindings_agree():
    from mscs_amd import _lib_lovasz as lv
    _lib.build()
    hdr = _header()
    names = sorted(set(re.findall(r"\b(dlv_[a-z0-9_]+)\s*\(", hdr)))
    assert len(names) >= 5
    assert not re.findall(r"\bdcl_[a-z0-9_]+\s*\(", hdr), "the main library's prefix in the second library's header"
    raw = ctypes.CDLL(lv.LIB_PATH)
    for name in names:
        assert hasattr(raw, name), f"{name} declared in include/dcl_lovasz.h but not exported"
    assert set(lv.SIGNATURES) | {"dlv_last_error"} == set(names)          # dlv_last_error: a char * result, bound separately
    assert not any(n.startswith("dlv_") for n in _lib.SIGNATURES)
    L = lv.lib()
    assert L.dlv_version() >= 1
    for name, sig in lv.SIGNATURES.items():          # the arity of every binding is the declaration's
        decl = re.search(rf"\b{name}\s*\(([^;]*)\);", hdr).group(1).strip()
        assert len(sig) == (0 if decl == "void" else decl.count(",") + 1), name


def test_missing_library_error_names_the_build(monkeypatch):
    from mscs_amd import _lib_lovasz as lv
    monkeypatch.setattr(lv, "_lib", None)
    monkeypatch.setattr(lv, "LIB_PATH", os.path.join(ROOT, "no_such_dir", "libdcl_lovasz.so"))
    try:
        lv.lib()
    except RuntimeError as e:
        assert "not found" in str(e) and "build" in str(e)
    else:
        raise AssertionError("a missing library must raise")


def _formula(n, c, hw, per_image, tile=4096):
    r = lambda x: (x + 255) // 256 * 256
    t = n * c * hw
    s, l = (n * c, hw) if per_image else (c, n * hw)
    tps = (l + tile - 1) // tile
    return 4 * r(4 * t) + r(4 * 256 * s * tps) + r(4 * 256 * s) + r(4 * s * tps) + r(8 * s * tps) + 3 * r(8 * s)


def test_workspace_bytes_formula_and_monotone():
    from mscs_amd import _lib_lovasz as lv
    assert lv.TILE == int(re.search(r"#define DLV_TILE (\d+)", _header()).group(1))
    for per_image in (False, True):
        # the benchmark shape (12 x 19 x 512 x 1024), ADE20K's, and small / odd ones
        for n, c, hw in [(12, 19, 512 * 1024), (16, 150, 512 * 512), (2, 5, 37 * 53), (1, 3, 1), (1, 256, 4097)]:
            got = lv.workspace_bytes(n, c, hw, per_image)
            assert got == _formula(n, c, hw, per_image), (n, c, hw, per_image, got)
            assert got >= 16 * n * c * hw
            assert lv.workspace_bytes(n + 1, c, hw, per_image) >= got
            if c < 256:
                assert lv.workspace_bytes(n, c + 1, hw, per_image) >= got
            assert lv.workspace_bytes(n, c, hw + 1, per_image) >= got
        bench = lv.workspace_bytes(12, 19, 512 * 1024, per_image)
        assert 1.9e9 < bench < 2.0e9                                  # 2 x 8 B x 119.5 M elements + 1.6 % of bookkeeping
    # what the kernels do not index
    assert lv.workspace_bytes(1, 257, 16, False) == -1 and lv.workspace_bytes(0, 19, 16, False) == -1
    assert lv.workspace_bytes(64, 256, 512 * 512, False) == -1        # N*C*HW >= 2^31


def test_cpu_tensors_take_the_pytorch_path_with_unchanged_values(monkeypatch):
    from mscs_amd import _lib_lovasz as lv
    from mscs_amd.debug import cfg as dbg
    from mscs_amd.losses import LovaszSoftmax
    assert dbg.lovasz_hip is True or os.environ.get("DCL_LOVASZ_HIP") == "0"
    monkeypatch.setattr(lv, "lib", lambda: (_ for _ in ()).throw(AssertionError("the HIP library was asked for a CPU tensor")))
    z = np.load(os.path.join(GOLDEN, "G10_lovasz.npz"))
    for name in ("default", "per_image", "all"):
        m = LovaszSoftmax(json.loads(str(z[name + "_cfg"])))
        x = torch.from_numpy(z["logits"]).requires_grad_(True)
        loss = m(x, torch.from_numpy(z["label"].astype(np.int64)))
        loss.backward()
        np.testing.assert_allclose(loss.item(), z[name + "_loss"], rtol=1e-5)
        np.testing.assert_allclose(x.grad.numpy(), z[name + "_grad"], atol=1e-6 * np.abs(z[name + "_grad"]).max() + 1e-9)
    # without a term the result is a zero tensor with a zero gradient, on this path too
    x = torch.randn(1, 19, 4, 4, requires_grad=True)
    loss = LovaszSoftmax({"dataset": "CITYSCAPES", "experiment": 1, "per_image": True})(x, torch.full((1, 4, 4), 19))
    loss.backward()
    assert torch.is_tensor(loss) and loss.dim() == 0 and loss.item() == 0.0 and bool(x.grad.eq(0).all())
