"""Host half of the attention library and of Projector(trans=True): the library is built next to the main one, exports and binds
exactly what its header declares, answers the shape test and sizes its workspace by the documented formula; the module builds
with the reference's state_dict keys and reproduces the reference's values and gradients on the CPU (fixtures G14)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import mscs_amd  # noqa: F401
from mscs_amd import _lib

import _attn_golden as ag


def _header():
    return open(os.path.join(ROOT, "include", "dcl_attn.h")).read()


def test_third_library_is_built_by_the_same_target():
    from mscs_amd import _lib_attn as la
    _lib.build()
    assert os.path.exists(la.LIB_PATH) and os.path.basename(la.LIB_PATH) == "libdcl_attn.so"
    assert os.path.dirname(la.LIB_PATH) == os.path.dirname(_lib.LIB_PATH)


def test_header_exports_and_bindings_agree():
    from mscs_amd import _lib_attn as la
    _lib.build()
    hdr = _header()
    names = sorted(set(re.findall(r"\b(dat_[a-z0-9_]+)\s*\(", hdr)))
    assert set(names) == {"dat_version", "dat_last_error", "dat_supported", "dat_workspace_bytes", "dat_attn_fwd", "dat_attn_bwd"}
    assert not re.findall(r"\bdcl_[a-z0-9_]+\s*\(", hdr), "the main library's prefix in the third library's header"
    raw = ctypes.CDLL(la.LIB_PATH)
    for name in names:
        assert hasattr(raw, name), f"{name} declared in include/dcl_attn.h but not exported"
    assert set(la.SIGNATURES) | {"dat_last_error"} == set(names)          # dat_last_error: a char * result, bound separately
    assert not any(n.startswith("dat_") for n in _lib.SIGNATURES)
    L = la.lib()
    assert L.dat_version() >= 1
    for name, sig in la.SIGNATURES.items():          # the arity of every binding is the declaration's
        decl = re.search(rf"\b{name}\s*\(([^;]*)\);", hdr).group(1).strip()
        assert len(sig) == (0 if decl == "void" else decl.count(",") + 1), name


def test_missing_library_error_names_the_build(monkeypatch):
    from mscs_amd import _lib_attn as la
    monkeypatch.setattr(la, "_lib", None)
    monkeypatch.setattr(la, "LIB_PATH", os.path.join(ROOT, "no_such_dir", "libdcl_attn.so"))
    with pytest.raises(RuntimeError) as e:
        la.lib()
    assert "not found" in str(e.value) and "build" in str(e.value)


def test_supported_is_host_arithmetic():
    from mscs_amd import _lib_attn as la
    for d in (16, 48, 256):
        for n in (1, 32768):
            assert la.supported(1, n, 1, d), (n, d)
    for d in (18, 8, 272):
        assert not la.supported(1, 64, 1, d), d
    assert la.supported(2, 32768, 4, 64)                                  # the benchmark's 1/4-resolution map
    assert not la.supported(8, 32768, 32, 256)                            # 8 * 32768 * 3 * 32 * 256 >= 2^31
    assert not la.supported(1, 1 << 22, 1, 256)                           # 2^22 * 768 >= 2^31
    assert la.supported(1, (1 << 31) // 768 - 1, 1, 256)                  # the last N below it
    assert not la.supported(0, 64, 1, 16) and not la.supported(1, 0, 1, 16) and not la.supported(1, 64, 0, 16)


def _formula(b, n, heads, backward):
    r = lambda x: (x + 255) // 256 * 256
    return r(16 * b * heads) + (r(4 * b * heads * n) if backward else 0)


def test_workspace_bytes_formula_and_linear_in_tokens():
    from mscs_amd import _lib_attn as la
    for b, n, heads, d in [(2, 32768, 4, 64), (2, 32768, 1, 256), (1, 1, 1, 16), (2, 1995, 1, 48), (3, 300, 3, 32)]:
        for bwd in (False, True):
            got = la.workspace_bytes(b, n, heads, d, bwd)
            assert got == _formula(b, n, heads, bwd), (b, n, heads, d, bwd, got)
            assert la.workspace_bytes(b, n + 1, heads, d, bwd) >= got
    for heads, d in [(1, 256), (4, 64), (16, 16)]:
        b, n = 2, 32768
        assert la.workspace_bytes(b, n, heads, d, True) < 64 * b * heads * n + 4096      # O(B heads N): lse-sized, no N x N
    assert la.workspace_bytes(1, 64, 1, 18, True) == -1 and la.workspace_bytes(1, 1 << 22, 1, 256, False) == -1


@pytest.mark.parametrize("case", ag.CASES)
def test_projector_trans_builds_with_the_reference_keys(case):
    g = ag.load(case)
    from mscs_amd.models.Projector import Projector
    from mscs_amd.models.Transformers import SelfAttention
    m = Projector(dict(g["config"]))
    assert list(m.state_dict()) == g["keys"].tolist()
    heads = [getattr(m, f"project{i}") for i in range(len(m.c_in))] if m.is_ms else [m.project]
    for h in heads:
        assert isinstance(h[-2], SelfAttention) and h[-2].num_heads == g["config"]["heads"]
        assert isinstance(h[-1], torch.nn.Conv2d) and h[-1].kernel_size == (1, 1)


@pytest.mark.parametrize("case", ag.CASES)
def test_cpu_forward_and_gradients_match_the_reference(case, monkeypatch):
    from mscs_amd import _lib_attn as la
    monkeypatch.setattr(la, "lib", lambda: (_ for _ in ()).throw(AssertionError("the HIP library was asked for a CPU tensor")))
    g = ag.load(case)
    m = ag.build(g)
    outs, gxs, gps = ag.run(m, g)
    print(case, {k: f"{v:.2e}" for k, v in ag.distances((outs, gxs, gps), g).items()})
    for i in range(g["n"]):
        assert tuple(outs[i].shape) == g[f"out{i}"].shape
        np.testing.assert_allclose(outs[i].numpy(), g[f"out{i}"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(gxs[i].numpy(), g[f"gx{i}"], rtol=1e-5, atol=1e-6)
    assert sorted(gps) == sorted(k[2:] for k in g if k.startswith("g:"))
    for k, v in gps.items():
        np.testing.assert_allclose(v.numpy(), g["g:" + k], rtol=1e-5, atol=1e-6, err_msg=k)


def test_token_view_quirk_and_output_strides():
    """A 4-D input is reread as [B, H W, C] rows of its NCHW memory (no transpose); the result has NCHW shape and channels-last
    strides, as the reference's ``view(B, H, W, C).permute(0, 3, 1, 2)``."""
    from mscs_amd.models.Transformers import SelfAttention
    torch.manual_seed(0)
    sa = SelfAttention(dim=8, heads=2)
    assert list(sa.state_dict()) == ["qkv.weight", "proj.weight", "proj.bias"]
    assert list(SelfAttention(dim=8, heads=2, qkv_bias=True).state_dict()) == ["qkv.weight", "qkv.bias", "proj.weight", "proj.bias"]
    x = torch.randn(2, 8, 3, 5)
    y = sa(x)
    assert y.shape == x.shape and y.stride() == (120, 1, 40, 8)
    tok = sa(x.reshape(2, 15, 8))                                         # the same memory as tokens
    assert torch.equal(y.permute(0, 2, 3, 1).reshape(2, 15, 8), tok)
    assert torch.equal(sa(x.to(memory_format=torch.channels_last)), y)    # other strides in: made NCHW-contiguous first
    assert sa(x, unflatten_output=False).shape == (2, 15, 8)


def test_projector_without_trans_is_unchanged():
    from mscs_amd.models.Projector import Projector
    m = Projector({"c_in": 32, "mlp": [[1, -1, 1], [1, 64, 1]], "use_bn": True, "d": 32})
    assert [type(l).__name__ for l in m.project] == ["Conv2d", "ReLU", "BatchNorm2d", "Conv2d", "ReLU", "BatchNorm2d", "Conv2d"]
    assert list(m.state_dict()) == [f"project.{i}.{k}" for i, ks in (
        (0, ["weight"]), (2, ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]),
        (3, ["weight"]), (5, ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]),
        (6, ["weight", "bias"])) for k in ks]
    ms = Projector({"c_in": [16, 32], "mlp": [], "d": 16, "trans": False, "heads": 4})
    assert list(ms.state_dict()) == ["project0.0.weight", "project0.0.bias", "project1.0.weight", "project1.0.bias"]
    assert not any("Attention" in type(l).__name__ for l in ms.modules())


def test_switch_defaults_on():
    from mscs_amd.debug import cfg as dbg
    assert dbg.attn_hip is True or os.environ.get("DCL_ATTN_HIP") == "0"
