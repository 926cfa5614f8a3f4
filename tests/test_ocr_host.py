"""Host half of the OCR library and of OCRNet: the library is built next to the main one, exports and binds exactly what its
header declares, answers the shape test and sizes its workspaces by the documented formulas without touching a device; the modules
reproduce the reference's values and gradients on the CPU (fixtures G15); OCRNet builds from the shipped config with the
reference's state_dict keys and runs a training step through the manager's call pattern."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import mscs_amd  # noqa: F401
from mscs_amd import _lib
from mscs_amd.models import OCRNet          # (the feature: this import fails without it)

import _ocr_golden as og

REF = "/root/reference"
CONFIG = os.path.join(GOLDEN, "reference_configs", "hrnetocr_contrastive_ADE20K.json")


def _header():
    return open(os.path.join(ROOT, "include", "dcl_ocr.h")).read()


def test_fourth_library_is_built_by_the_same_target():
    from mscs_amd import _lib_ocr as la
    _lib.build()
    assert os.path.exists(la.LIB_PATH) and os.path.basename(la.LIB_PATH) == "libdcl_ocr.so"
    assert os.path.dirname(la.LIB_PATH) == os.path.dirname(_lib.LIB_PATH)


def test_header_exports_and_bindings_agree():
    from mscs_amd import _lib_ocr as la
    _lib.build()
    hdr = _header()
    names = sorted(set(re.findall(r"\b(dco_[a-z0-9_]+)\s*\(", hdr)))
    assert set(names) == {"dco_version", "dco_last_error", "dco_supported", "dco_splits", "dco_workspace_bytes", "dco_gather_fwd",
                          "dco_gather_bwd", "dco_attn_fwd", "dco_attn_bwd"}
    assert not re.findall(r"\b(dcl|dat)_[a-z0-9_]+\s*\(", hdr), "another library's prefix in this library's header"
    raw = ctypes.CDLL(la.LIB_PATH)
    for name in names:
        assert hasattr(raw, name), f"{name} declared in include/dcl_ocr.h but not exported"
    assert set(la.SIGNATURES) | {"dco_last_error"} == set(names)
    assert not any(n.startswith("dco_") for n in _lib.SIGNATURES)
    L = la.lib()
    assert L.dco_version() >= 1
    for name, sig in la.SIGNATURES.items():
        decl = re.search(rf"\b{name}\s*\(([^;]*)\);", hdr).group(1).strip()
        assert len(sig) == (0 if decl == "void" else decl.count(",") + 1), name
    for macro, value in (("DCO_TILE_N", la.TILE_N), ("DCO_CHUNK_C", la.CHUNK_C), ("DCO_MAX_SPLIT", la.MAX_SPLIT)):
        assert int(re.search(rf"#define {macro} (\d+)", hdr).group(1)) == value


def test_missing_library_error_names_the_build(monkeypatch):
    from mscs_amd import _lib_ocr as la
    monkeypatch.setattr(la, "_lib", None)
    monkeypatch.setattr(la, "LIB_PATH", os.path.join(ROOT, "no_such_dir", "libdcl_ocr.so"))
    with pytest.raises(RuntimeError) as e:
        la.lib()
    assert "not found" in str(e.value) and "build" in str(e.value)


def test_supported_is_host_arithmetic():
    from mscs_amd import _lib_ocr as la
    for c in (16, 48, 512, 1024):
        for k in (1, 19, 150, 256):
            for n in (1, 63, 64, 65, 16384):
                assert la.supported(1, c, k, n), (c, k, n)
    assert la.supported(16, 512, 150, 128 * 128) and la.supported(16, 256, 150, 128 * 128)        # the shipped config's sizes
    assert la.supported(12, 512, 19, 128 * 256)
    for c in (0, 8, 24, 40, 1040, 2048):
        assert not la.supported(1, c, 19, 64), c
    for k in (0, -1, 257):
        assert not la.supported(1, 64, k, 64), k
    assert not la.supported(1, 64, 19, 0) and not la.supported(0, 64, 19, 64)
    assert la.supported(65535, 16, 1, 1) and not la.supported(65536, 16, 1, 1)                   # the grid's y dimension
    assert not la.supported(1, 1024, 1, 1 << 21)                                                # B C N = 2^31
    assert la.supported(1, 1024, 1, (1 << 21) - 1)
    assert not la.supported(1, 16, 256, 1 << 23) and la.supported(1, 16, 256, (1 << 23) - 1)     # B K N = 2^31


def _splits(b, c, n):
    tiles, chunks = -(-n // 64), -(-c // 64)
    want = min(tiles, 16, max(1, -(-512 // (b * chunks))))
    per = -(-tiles // want)
    return -(-tiles // per)


def _formula(op, b, c, k, n):
    r = lambda x: (x + 255) // 256 * 256
    sp = _splits(b, c, n)
    return [r(4 * b * sp * k * c), 0, 0, r(8 * b * sp * c * k)][op]


def test_workspace_bytes_formulas():
    from mscs_amd import _lib_ocr as la
    shapes = [(16, 512, 150, 16384), (16, 256, 150, 16384), (12, 512, 19, 32768), (1, 16, 1, 1), (2, 48, 5, 37), (1, 512, 19, 16384),
              (1, 256, 150, 300), (2, 1024, 256, 65), (600, 64, 3, 100), (1, 64, 3, 17 * 64), (1, 64, 3, 35 * 57)]
    for b, c, k, n in shapes:
        assert la.splits(b, c, n) == _splits(b, c, n), (b, c, n)
        tiles, sp = -(-n // 64), la.splits(b, c, n)
        assert (sp - 1) * -(-tiles // sp) < tiles, "an empty split"
        for op in (la.GATHER_FWD, la.GATHER_BWD, la.ATTN_FWD, la.ATTN_BWD):
            assert la.workspace_bytes(op, b, c, k, n) == _formula(op, b, c, k, n), (op, b, c, k, n)
    # nothing of the size of a feature map or of the [B, N, K] scores: the largest workspace is 16 partial [K, C] matrices per image
    assert la.workspace_bytes(la.GATHER_FWD, 1, 512, 19, 16384) < 4 * 512 * 16384 // 4
    assert la.workspace_bytes(la.ATTN_BWD, 1, 256, 150, 16384) < 4 * 16384 * 150
    assert la.workspace_bytes(la.GATHER_FWD, 1, 24, 19, 64) == -1 and la.workspace_bytes(7, 1, 16, 1, 1) == -1
    assert la.workspace_bytes(la.ATTN_BWD, 1, 64, 257, 64) == -1 and la.splits(1, 24, 64) == 0


@pytest.mark.parametrize("case", og.CASES)
def test_cpu_forward_and_gradients_match_the_reference(case, monkeypatch):
    from mscs_amd import _lib_ocr as la
    monkeypatch.setattr(la, "lib", lambda: (_ for _ in ()).throw(AssertionError("the HIP library was asked for a CPU tensor")))
    g = og.load(case)
    assert os.path.getsize(os.path.join(GOLDEN, f"G15_ocr_{case}.npz")) < 100 * 1024
    threads = torch.get_num_threads()
    torch.set_num_threads(4)            # as tools/gen_golden_ocr.py: the CPU kernels' summation order depends on the thread count
    try:
        got = og.run(og.build(g), g)
    finally:
        torch.set_num_threads(threads)
    print(case, {k: f"{v:.2e}" for k, v in og.distances(got, og.golden(g)).items()})
    out, ctx, gxs, gps = got
    assert tuple(out.shape) == g["out0"].shape and tuple(ctx.shape) == g["ctx"].shape
    np.testing.assert_allclose(out.numpy(), g["out0"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(ctx.numpy(), g["ctx"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(gxs[0].numpy(), g["gx0"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(gxs[1].numpy(), g["gx1"], rtol=1e-5, atol=1e-6)
    assert sorted(gps) == sorted(g["g"])
    for k, v in gps.items():
        np.testing.assert_allclose(v.numpy(), g["g"][k], rtol=1e-5, atol=1e-6, err_msg=k)


def test_eager_cores_are_the_reference_compositions_and_work_without_grad():
    from mscs_amd.models import ops_ocr
    torch.manual_seed(0)
    feats, logits = torch.randn(2, 16, 3, 5), torch.randn(2, 4, 3, 5)
    ctx = ops_ocr.gather(feats, logits, 1)
    assert ctx.shape == (2, 16, 4, 1) and ctx.stride() == (64, 1, 16, 1)          # the permuted view of [B, K, C]
    p = torch.softmax(logits.view(2, 4, 15), dim=2)
    assert torch.allclose(ctx[..., 0], torch.einsum("bkn,bcn->bck", p, feats.view(2, 16, 15)), atol=1e-6)
    q, key, val = torch.randn(2, 16, 15), torch.randn(2, 16, 4), torch.randn(2, 16, 4)
    with torch.no_grad():
        out = ops_ocr.object_attention(q, key, val)
    a = torch.softmax(torch.einsum("bcn,bck->bnk", q, key) * 16 ** -0.5, dim=-1)
    assert out.is_contiguous() and torch.allclose(out, torch.einsum("bnk,bck->bcn", a, val), atol=1e-6)
    assert not ops_ocr.gather_hip_applies(feats, logits) and not ops_ocr.object_attention_hip_applies(q, key, val)


def _shipped(patch=None):
    with open(CONFIG) as f:
        cfg = json.load(f)
    cfg["graph"]["pretrained"] = False
    if patch:
        patch(cfg)
    dataset, experiment = cfg["data"]["dataset"], cfg["data"]["experiment"]
    cfg["graph"]["dataset"] = dataset
    cfg["loss"].update({"dataset": dataset, "experiment": experiment, "device": "cpu"})
    return cfg, experiment


def test_shipped_config_names_this_packages_classes():
    import mscs_amd.models as models
    cfg, _ = _shipped()
    assert cfg["graph"]["model"] == "OCRNet" and cfg["manager"] == "OCRNet" and cfg["graph"]["backbone"] == "hrnet48"
    for n in ("OCRNet", "SpatialGatherModule", "ObjectAttentionBlock2D", "SpatialOCR_Module"):
        assert getattr(models, n).__module__.endswith("models.OCR"), n
    assert models.OCRNet is OCRNet


def test_ocrnet_hrnet48_has_the_reference_state_dict():
    cfg, experiment = _shipped()
    model = OCRNet(config=cfg["graph"], experiment=experiment)
    with open(os.path.join(GOLDEN, "G15_ocrnet_hrnet48_keys.json")) as f:
        want = json.load(f)
    assert len(want) == 1922
    mine = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    assert [k for k, _ in mine] == [k for k, _ in want], "state_dict keys / order differ from the reference"
    assert mine == want
    assert model.num_classes == 150 and model.use_ms_projector and model.return_features and model.get_intermediate
    assert model.backbone.lazy_concat is False


def test_training_step_through_the_managers_call_pattern():
    from mscs_amd.losses import LossWrapper
    from mscs_amd.managers import OCRNetManager

    def small(cfg):
        cfg["graph"]["backbone"] = "hrnet18"
        cfg["loss"]["losses"] = {"TwoScaleLoss": 1}
    cfg, experiment = _shipped(small)
    torch.manual_seed(0)
    mgr = object.__new__(OCRNetManager)                 # forward_step only: no log directory, no dataset, no process group
    mgr.model = OCRNet(config=cfg["graph"], experiment=experiment).train()
    mgr.loss = LossWrapper(cfg["loss"])
    mgr.return_features, mgr.epoch, mgr.empty_cache = mgr.model.return_features, 0, False
    g = torch.Generator().manual_seed(0)
    img = torch.randn(2, 3, 64, 64, generator=g)
    lbl = torch.randint(0, 150, (2, 64, 64), generator=g)
    ret = mgr.forward_step(img, lbl)
    ret["loss"].backward()
    assert list(ret["interm_output"].shape) == [2, 150, 64, 64] and list(ret["output"].shape) == [2, 150, 64, 64]
    assert [list(f.shape) for f in ret["feats"]] == [[2, 256, 16, 16], [2, 256, 8, 8], [2, 256, 4, 4], [2, 256, 2, 2]]
    assert bool(torch.isfinite(ret["loss"])) and float(ret["loss"]) > 0
    assert sorted(mgr.loss.loss_vals) == ["TwoScaleLoss"]
    missing = [k for k, p in mgr.model.named_parameters() if not k.startswith("projector_model") and p.grad is None]
    assert not missing, missing[:5]
    # get_intermediate / return_features as in the reference
    mgr.model.eval()
    with torch.no_grad():
        mgr.model.get_intermediate = False
        assert len(mgr.model(img)) == 2
        mgr.model.return_features = False
        out = mgr.model(img)
        assert torch.is_tensor(out) and list(out.shape) == [2, 150, 64, 64]


def test_single_projector_reads_the_concatenation_or_the_ocr_features():
    for before, c_in in ((True, 270), (False, 512)):
        graph = {"dataset": "CITYSCAPES", "backbone": "hrnet18", "pretrained": False, "align_corners": True,
                 "projector": {"mlp": [[1, -1, 1]], "d": 32, "before_context": before}}
        model = OCRNet(config=graph, experiment=1).eval()
        assert model.projector_model.c_in == c_in
        with torch.no_grad():
            interm, out, feats = model(torch.randn(1, 3, 64, 64))
        assert list(out.shape) == [1, 19, 64, 64] and list(interm.shape) == [1, 19, 64, 64] and list(feats.shape) == [1, 32, 16, 16]


def test_resnet_backbone_raises_the_documented_error():
    for name in ("resnet50", "resnet101"):
        with pytest.raises(NotImplementedError, match="torchvision"):
            OCRNet(config={"dataset": "CITYSCAPES", "backbone": name, "pretrained": False}, experiment=1)
    with pytest.raises(NotImplementedError, match="torchvision"):
        OCRNet(config={"dataset": "CITYSCAPES", "pretrained": False}, experiment=1)      # the reference's default backbone


def test_scale_two_raises_the_documented_error():
    from mscs_amd.models import ObjectAttentionBlock2D, SpatialOCR_Module
    with pytest.raises(NotImplementedError, match="scale must be 1"):
        ObjectAttentionBlock2D(32, 16, scale=2)
    with pytest.raises(NotImplementedError, match="scale must be 1"):
        SpatialOCR_Module(32, 16, 32, scale=2)


def test_switch_defaults_on():
    from mscs_amd.debug import cfg as dbg
    assert dbg.ocr_hip is True or os.environ.get("DCL_OCR_HIP") == "0"


LIVE = r"""
import json, os, sys
sys.path.insert(0, os.path.join(%(root)r, "tools"))
sys.path.insert(0, %(root)r)
import ref_shim
ref_shim.install(); ref_shim.quiet()
import numpy as np
import torch
import builtins
_print = builtins.print
builtins.print = lambda *a, **k: None
import mscs_amd
from mscs_amd.models import OCRNet as Mine
from models.OCR import OCRNet as Ref                       # the REFERENCE's
import models.OCR as refmod
assert refmod.__file__.startswith("/root/reference/"), refmod.__file__
cfg = json.load(open(%(config)r))
graph = cfg["graph"]; graph["pretrained"] = False; graph["dataset"] = cfg["data"]["dataset"]
torch.manual_seed(0)
ref = Ref(config=json.loads(json.dumps(graph)), experiment=cfg["data"]["experiment"]).train()
x = torch.randn(2, 3, 64, 64)
state = {k: v.clone() for k, v in ref.state_dict().items()}
want = ref(x)
mine = Mine(config=json.loads(json.dumps(graph)), experiment=cfg["data"]["experiment"]).train()
mine.load_state_dict(state, strict=True)
ref.load_state_dict(mine.state_dict(), strict=True)
got = mine(x)
flat = lambda o: [o[0], o[1]] + list(o[2])
out = {"n": [len(flat(want)), len(flat(got))], "err": [], "shapes": []}
for a, b in zip(flat(got), flat(want)):
    a, b = a.detach().numpy(), b.detach().numpy()
    out["shapes"].append([list(a.shape), list(b.shape)])
    tol = 1e-4 * max(1.0, float(np.abs(b).max()))
    out["err"].append([float(np.abs(a - b).max()), tol])
    np.testing.assert_allclose(a, b, atol=tol, rtol=1e-4)
_print("RESULT " + json.dumps(out))
"""


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference checkout not present (GPU box)")
@pytest.mark.timeout(600)
def test_live_comparison_with_the_reference_ocrnet():
    env = dict(os.environ, OMP_NUM_THREADS="4")
    r = subprocess.run([sys.executable, "-c", LIVE % {"root": ROOT, "config": CONFIG}], capture_output=True, text=True, env=env,
                       cwd=REF, timeout=580)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    print(out)
    assert out["n"] == [6, 6]
    assert all(a == b for a, b in out["shapes"])
    assert out["shapes"][0][0] == [2, 150, 64, 64] and out["shapes"][1][0] == [2, 150, 64, 64]
