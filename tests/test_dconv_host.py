"""Host half of the dilated-convolution library and of DeepLabv3: the fifth library is built next to the main one, exports and binds
exactly what its header declares, answers the shape test, the live-tap mask, the slab count and the workspace sizes by the
documented formulas without touching a device; DilatedConv2d is nn.Conv2d on the CPU; ASPP reproduces the reference's values and
gradients (fixtures G16 a / b / c), DeepLabv3 its wiring (G16_deeplabv3_wiring); the ResNet backbones have torchvision's parameters
and dilation rule; the manager's forward_step runs a CE training step."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import mscs_amd  # noqa: F401
from mscs_amd import _lib
from mscs_amd.models import ASPP, DeepLabv3, resnet50, resnet101          # (the feature: this import fails without it)

import _aspp_golden as ag

ENTRIES = {"ddc_version", "ddc_last_error", "ddc_supported", "ddc_live_taps", "ddc_wgrad_slabs", "ddc_workspace_bytes",
           "ddc_packed_bytes", "ddc_pack", "ddc_fwd", "ddc_dgrad", "ddc_wgrad"}


def _header():
    return open(os.path.join(ROOT, "include", "dcl_dconv.h")).read()


def test_fifth_library_is_built_by_the_same_target():
    from mscs_amd import _lib_dconv as ld
    _lib.build()
    assert os.path.exists(ld.LIB_PATH) and os.path.basename(ld.LIB_PATH) == "libdcl_dconv.so"
    assert os.path.dirname(ld.LIB_PATH) == os.path.dirname(_lib.LIB_PATH)
    flags = subprocess.run(["make", "-s", "-C", _lib.CSRC_DIR, "print-cxxflags"], capture_output=True, text=True).stdout
    assert "--offload-arch=gfx950" in flags


def test_header_exports_and_bindings_agree():
    from mscs_amd import _lib_dconv as ld
    _lib.build()
    hdr = _header()
    names = set(re.findall(r"\b(ddc_[a-z0-9_]+)\s*\(", hdr))
    assert names == ENTRIES
    assert not re.findall(r"\b(dcl|dat|dco)_[a-z0-9_]+\s*\(", hdr), "another library's prefix in this library's header"
    nm = subprocess.run(["nm", "-D", "--defined-only", ld.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l}
    assert exported == ENTRIES, exported ^ ENTRIES           # exactly the header's symbols
    raw = ctypes.CDLL(ld.LIB_PATH)
    assert all(hasattr(raw, n) for n in names)
    assert set(ld.SIGNATURES) | {"ddc_last_error"} == names
    assert not any(n.startswith("ddc_") for n in _lib.SIGNATURES)
    assert ld.lib().ddc_version() >= 1
    for name, sig in ld.SIGNATURES.items():
        decl = re.search(rf"^[a-z0-9_ ]+\*?{name}\s*\(([^;]*)\);", hdr, re.M).group(1).strip()      # (the declaration, not a mention)
        assert len(sig) == (0 if decl == "void" else decl.count(",") + 1), name
    for macro, value in (("DDC_TILE_P", ld.TILE_P), ("DDC_TILE_CO", ld.TILE_CO), ("DDC_CHUNK_CI", ld.CHUNK_CI),
                         ("DDC_WG_TILE", ld.WG_TILE), ("DDC_WG_CHUNK_P", ld.WG_CHUNK_P), ("DDC_MAX_SLABS", ld.MAX_SLABS),
                         ("DDC_SLAB_MIN_UNITS", ld.SLAB_MIN_UNITS), ("DDC_WG_TARGET", ld.WG_TARGET)):
        assert int(re.search(rf"#define {macro} (\d+)", hdr).group(1)) == value


def test_missing_library_error_names_the_build(monkeypatch):
    from mscs_amd import _lib_dconv as ld
    monkeypatch.setattr(ld, "_lib", None)
    monkeypatch.setattr(ld, "LIB_PATH", os.path.join(ROOT, "no_such_dir", "libdcl_dconv.so"))
    with pytest.raises(RuntimeError) as e:
        ld.lib()
    assert "not found" in str(e.value) and "build" in str(e.value)


def test_supported_accepts_and_refuses_by_the_table():
    from mscs_amd import _lib_dconv as ld
    ok = (2, 32, 48, 9, 13, 2)                                  # (N, Ci, Co, H, W, d)
    assert ld.supported(*ok)
    assert ld.supported(16, 2048, 256, 32, 32, 36) and ld.supported(16, 2048, 256, 64, 64, 12)      # ASPP, out_stride 16 / 8
    assert ld.supported(16, 512, 512, 32, 32, 2) and ld.supported(16, 256, 256, 64, 64, 2)          # layer4, layer3
    for ci in (8, 24, 40, 4104):                                # Ci % 16 == 0
        assert not ld.supported(2, ci, 48, 9, 13, 2), ci
    for co in (8, 24, 40, 4104):                                # Co % 16 == 0
        assert not ld.supported(2, 32, co, 9, 13, 2), co
    assert ld.supported(1, 16, 16, 1, 1, 1) and not ld.supported(1, 0, 16, 1, 1, 1) and not ld.supported(1, 16, 0, 1, 1, 1)
    assert ld.supported(1, 4096, 4096, 1, 1, 1)                 # 16 <= Ci, Co <= 4096
    assert not ld.supported(1, 4112, 16, 1, 1, 1) and not ld.supported(1, 16, 4112, 1, 1, 1)
    assert ld.supported(1, 16, 16, 4, 4, 64) and not ld.supported(1, 16, 16, 4, 4, 65)              # 1 <= d <= 64
    assert not ld.supported(1, 16, 16, 4, 4, 0) and not ld.supported(1, 16, 16, 4, 4, -1)
    assert not ld.supported(1, 16, 16, 0, 4, 1) and not ld.supported(1, 16, 16, 4, 0, 1)            # H, W >= 1
    assert ld.supported(65535, 16, 16, 1, 1, 1) and not ld.supported(65536, 16, 16, 1, 1, 1)        # N <= 65535
    assert not ld.supported(0, 16, 16, 1, 1, 1)
    assert not ld.supported(1, 16, 32, 1 << 13, 1 << 14, 1)     # N Ci H W = 2^31
    assert not ld.supported(1, 32, 16, 1 << 13, 1 << 14, 1)
    assert ld.supported(1, 16, 16, (1 << 13) - 1, 1 << 14, 1)   # just under 2^31 elements
    assert not ld.supported(1, 16, 16, 1 << 16, 1 << 16, 1)     # H W itself past 2^31


def _live(h, w, d):
    m = 0
    for ky in range(3):
        for kx in range(3):
            dead = (ky != 1 and d >= h) or (kx != 1 and d >= w)
            if not dead:
                m |= 1 << (3 * ky + kx)
    return m


def _slabs(n, ci, co, h, w, d):
    units = n * -(-h * w // 16)
    tiles = -(-co // 32) * -(-ci // 32) * bin(_live(h, w, d)).count("1")
    want = min(max(1, -(-2048 // tiles)), 64, max(1, units // 32))
    per = -(-units // want)
    return -(-units // per)


def _formula(op, n, ci, co, h, w, d):
    r = lambda x: (x + 255) // 256 * 256
    return [256, 256, 512 + r(4 * _slabs(n, ci, co, h, w, d) * bin(_live(h, w, d)).count("1") * co * ci)][op]


def test_live_tap_mask_is_the_stated_rule():
    from mscs_amd import _lib_dconv as ld
    for h, w in ((5, 5), (13, 17), (32, 32)):
        for d in (1, 2, 6, 12, 18, 36):
            assert ld.live_taps(h, w, d) == _live(h, w, d), (h, w, d)
    assert ld.live_taps(32, 32, 36) == 1 << 4 and ld.live_taps(5, 5, 6) == 1 << 4      # centre only: a 1x1 convolution
    assert ld.live_taps(13, 17, 12) == 0x1FF and ld.live_taps(13, 17, 6) == 0x1FF
    assert ld.live_taps(13, 17, 13) == 0b000111000                                     # the centre row of taps
    assert ld.live_taps(13, 17, 18) == 1 << 4 and ld.live_taps(1, 1, 1) == 1 << 4
    assert ld.live_taps(0, 5, 1) == 0 and ld.live_taps(5, 5, 0) == 0


def test_workspace_bytes_formulas():
    from mscs_amd import _lib_dconv as ld
    shapes = [(16, 2048, 256, 32, 32, 12), (16, 2048, 256, 32, 32, 36), (16, 2048, 256, 64, 64, 24), (16, 512, 512, 32, 32, 2),
              (16, 256, 256, 64, 64, 2), (2, 16, 16, 5, 7, 1), (1, 32, 48, 9, 13, 2), (2, 48, 16, 13, 17, 6), (1, 16, 32, 13, 17, 12),
              (1, 16, 16, 8, 8, 12), (1, 16, 16, 1, 1, 3), (2, 48, 80, 23, 29, 4), (3, 16, 16, 100, 100, 3)]
    for s in shapes:
        assert ld.wgrad_slabs(*s) == _slabs(*s), s
        n, h, w = s[0], s[3], s[4]
        units, sl = n * -(-h * w // 16), ld.wgrad_slabs(*s)
        assert 1 <= sl <= 64 and (sl - 1) * -(-units // sl) < units, "an empty slab"
        for op in (ld.FWD, ld.DGRAD, ld.WGRAD):
            assert ld.workspace_bytes(op, *s) == _formula(op, *s), (op, s)
    assert ld.wgrad_slabs(2, 48, 80, 23, 29, 4) > 1 and ld.wgrad_slabs(16, 256, 256, 64, 64, 2) > 1
    assert ld.workspace_bytes(ld.FWD, 1, 24, 16, 4, 4, 1) == -1 and ld.workspace_bytes(7, 1, 16, 16, 4, 4, 1) == -1
    assert ld.workspace_bytes(ld.WGRAD, 1, 16, 16, 4, 4, 65) == -1 and ld.wgrad_slabs(1, 24, 16, 4, 4, 1) == 0
    assert ld.packed_bytes(48, 32, False) == 36 * 64 * 32 and ld.packed_bytes(48, 32, True) == 36 * 32 * 48
    assert ld.packed_bytes(24, 32, False) == -1


def test_dilated_conv2d_on_cpu_is_nn_conv2d(monkeypatch):
    from mscs_amd import _lib_dconv as ld
    from mscs_amd.models.ops_dconv import DilatedConv2d
    monkeypatch.setattr(ld, "lib", lambda: (_ for _ in ()).throw(AssertionError("the HIP library was asked for a CPU tensor")))
    torch.manual_seed(0)
    ref = torch.nn.Conv2d(16, 32, 3, padding=3, dilation=3)
    mine = DilatedConv2d(16, 32, 3, padding=3, dilation=3)
    assert list(mine.state_dict()) == list(ref.state_dict())
    mine.load_state_dict(ref.state_dict(), strict=True)
    x = torch.randn(2, 16, 9, 11)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    assert not mine.eligible(xa)
    ya, yb = ref(xa), mine(xb)
    cot = torch.randn_like(ya)
    ya.backward(cot)
    yb.backward(cot)
    assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad)
    assert torch.equal(ref.weight.grad, mine.weight.grad) and torch.equal(ref.bias.grad, mine.bias.grad)


def test_use_dilated_conv3x3_swaps_only_its_geometry():
    from mscs_amd.models.ops_dconv import DilatedConv2d, use_dilated_conv3x3
    C = torch.nn.Conv2d
    mods = {"yes2": C(16, 16, 3, padding=2, dilation=2), "yes36": C(16, 16, 3, padding=36, dilation=36, bias=False),
            "d1": C(16, 16, 3, padding=1), "stride2": C(16, 16, 3, stride=2, padding=2, dilation=2),
            "pad": C(16, 16, 3, padding=1, dilation=2), "groups": C(16, 16, 3, padding=2, dilation=2, groups=2),
            "k1": C(16, 16, 1), "k5": C(16, 16, 5, padding=4, dilation=2), "aniso": C(16, 16, 3, padding=(2, 3), dilation=(2, 3)),
            "reflect": C(16, 16, 3, padding=2, dilation=2, padding_mode="reflect")}
    net = use_dilated_conv3x3(torch.nn.ModuleDict(mods))
    swapped = sorted(k for k, m in net.items() if type(m) is DilatedConv2d)
    assert swapped == ["yes2", "yes36"]
    assert all(type(m) is C for k, m in net.items() if k not in swapped)


def test_switch_defaults_on():
    from mscs_amd.debug import cfg as dbg
    assert dbg.dconv_hip is True or os.environ.get("DCL_DCONV_HIP") == "0"


@pytest.mark.parametrize("case", ag.CASES)
def test_aspp_cpu_forward_and_gradients_match_the_reference(case, monkeypatch):
    from mscs_amd import _lib_dconv as ld
    monkeypatch.setattr(ld, "lib", lambda: (_ for _ in ()).throw(AssertionError("the HIP library was asked for a CPU tensor")))
    g = ag.load(case)
    assert os.path.getsize(os.path.join(GOLDEN, f"G16_aspp_{case}.npz")) < 1024 * 1024
    assert g["config"]["B"] >= 2 and g["config"]["mult"] == 1
    threads = torch.get_num_threads()
    torch.set_num_threads(4)            # as tools/gen_golden_aspp.py: the CPU kernels' summation order depends on the thread count
    try:
        m = ag.build(g)                 # (loads the fixture's state strictly)
        assert m.aspp1_bn.eps == 0.0003 and m.aspp1_bn.momentum == 0.1 and m.bn2.eps == 0.0003
        got = ag.run(m, g)
    finally:
        torch.set_num_threads(threads)
    print(case, {k: f"{v:.2e}" for k, v in ag.distances(got, ag.golden(g)).items()})
    out, gx, gps = got
    assert tuple(out.shape) == g["out0"].shape
    np.testing.assert_allclose(out.numpy(), g["out0"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(gx.numpy(), g["gx0"], rtol=1e-5, atol=1e-6)
    assert sorted(gps) == sorted(g["g"])
    for k, v in gps.items():
        np.testing.assert_allclose(v.numpy(), g["g"][k], rtol=1e-5, atol=1e-6, err_msg=k)


def test_deeplabv3_wiring_matches_the_reference():
    from mscs_amd.utils import set_verbosity
    set_verbosity(40)
    w = ag.wiring()
    assert os.path.getsize(ag.WIRING) < 1024 * 1024
    c = w["config"]
    model = DeepLabv3(c["graph"], c["experiment"])
    mine = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    head = [e for e in mine if not e[0].startswith("backbone.")]
    assert [k for k, _ in head] == [k for k, _ in w["head"]], "head keys / order differ from the reference"
    assert head == w["head"]
    assert {k.split(".")[0] for k, _ in head} == {"aspp", "conv_out", "projector_model"}
    assert mine == w["keys"]
    model.load_state_dict({k: ag.formula_tensor(k, tuple(s)) for k, s in w["keys"]}, strict=True)
    model.eval()
    threads = torch.get_num_threads()
    torch.set_num_threads(4)
    try:
        with torch.no_grad():
            logits, feats = model(ag.wiring_input(c))
    finally:
        torch.set_num_threads(threads)
    assert list(logits.shape) == [c["B"], 19, c["H"], c["W"]] and len(feats) == 3
    np.testing.assert_allclose(logits.numpy(), w["logits"], rtol=1e-5, atol=1e-6)
    for i, f in enumerate(feats):
        np.testing.assert_allclose(f.numpy(), w[f"feat{i}"], rtol=1e-5, atol=1e-6, err_msg=f"feat{i}")


def _torchvision_dilations(blocks, out_stride):
    """torchvision's rule: a dilated layer multiplies the running dilation by its stride; its first block keeps the previous one"""
    flags = {8: [False, True, True], 16: [False, False, True], 32: [False, False, False]}[out_stride]
    want, dil = {}, 1
    for L, (n, flag) in enumerate(zip(blocks, [False] + flags), start=1):
        prev = dil
        if flag:
            dil *= 2
        for b in range(n):
            want[f"layer{L}.{b}"] = prev if b == 0 else dil
    return want, flags


def test_resnet_backbones_have_torchvisions_parameters_and_dilations():
    for factory, blocks, total in ((resnet50, [3, 4, 6, 3], 23508032), (resnet101, [3, 4, 23, 3], 42500160)):
        m = factory(pretrained=False)
        sd = m.state_dict()
        assert sum(p.numel() for p in m.parameters()) == total
        assert list(sd["layer1.0.downsample.0.weight"].shape) == [256, 64, 1, 1]
        assert list(sd["layer4.2.conv3.weight"].shape) == [2048, 512, 1, 1]
        assert list(sd["conv1.weight"].shape) == [64, 3, 7, 7] and "bn1.running_var" in sd and "layer4.0.downsample.1.bias" in sd
        assert ("layer3.22.conv2.weight" in sd) == (blocks[2] == 23)
        assert not any(k.startswith(("fc.", "avgpool")) for k in sd)
        top = {k.split(".")[0] for k in sd}
        assert top == {"conv1", "bn1", "layer1", "layer2", "layer3", "layer4"}
    for out_stride in (8, 16, 32):
        want, flags = _torchvision_dilations([3, 4, 6, 3], out_stride)
        m = resnet50(pretrained=False, replace_stride_with_dilation=flags,
                     return_layers={"layer1": "C2", "layer2": "C3", "layer3": "C4", "layer4": "C5"}).eval()
        for name, d in want.items():
            L, b = name.split(".")
            conv2 = getattr(m, L)[int(b)].conv2
            assert conv2.dilation == (d, d) and conv2.padding == (d, d), (out_stride, name, conv2.dilation)
        with torch.no_grad():
            out = m(torch.randn(1, 3, 64, 96))
        assert list(out) == ["C2", "C3", "C4", "C5"]
        assert list(out["C5"].shape) == [1, 2048, 64 // out_stride, 96 // out_stride], (out_stride, out["C5"].shape)
        assert list(out["C2"].shape) == [1, 256, 16, 24]


def test_strided_shortcut_is_a_correct_sequential():
    """downsample.0 of a strided block keeps torchvision's attributes and, called as the Sequential it is, gives the strided 1x1
    convolution's values and shape."""
    from mscs_amd.models.ResNet import SubsampledConv1x1
    torch.manual_seed(1)
    m = resnet50(pretrained=False).eval()
    for L, strided in (("layer1", False), ("layer2", True), ("layer3", True), ("layer4", True)):
        conv = getattr(m, L)[0].downsample[0]
        assert (type(conv) is SubsampledConv1x1) == strided and conv.stride == ((2, 2) if strided else (1, 1))
    ds = m.layer2[0].downsample
    x = torch.randn(2, 256, 9, 13)
    with torch.no_grad():
        got = ds(x)
        want = ds[1](torch.nn.functional.conv2d(x, ds[0].weight, None, stride=2))
    assert list(got.shape) == [2, 512, 5, 7]
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-6)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ds[0](xa).sum().backward()
    torch.nn.functional.conv2d(xb, ds[0].weight, None, stride=2).sum().backward()
    assert torch.allclose(xa.grad, xb.grad, rtol=1e-5, atol=1e-6)


def test_pretrained_checkpoint_must_fit(monkeypatch, tmp_path):
    good = {k: v for k, v in resnet50(pretrained=False).state_dict().items() if not k.endswith("num_batches_tracked")}
    good["fc.weight"], good["fc.bias"] = torch.zeros(2, 2048), torch.zeros(2)          # torchvision's classifier: dropped
    path = tmp_path / "r50.pth"
    monkeypatch.setenv("RESNET_PRETRAINED", str(path))
    torch.save(good, path)
    m = resnet50(pretrained=True)
    assert torch.equal(m.layer4[2].conv3.weight, good["layer4.2.conv3.weight"])
    torch.save({"module." + k: v for k, v in good.items()}, path)                       # a prefixed checkpoint loads nothing: refused
    with pytest.raises(RuntimeError, match="missing"):
        resnet50(pretrained=True)
    bad = dict(good)
    del bad["layer1.0.conv1.weight"]
    torch.save(bad, path)
    with pytest.raises(RuntimeError, match="layer1.0.conv1.weight"):
        resnet50(pretrained=True)


def test_pretrained_never_fetches_and_resnet18_is_refused(monkeypatch, tmp_path):
    monkeypatch.setenv("RESNET_PRETRAINED", str(tmp_path / "absent.pth"))
    with pytest.raises(FileNotFoundError, match="RESNET_PRETRAINED"):
        resnet50(pretrained=True)
    with pytest.raises(FileNotFoundError):
        DeepLabv3({"dataset": "CITYSCAPES", "backbone": "resnet101"}, 1)          # ``pretrained`` defaults to true, as in the reference
    with pytest.raises(NotImplementedError, match="resnet18"):
        DeepLabv3({"dataset": "CITYSCAPES", "backbone": "resnet18", "pretrained": False}, 1)


def test_kernels_are_selected_by_geometry():
    from mscs_amd.models.ops import DirectConv2d
    from mscs_amd.models.ops_dconv import DilatedConv2d
    from mscs_amd.utils import set_verbosity
    set_verbosity(40)
    m = DeepLabv3({"dataset": "CITYSCAPES", "pretrained": False, "out_stride": 8}, 1)
    assert not m.return_features and m.projector_model is None and m.aspp._c_in == 2048
    assert [type(getattr(m.aspp, f"aspp{i}")) for i in range(1, 6)] == [DirectConv2d] + [DilatedConv2d] * 3 + [DirectConv2d]
    assert [getattr(m.aspp, f"aspp{i}").dilation[0] for i in (2, 3, 4)] == [12, 24, 36]
    assert type(m.backbone.conv1) is torch.nn.Conv2d                                     # the 7x7 stem stays on PyTorch
    for L, blocks in (("layer3", 6), ("layer4", 3)):
        kinds = [type(getattr(m.backbone, L)[b].conv2) for b in range(blocks)]
        assert kinds == [DirectConv2d] + [DilatedConv2d] * (blocks - 1) if L == "layer3" else kinds == [DilatedConv2d] * blocks
    assert type(m.backbone.layer2[0].conv2) is DirectConv2d and type(m.backbone.layer2[0].conv1) is DirectConv2d


def test_manager_forward_step_cross_entropy_on_cpu():
    from mscs_amd.losses import LossWrapper
    from mscs_amd.managers import DeepLabv3Manager
    from mscs_amd.utils import set_verbosity
    set_verbosity(40)
    torch.manual_seed(0)
    graph = {"dataset": "CITYSCAPES", "backbone": "resnet50", "pretrained": False, "out_stride": 16,
             "ms_projector": {"mlp": [[1, -1, 1]], "feats": ["layer1", "layer3", "layer4"], "d": 16, "use_bn": True,
                              "before_context": True}}
    mgr = object.__new__(DeepLabv3Manager)              # forward_step only: no log directory, no dataset, no process group
    mgr.model = DeepLabv3(graph, 1).train()
    mgr.loss = LossWrapper({"dataset": "CITYSCAPES", "experiment": 1, "device": "cpu", "losses": {"CrossEntropyLoss": 1}})
    mgr.return_features, mgr.epoch, mgr.empty_cache = mgr.model.return_features, 0, False
    g = torch.Generator().manual_seed(0)
    img = torch.randn(2, 3, 33, 49, generator=g)
    lbl = torch.randint(0, 19, (2, 33, 49), generator=g)
    ret = mgr.forward_step(img, lbl)
    assert sorted(ret) == ["feats", "interm_output", "loss", "output"] and ret["interm_output"] is None
    ret["loss"].backward()
    assert list(ret["output"].shape) == [2, 19, 33, 49]
    assert [list(f.shape) for f in ret["feats"]] == [[2, 16, 9, 13], [2, 16, 3, 4], [2, 16, 3, 4]]
    assert bool(torch.isfinite(ret["loss"])) and float(ret["loss"].detach()) > 0
    missing = [k for k, p in mgr.model.named_parameters() if not k.startswith("projector_model") and p.grad is None]
    assert not missing, missing[:5]
