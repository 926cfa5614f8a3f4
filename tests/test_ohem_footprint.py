"""Footprint of the hard-pixel mining entries at the C ABI (include/dcl_ohem.h): doh_target_prob, doh_select and doh_reduce on guarded
buffers (tests/_footprint.py): every band intact, the maps, the result words and the whole workspace (exactly doh_workspace_bytes)
fully written, and nothing depends on what lies outside the inputs."""
import pytest
import torch

import _ohem_cases as cases
from _footprint import run_both

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib, _lib_ohem
    _lib.lib()
    _lib_ohem.lib()
    return torch.device("cuda:0")


@pytest.mark.parametrize("ci", [2, 1], ids=lambda ci: "x".join(str(v) for v in cases.CASES[ci][:5]))
def test_ohem_entries_footprint(dev, ci):
    import importlib

    from mscs_amd import _lib, _lib_ohem as oh
    d = cases.inputs(ci)
    N, C, h, w = d["z"].shape
    H, W = d["size"]
    thresh, mk = cases.settings(d["n"])[2]
    z, t = d["z"].to(dev), d["t"].to(dev)
    wt = None if d["w"] is None else d["w"].to(dev)
    st = oh.stream_ptr(dev)
    # the log-sum-exp map the first entry reads: the main library's, on ordinary buffers
    lse = torch.empty(N, H, W, device=dev)
    partial, out2 = torch.empty(N * H, 2, device=dev), torch.empty(2, device=dev)
    _lib.check(_lib.lib().dcl_upsample_ce_fwd(_lib.ptr(z), N, C, h, w, H, W, 1 if d["align"] else 0, _lib.ptr(t), None, d["ignore"],
                                              _lib.ptr(lse), None, _lib.ptr(partial), _lib.ptr(out2), st), "dcl_upsample_ce_fwd")
    nbytes = oh.workspace_bytes(N, H)
    off, bins = oh.layout()
    assert nbytes == 4 * (off["part"] + 2 * N * H) and bins == [2048, 2048, 1024]

    def body(ar):
        zz, tt, ll = ar.inp(z, "logits"), ar.inp(t, "labels"), ar.inp(lse, "lse")
        ww = None if wt is None else ar.inp(wt, "weights")
        ws = ar.out(nbytes, torch.uint8, "workspace")
        p, l = ar.out((N, H, W), name="p"), ar.out((N, H, W), name="l")
        hard, kept = ar.out((N, H, W), torch.int64, "hard"), ar.out((N, H, W), torch.uint8, "kept")
        res = ar.out(oh.RES_WORDS, torch.int32, "res")
        oh.target_prob(zz, (H, W), d["align"], tt, ww, d["ignore"], ll, p, l, ws, st)
        oh.select(p, mk, thresh, ws, st)
        oh.reduce(p, l, tt, d["ignore"], ws, hard, kept, res, st)
        # (p holds a NaN pattern at the invalid pixels: compared as words)
        return {"p": p.view(torch.int32), "l": l, "hard": hard, "kept": kept, "res": res, "workspace": ws}
    got = run_both(dev, body, ("ohem", cases.CASES[ci]))

    # and the values are those of the module (which takes the same entries through torch-allocated buffers)
    m = importlib.import_module("mscs_amd.losses.OhemCrossEntropy")
    holder = {"want_kept": True}
    loss = m.ohem_cross_entropy(z, t, wt, d["ignore"], thresh, mk, size=d["size"], align_corners=d["align"], holder=holder)
    assert holder["path"] == "hip"
    assert torch.equal(got["res"], holder["res"]) and torch.equal(got["res"].view(torch.float32)[oh.RES_LOSS], loss)
    assert torch.equal(got["p"], holder["p"].view(torch.int32)) and torch.equal(got["hard"], holder["hard"])
    assert torch.equal(got["kept"], holder["kept"]) and int(got["res"][oh.RES_M]) == int(got["kept"].sum()) > 0
    # the histograms of the three passes count what they should: all valid pixels, then the pivot's bin of the pass before
    words = got["workspace"].view(torch.int32)
    h0 = words[off["hist0"]:off["hist0"] + bins[0]]
    assert int(h0.sum()) == d["n"] == int(got["res"][oh.RES_N])
    vbits = int(got["res"][oh.RES_V])
    assert int(words[off["hist1"]:off["hist1"] + bins[1]].sum()) == int(h0[vbits >> 21])
