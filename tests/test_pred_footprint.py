"""Footprint of the prediction entries at the C ABI (include/dcl_pred.h): dpr_predict and dpr_panel on guarded buffers
(tests/_footprint.py): every band around every output intact, every output fully written and independent of what lies outside the
inputs, at a width that forces the byte-wise stores, at one that takes the 4-byte stores, and on an output that starts off a 4-byte
boundary; the values are those of utils/predict.py on torch-allocated buffers."""
import pytest
import torch

from _footprint import SENTINEL, bands_intact, fill_bits, first_damage, guarded, run_both

import _pred_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_pred
    _lib_pred.lib()
    return torch.device("cuda:0")


#        (N, C, h, w, H, W, align)
CASES = [(2, 19, 5, 7, 17, 23, 0),           # W = 23: byte by byte, a tail of three
         (2, 19, 8, 12, 32, 48, 1),          # W = 48: 4-byte stores
         (1, 150, 13, 9, 50, 33, 1),         # W = 33: a tail of one
         (2, 19, 16, 24, 16, 24, 0),         # the identity level, 16-byte loads
         (1, 19, 16, 21, 16, 21, 0)]         # the identity level, scalar loads


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_predict_and_panel_footprint(dev, case):
    from mscs_amd import _lib_pred as lp
    from mscs_amd.models.ops_logits import UpsampledLogits
    from mscs_amd.utils import panel_image, predict_maps
    N, C, h, w, H, W, align = case
    L, st = lp.lib(), lp.stream_ptr(dev)
    z = cases.logits(C, h, w, N).to(dev)
    lut, pal = (t.to(dev) for t in cases.tables())
    g = torch.Generator().manual_seed(H * W)
    img = torch.randn(3, H, W, generator=g).to(dev)
    lbl = torch.randint(0, 21, (H, W), generator=g).to(dev)

    def body(ar):
        zg, lg, pg = ar.inp(z, "z"), ar.inp(lut, "lut"), ar.inp(pal, "palette")
        ids, mapped = ar.out((N, H, W), torch.uint8, "ids"), ar.out((N, H, W), torch.uint8, "mapped")
        rgb = ar.out((N, H, W, 3), torch.uint8, "rgb")
        lp.check(L.dpr_predict(zg.data_ptr(), N, C, h, w, H, W, align, lg.data_ptr(), pg.data_ptr(), ids.data_ptr(), mapped.data_ptr(),
                               rgb.data_ptr(), st), "dpr_predict")
        only = ar.out((N, H, W), torch.uint8, "ids alone")
        lp.check(L.dpr_predict(zg.data_ptr(), N, C, h, w, H, W, align, None, None, only.data_ptr(), None, None, st), "dpr_predict")
        torch.cuda.synchronize()
        panel = ar.out((H, 3 * W, 3), torch.uint8, "panel")
        lp.check(L.dpr_panel(ar.inp(img, "img").data_ptr(), ar.inp(lbl, "label").data_ptr(), 8, ar.inp(ids[0], "ids in").data_ptr(),
                             pg.data_ptr(), H, W, 0.485, 0.456, 0.406, 0.229, 0.224, 0.225, 20, 19, panel.data_ptr(), st), "dpr_panel")
        return {"ids": ids, "mapped": mapped, "rgb": rgb, "only": only, "panel": panel}
    got = run_both(dev, body, ("pred", case))

    out = UpsampledLogits(z, (H, W), bool(align)) if (h, w) != (H, W) else z
    want = predict_maps(out, lut, pal)
    assert torch.equal(got["ids"], want[0]) and torch.equal(got["mapped"], want[1]) and torch.equal(got["rgb"], want[2])
    assert torch.equal(got["only"], want[0])
    assert torch.equal(got["panel"], panel_image(img, lbl, want[0][0], pal, label_ignore=20, ids_ignore=19))


@pytest.mark.parametrize("shift", (1, 2, 3))
def test_outputs_off_the_word_boundary(dev, shift):
    """W is a multiple of the run, but the outputs start 1, 2 or 3 bytes off a 4-byte boundary: byte stores, the same values, and the
    bytes in front of and behind each output unchanged."""
    from mscs_amd import _lib_pred as lp
    from mscs_amd.models.ops_logits import UpsampledLogits
    from mscs_amd.utils import predict_maps
    N, C, h, w, H, W, align = CASES[1]
    L, st = lp.lib(), lp.stream_ptr(dev)
    z = cases.logits(C, h, w, N).to(dev)
    lut, pal = (t.to(dev) for t in cases.tables())
    views = {}
    for name, n in (("ids", N * H * W), ("mapped", N * H * W), ("rgb", 3 * N * H * W)):
        view, whole = guarded((n + 4,), torch.uint8, dev)
        fill_bits(whole, SENTINEL)
        views[name] = (view, whole, view[shift:shift + n])
    lp.check(L.dpr_predict(z.data_ptr(), N, C, h, w, H, W, align, lut.data_ptr(), pal.data_ptr(), views["ids"][2].data_ptr(),
                           views["mapped"][2].data_ptr(), views["rgb"][2].data_ptr(), st), "dpr_predict")
    torch.cuda.synchronize()
    want = predict_maps(UpsampledLogits(z, (H, W), bool(align)), lut, pal)
    pattern = torch.tensor([SENTINEL], dtype=torch.int32, device=dev).view(torch.uint8)
    for (name, (view, whole, body)), ref in zip(views.items(), want):
        assert bands_intact(whole, view), (name, first_damage(whole, view))
        assert torch.equal(body, ref.reshape(-1)), name
        assert torch.equal(view[:shift], pattern[:shift]), name                        # (the view starts on a 16-byte boundary)
        tail = view[shift + body.numel():]
        assert torch.equal(tail, pattern.repeat(2)[(shift + body.numel()) % 4:][:tail.numel()]), name
