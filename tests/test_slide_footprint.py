"""Footprint of the sliding-window entries at the C ABI (include/dcl_slide.h): dsw_crops / dsw_gather on guarded buffers
(tests/_footprint.py): every band intact, every output fully written, finite and independent of what lies outside the inputs, and
the values those of models/ops_slide.py on torch-allocated buffers."""
import pytest
import torch

from _footprint import run_both
import _slide_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_slide
    _lib_slide.lib()
    return torch.device("cuda:0")


#        (C, image (H, W), resized (nh, nw), window (wh, ww), row starts, column starts)
CASES = [(5, (22, 30), (44, 60), (16, 24), [0, 10, 20, 30], [0, 16, 32, 48]),     # every row length a multiple of 4: 16-byte stores
         (19, (17, 29), (23, 31), (7, 10), [0, 5, 11, 16], [0, 9, 15, 21]),       # odd everywhere: element by element
         (150, (9, 11), (13, 18), (8, 12), [0, 5], [0, 6])]                       # classes split over grid y


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"C{c[0]}_{c[2][0]}x{c[2][1]}")
def test_slide_entries_footprint(dev, case):
    from mscs_amd import _lib_slide as ls
    from mscs_amd.models import ops_slide
    C, (H, W), (nh, nw), (wh, ww), rows_lo, cols_lo = case
    R, Q = len(rows_lo), len(cols_lo)
    N = R * Q
    L = ls.lib()
    st = ls.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(C * 100 + nh + nw)
    x = torch.randn(3, H, W, device=dev, generator=g)
    h, w = -(-wh // 4), -(-ww // 4)
    z = torch.randn(N, C, h, w, device=dev, generator=g) * 2
    zf = torch.randn(N, C, h, w, device=dev, generator=g) * 2
    rl, cl, pad = ls.ints(rows_lo), ls.ints(cols_lo), ls.floats(sc.PAD)

    def body(ar):
        out = ar.out((2 * N, 3, wh, ww), name="crops")
        ls.check(L.dsw_crops(ar.inp(x, "x").data_ptr(), 3, H, W, nh, nw, rl, R, cl, Q, wh, ww, pad, 1, out.data_ptr(), st), "dsw_crops")
        out1 = ar.out((N, 3, wh, ww), name="crops plain")
        ls.check(L.dsw_crops(ar.inp(x, "x 2").data_ptr(), 3, H, W, nh, nw, rl, R, cl, Q, wh, ww, pad, 0, out1.data_ptr(), st), "dsw_crops")
        canvas = ar.out((C, nh, nw), name="canvas")
        ls.check(L.dsw_gather(ar.inp(z, "z").data_ptr(), ar.inp(zf, "zf").data_ptr(), C, h, w, wh, ww, 1, rl, R, cl, Q,
                              canvas.data_ptr(), nh, nw, st), "dsw_gather")
        canvas1 = ar.out((C, nh, nw), name="canvas no flip")
        ls.check(L.dsw_gather(ar.inp(z, "z 2").data_ptr(), None, C, h, w, wh, ww, 0, rl, R, cl, Q, canvas1.data_ptr(), nh, nw, st),
                 "dsw_gather")
        return {"crops": out, "crops1": out1, "canvas": canvas, "canvas1": canvas1}
    got = run_both(dev, body, ("slide", case[:4]))

    # the values are those of the Python entry points (the same calls on torch-allocated buffers)
    assert torch.equal(got["crops"], ops_slide.crops(x, (nh, nw), rows_lo, cols_lo, (wh, ww), sc.PAD, True))
    assert torch.equal(got["crops1"], ops_slide.crops(x, (nh, nw), rows_lo, cols_lo, (wh, ww), sc.PAD, False))
    assert torch.equal(got["crops1"], got["crops"][:N])
    assert torch.equal(got["canvas"], ops_slide.gather(z, zf, (wh, ww), 1, rows_lo, cols_lo, torch.empty(C, nh, nw, device=dev)))
    assert torch.equal(got["canvas1"], ops_slide.gather(z, None, (wh, ww), 0, rows_lo, cols_lo, torch.empty(C, nh, nw, device=dev)))
    assert bool((got["canvas"] > 0).all()) and bool((got["canvas1"] > 0).all())           # a mean of exp(.)
