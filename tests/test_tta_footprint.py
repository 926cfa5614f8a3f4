"""Footprint of the test-time-augmentation entries at the C ABI (include/dcl_tta.h): dtt_merge / dtt_window_accum / dtt_canvas_merge
on guarded buffers (tests/_footprint.py): every band intact, every accumulator finite and independent of what lies outside the
inputs, only the window region of the canvas changed, and the values those of models/ops_tta.py on torch-allocated buffers."""
import pytest
import torch

from _footprint import run_both

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_tta
    _lib_tta.lib()
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else t.data_ptr()


#        (C, h, w, Hm, Wm, H, W, canvas Hc x Wc, crop, window (h0, w0, wh, ww))
CASES = [(5, 6, 9, 22, 33, 30, 44, (24, 48), (16, 24), (8, 24, 16, 24)),       # W a multiple of 4: 16-byte accesses
         (19, 4, 5, 16, 18, 8, 9, (12, 23), (7, 9), (5, 13, 7, 9)),            # odd everything: element by element
         (150, 3, 3, 3, 3, 7, 5, (9, 8), (9, 8), (0, 0, 9, 8)),                # identity inner level, classes split over grid y
         (5, 4, 6, 16, 24, 20, 40, (24, 48), (16, 24), (3, 4, 13, 22))]        # aligned start, a tail of two columns


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c[:7]))
def test_tta_entries_footprint(dev, case):
    from mscs_amd import _lib_tta as lt
    from mscs_amd.models import ops_tta
    C, h, w, Hm, Wm, H, W, (Hc, Wc), (ch, cw), (h0, w0, wh, ww) = case
    L = lt.lib()
    st = lt.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(C * 100 + H + W)
    z = torch.randn(C, h, w, device=dev, generator=g) * 2
    zh, zw = -(-ch // 4), -(-cw // 4)
    zc = torch.randn(C, zh, zw, device=dev, generator=g) * 2
    zf = torch.randn(C, zh, zw, device=dev, generator=g) * 2
    acc0 = torch.randn(C, H, W, device=dev, generator=g)
    canvas0 = torch.rand(C, Hc, Wc, device=dev, generator=g) + 0.5
    rowcnt = torch.randint(1, 4, (Hc,), device=dev, generator=g, dtype=torch.int32)
    colcnt = torch.randint(1, 4, (Wc,), device=dev, generator=g, dtype=torch.int32)

    def body(ar):
        zg = ar.inp(z, "z")
        acc = ar.io(acc0, "acc")
        lt.check(L.dtt_merge(_p(zg), C, h, w, Hm, Wm, 0, 1, _p(acc), H, W, 1, 0.5, st), "dtt_merge")
        canvas = ar.io(canvas0, "canvas")
        lt.check(L.dtt_window_accum(_p(ar.inp(zc, "zc")), _p(ar.inp(zf, "zf")), C, zh, zw, ch, cw, 1, _p(canvas), Hc, Wc, h0, w0, wh, ww,
                                    st), "dtt_window_accum")
        canvas1 = ar.io(canvas0, "canvas no flip")
        lt.check(L.dtt_window_accum(_p(ar.inp(zc, "zc 2")), None, C, zh, zw, ch, cw, 0, _p(canvas1), Hc, Wc, h0, w0, wh, ww, st),
                 "dtt_window_accum")
        torch.cuda.synchronize()
        acc2 = ar.io(acc0, "acc 2")
        lt.check(L.dtt_canvas_merge(_p(ar.inp(canvas, "canvas in")), _p(ar.inp(rowcnt, "rowcnt")), _p(ar.inp(colcnt, "colcnt")), C, Hc,
                                    Wc, _p(acc2), H, W, 0, st), "dtt_canvas_merge")
        return {"acc": acc, "canvas": canvas, "canvas1": canvas1, "acc2": acc2}
    got = run_both(dev, body, ("tta", case))

    # only the window region of the canvas changes
    inside = torch.zeros(Hc, Wc, dtype=torch.bool, device=dev)
    inside[h0:h0 + wh, w0:w0 + ww] = True
    for k in ("canvas", "canvas1"):
        assert torch.equal(got[k][:, ~inside], canvas0[:, ~inside]), k
        assert bool((got[k][:, inside] > canvas0[:, inside]).all()), k              # exp(.) > 0 was added everywhere inside
    # and the values are those of the Python entry points (the same calls on torch-allocated buffers)
    assert torch.equal(got["acc"], ops_tta.merge(z, (Hm, Wm), 0, 1, acc0.clone(), 1, 0.5))
    assert torch.equal(got["canvas"], ops_tta.window_accum(zc, zf, (ch, cw), 1, canvas0.clone(), h0, w0, wh, ww))
    assert torch.equal(got["canvas1"], ops_tta.window_accum(zc, None, (ch, cw), 0, canvas0.clone(), h0, w0, wh, ww))
    assert torch.equal(got["acc2"], ops_tta.canvas_merge(got["canvas"], rowcnt, colcnt, acc0.clone(), 0))
