"""Footprint of the OCR entries at the C ABI (include/dcl_ocr.h): dco_gather_fwd / dco_gather_bwd / dco_attn_fwd / dco_attn_bwd on
guarded buffers (tests/_footprint.py): every band intact, every output fully written, finite and independent of what lies outside
the inputs, workspaces of exactly dco_workspace_bytes whose bands stay untouched, and a workspace one byte short refused before
anything is launched (dco_gather_bwd and dco_attn_fwd need none: there is no byte to take away)."""
import pytest
import torch

from _footprint import run_both

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_ocr
    _lib_ocr.lib()
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else t.data_ptr()


CASES = [(2, 16, 16, 5, 37), (1, 48, 32, 19, 65), (1, 512, 256, 150, 300)]       # (B, C, Ck, K, N); 65 = one tile + 1


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_ocr_entries_footprint(dev, case):
    from mscs_amd import _lib_ocr as la
    from mscs_amd.models.ops_ocr import _Gather, _ObjectAttention
    B, C, Ck, K, N = case
    L = la.lib()
    st = la.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(B * 100 + N + C)
    x = torch.randn(B, C, N, device=dev, generator=g)
    logits = torch.randn(B, K, N, device=dev, generator=g) * 3
    dctx = torch.randn(B, K, C, device=dev, generator=g)
    q = torch.randn(B, Ck, N, device=dev, generator=g)
    key = torch.randn(B, Ck, K, device=dev, generator=g)
    val = torch.randn(B, Ck, K, device=dev, generator=g)
    dout = torch.randn(B, Ck, N, device=dev, generator=g)
    s = Ck ** -0.5
    ngf, ngb = la.workspace_bytes(la.GATHER_FWD, B, C, K, N), la.workspace_bytes(la.GATHER_BWD, B, C, K, N)
    naf, nab = la.workspace_bytes(la.ATTN_FWD, B, Ck, K, N), la.workspace_bytes(la.ATTN_BWD, B, Ck, K, N)
    assert ngf > 0 and ngb == 0 and naf == 0 and nab > 0

    def body(ar):
        xg, lg = ar.inp(x, "x"), ar.inp(logits, "logits")
        w1 = ar.out(ngf, torch.uint8, "workspace gather fwd")
        assert w1.data_ptr() % 256 == 0
        ctx, stats = ar.out((B, K, C), name="ctx"), ar.out((B, K, 2), name="stats")
        la.check(L.dco_gather_fwd(_p(xg), _p(lg), B, C, K, N, 1.0, _p(w1), ngf, _p(ctx), _p(stats), st), "dco_gather_fwd")
        torch.cuda.synchronize()
        dx, dl = ar.out((B, C, N), name="dx"), ar.out((B, K, N), name="dlogits")
        la.check(L.dco_gather_bwd(_p(xg), _p(lg), _p(ar.inp(ctx, "ctx in")), _p(ar.inp(stats, "stats in")), _p(ar.inp(dctx, "dctx")),
                                  B, C, K, N, 1.0, None, 0, _p(dx), _p(dl), st), "dco_gather_bwd")
        qg, kg, vg = ar.inp(q, "q"), ar.inp(key, "key"), ar.inp(val, "val")
        out = ar.out((B, Ck, N), name="out")
        la.check(L.dco_attn_fwd(_p(qg), _p(kg), _p(vg), B, Ck, K, N, s, None, 0, _p(out), st), "dco_attn_fwd")
        w4 = ar.out(nab, torch.uint8, "workspace attn bwd")
        assert w4.data_ptr() % 256 == 0
        dq, dk, dv = ar.out((B, Ck, N), name="dq"), ar.out((B, Ck, K), name="dkey"), ar.out((B, Ck, K), name="dval")
        la.check(L.dco_attn_bwd(_p(qg), _p(kg), _p(vg), _p(ar.inp(dout, "dout")), B, Ck, K, N, s, _p(w4), nab, _p(dq), _p(dk),
                                _p(dv), st), "dco_attn_bwd")
        return {"ctx": ctx, "stats": stats, "dx": dx, "dlogits": dl, "out": out, "dq": dq, "dkey": dk, "dval": dv}
    got = run_both(dev, body, ("ocr", case))

    # and the values are those of the autograd Functions (which take the same entries through torch-allocated buffers)
    xa, la_ = x.clone().requires_grad_(True), logits.clone().requires_grad_(True)
    ctx = _Gather.apply(xa, la_, 1.0)
    ctx.backward(dctx)
    assert torch.equal(got["ctx"], ctx.detach()) and torch.equal(got["dx"], xa.grad) and torch.equal(got["dlogits"], la_.grad)
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, key, val))
    out = _ObjectAttention.apply(qa, ka, va)
    out.backward(dout)
    assert torch.equal(got["out"], out.detach()) and torch.equal(got["dq"], qa.grad)
    assert torch.equal(got["dkey"], ka.grad) and torch.equal(got["dval"], va.grad)

    # a too small workspace is refused before anything is launched
    ws = torch.empty(max(ngf, nab), dtype=torch.uint8, device=dev)
    scratch = torch.empty_like(x), torch.empty_like(logits), torch.empty_like(q), torch.empty_like(key), torch.empty_like(val)
    assert L.dco_gather_fwd(_p(x), _p(logits), B, C, K, N, 1.0, _p(ws), ngf - 1, _p(got["ctx"]), _p(got["stats"]), st) != 0
    assert b"workspace" in L.dco_last_error()
    assert L.dco_gather_bwd(_p(x), _p(logits), _p(got["ctx"]), _p(got["stats"]), _p(dctx), B, C, K, N, 1.0, None, -1,
                            _p(scratch[0]), _p(scratch[1]), st) != 0
    assert b"workspace" in L.dco_last_error()
    assert L.dco_attn_bwd(_p(q), _p(key), _p(val), _p(dout), B, Ck, K, N, s, _p(ws), nab - 1, _p(scratch[2]), _p(scratch[3]),
                          _p(scratch[4]), st) != 0
    assert b"workspace" in L.dco_last_error()
    assert L.dco_attn_fwd(_p(q), _p(key), _p(val), B, Ck, K, N, s, None, -1, _p(scratch[2]), st) != 0
    assert b"workspace" in L.dco_last_error()
