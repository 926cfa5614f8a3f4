"""Footprint of the attention entries at the C ABI (include/dcl_attn.h): dat_attn_fwd and dat_attn_bwd on guarded buffers
(tests/_footprint.py): every band intact, out / lse / dqkv fully written, finite and independent of what lies outside the inputs
(a tail load that entered a result would show), and workspaces of exactly dat_workspace_bytes whose bands stay untouched."""
import pytest
import torch

from _footprint import run_both

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_attn
    _lib_attn.lib()
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else t.data_ptr()


CASES = [(2, 37, 2, 16), (1, 129, 1, 48), (1, 300, 1, 256)]       # (B, N, heads, D)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_attention_entries_footprint(dev, case):
    from mscs_amd import _lib_attn as la
    from mscs_amd.models.ops_attn import _Attention
    B, N, heads, D = case
    C = heads * D
    L = la.lib()
    st = la.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(B * 100 + N + D)
    qkv = torch.randn(B, N, 3 * C, device=dev, generator=g)
    dout = torch.randn(B, N, C, device=dev, generator=g)
    scale = D ** -0.5
    nf, nb = la.workspace_bytes(B, N, heads, D, False), la.workspace_bytes(B, N, heads, D, True)
    assert 0 < nf <= nb < 64 * B * heads * N + 4096

    def body(ar):
        x = ar.inp(qkv, "qkv")
        wf = ar.out(nf, torch.uint8, "workspace fwd")
        assert wf.data_ptr() % 256 == 0
        out, lse = ar.out((B, N, C), name="out"), ar.out((B, heads, N), name="lse")
        la.check(L.dat_attn_fwd(_p(x), B, N, heads, D, scale, _p(wf), nf, _p(out), _p(lse), st), "dat_attn_fwd")
        torch.cuda.synchronize()
        wb = ar.out(nb, torch.uint8, "workspace bwd")
        assert wb.data_ptr() % 256 == 0
        dqkv = ar.out((B, N, 3 * C), name="dqkv")
        la.check(L.dat_attn_bwd(_p(x), _p(ar.inp(out, "out in")), _p(ar.inp(lse, "lse in")), _p(ar.inp(dout, "dout")), B, N,
                                heads, D, scale, _p(wb), nb, _p(dqkv), st), "dat_attn_bwd")
        return {"out": out, "lse": lse, "dqkv": dqkv}
    got = run_both(dev, body, ("attention", case))

    # and the values are those of the autograd Function (which takes the same entries through torch-allocated buffers)
    x = qkv.clone().requires_grad_(True)
    out = _Attention.apply(x, heads, scale)
    out.backward(dout)
    assert torch.equal(got["out"], out.detach()) and torch.equal(got["dqkv"], x.grad)
    # a too small workspace is refused before anything is launched
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    assert L.dat_attn_bwd(_p(qkv), _p(out), _p(got["lse"]), _p(dout), B, N, heads, D, scale, _p(ws), nb - 1, _p(x.grad), st) != 0
    assert b"workspace" in L.dat_last_error()
