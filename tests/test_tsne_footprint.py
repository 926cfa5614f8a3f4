"""Footprint of every device entry of libdcl_tsne.so at the C ABI (include/dcl_tsne.h) on guarded buffers (tests/_footprint.py): P,
beta, Y, iY, gains, dY, every partial buffer and the KL history sit between poisoned bands that must be intact after each entry,
every output is fully written, and nothing depends on what lies outside the inputs.  Then the same entries on buffers whose base
lies 4 bytes off a 16-byte boundary: the 4-byte loads of P and Y, the same values."""
import pytest
import torch

from _footprint import SENTINEL, bands_intact, fill_bits, first_damage, guarded, run_both

import _tsne_cases as cases

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_tsne
    _lib_tsne.lib()
    return torch.device("cuda:0")


def _inputs(n):
    d, s = 17, 5.0
    X = cases.make_x(n, d, s)
    P, Y = cases.grad_state(n, d, s)
    dY, iY, gains, _ = cases.update_inputs(n)
    return X, P, Y, dY, iY, gains


def _sequence(lt, dev, n, new_in, new_out, new_io, check):
    """every entry once on buffers from the three makers; ``check(what)`` after each; returns {name: output}"""
    X, P0, Y0, dY0, iY0, g0 = (t.to(dev) for t in _inputs(n))
    plan, u = lt.plan(n), cases.perplexity_for(n)
    out = {}
    for scratch in (False, True):
        P, beta = new_out((n, n), "P"), new_out((n,), "beta")
        lt.cond_p(new_in(X, "X"), u, P, beta, scratch=scratch)
        check(f"cond_p scratch={scratch}")
        out[f"P{int(scratch)}"], out[f"beta{int(scratch)}"] = P, beta
    S, part = new_io(P0, "P in place"), new_out((plan["sym_groups"],), "sym partials")
    lt.symmetrize(S, part)
    check("symmetrize")
    Pin, Yin = new_in(P0, "P"), new_in(Y0, "Y")
    zpart, klpart = new_out((plan["z_parts"],), "zpart"), new_out((plan["grad_groups"],), "klpart")
    dY, dY1, z_out = new_out((n, 2), "dY"), new_out((n, 2), "dY no KL"), new_out((1,), "Z")
    lt.zsum(Yin, zpart)
    check("zsum")
    lt.gradient(Pin, Yin, 4.0, zpart, dY, klpart, z_out)
    check("gradient KL")
    lt.gradient(Pin, Yin, 1.0, zpart, dY1)
    check("gradient")
    iY, gains, Y = new_io(iY0, "iY"), new_io(g0, "gains"), new_io(Y0, "Y in place")
    colpart, kl_out = new_out((2 * plan["upd_groups"],), "colpart"), new_out((1,), "KL")
    lt.update(new_in(dY0, "dY in"), iY, gains, Y, 0.8, colpart, klpart, kl_out)
    check("update")
    rY, riY, rg = new_io(Y0, "run Y"), new_io(torch.zeros_like(Y0), "run iY"), new_io(torch.ones_like(Y0), "run gains")
    rdY, ws, hist = new_out((n, 2), "run dY"), new_out((plan["ws_floats"],), "ws"), new_out((2,), "kl history")
    lt.run(Pin, rY, riY, rg, rdY, ws, 0, 20, hist)
    check("run")
    out.update(S=S, part=part, zpart=zpart, klpart=klpart, dY=dY, dY1=dY1, Z=z_out, iY=iY, gains=gains, Y=Y, colpart=colpart, KL=kl_out,
               rY=rY, riY=riY, rg=rg, rdY=rdY, ws=ws, hist=hist)
    return out


@pytest.mark.parametrize("n", (33, 257))
def test_every_entry_between_guard_bands(dev, n):
    from mscs_amd import _lib_tsne as lt

    def body(ar):
        return _sequence(lt, dev, n, ar.inp, lambda shape, name: ar.out(shape, F32, name), ar.io, ar.check)
    got = run_both(dev, body, ("tsne", n))
    assert torch.equal(got["P0"], got["P1"]) and torch.equal(got["S"], got["S"].T)
    ref = cases.grad_reference(n, 17, 5.0, 4.0)
    assert cases.rel_max(got["dY"], ref["dY"]) <= max(4 * ref["e_dY"], cases.floor(n))


@pytest.mark.parametrize("n", (33, 257, 256))
def test_bases_four_bytes_off_sixteen(dev, n):
    """n = 256: rows of P that would take the 16-byte loads but for the base"""
    from mscs_amd import _lib_tsne as lt
    kept = []

    def shifted(shape):
        numel = 1
        for s in shape:
            numel *= int(s)
        view, whole = guarded((numel + 1,), F32, dev)
        fill_bits(whole, SENTINEL)
        body = view[1:].view(shape)
        assert body.data_ptr() % 16 == 4
        kept.append((whole, view, body))
        return body

    def put(t, _name=None):
        b = shifted(tuple(t.shape))
        b.copy_(t)
        return b

    def check(what):
        torch.cuda.synchronize()
        for whole, view, _ in kept:
            assert bands_intact(whole, view), (what, first_damage(whole, view))
            assert view.view(torch.int32)[0].item() == SENTINEL, (what, "the word in front of a shifted buffer")
    assert not lt.plan_grad_vec(16 + 4, n)
    off = _sequence(lt, dev, n, put, lambda shape, _name: shifted(shape), put, check)
    plain = _sequence(lt, dev, n, lambda t, _n=None: t.clone(), lambda shape, _n: torch.empty(shape, dtype=F32, device=dev),
                      lambda t, _n=None: t.clone(), lambda what: None)
    torch.cuda.synchronize()
    same_order = n % 4 != 0                                                              # else 4-byte against 16-byte loads: another order
    for k in ("P0", "beta0", "P1", "S", "zpart", "Z", "iY", "gains", "Y", "colpart", "KL"):
        assert torch.equal(off[k], plain[k]), k
    for k in ("dY", "dY1", "klpart", "rY", "hist"):
        if same_order:
            assert torch.equal(off[k], plain[k]), k
        elif k in ("rY", "hist"):                                                        # twenty iterations on: the trajectories part
            assert bool(torch.isfinite(off[k]).all()), k
        else:
            assert cases.rel_max(off[k], plain[k]) <= cases.floor(n), k
    ref = cases.grad_reference(n, 17, 5.0, 4.0)
    assert cases.rel_max(off["dY"], ref["dY"]) <= max(4 * ref["e_dY"], cases.floor(n))
