"""libdcl_tsne.so on the GPU against the torch composition of utils/tsne.py in float64 on the CPU (tests/_tsne_cases.py).  A bar
"4 x e32" is four times the distance of the SAME composition in float32 from the float64 one on the same inputs, with the stated
floor; the code under test never supplies its own bar.  N in {33, 130, 257} leaves remainders of every tile (32, 8, 4, 256) and
takes both the 16-byte and the 4-byte loads of P; dts_cond_p runs with a row's distances in LDS and in the row of P itself."""
import math

import numpy as np
import pytest
import torch

import _tsne_cases as cases
from _tsne_cases import F32, F64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_tsne
    _lib_tsne.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lt():
    from mscs_amd import _lib_tsne
    return _lib_tsne


def _empty(dev, *shape):
    return torch.full(shape, float("nan"), dtype=F32, device=dev)


# ---- dts_cond_p --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_cond_p(dev, lt, case):
    n, d, s = case
    X, u, ref = cases.make_x(n, d, s), cases.perplexity_for(n), cases.cond_reference(n, d, s)
    outs = []
    for scratch in (False, True):
        P, beta = _empty(dev, n, n), _empty(dev, n)
        lt.cond_p(X.to(dev), u, P, beta, scratch=scratch)
        outs.append((P.cpu(), beta.cpu()))
    (P, beta), (Pg, betag) = outs
    assert torch.equal(P, Pg) and torch.equal(beta, betag), "the row of P as scratch gives other values than LDS"
    assert bool(torch.isfinite(P).all()) and bool((beta > 0).all()) and float(P.diagonal().abs().max()) == 0.0
    P64, H = cases.p_at_beta(X, beta)
    err, res = cases.rel_max(P, P64, dim=1), float((H - math.log(u)).abs().max())
    bar = max(4 * ref["e32"], 4e-6)
    print(f"cond_p {cases.case_id(case)}: err {err:.3e} (e32 {ref['e32']:.3e}, bar {bar:.3e}); residual {res:.3e} (f32 {ref['res32']:.3e}); "
          f"beta {float(beta.min()):.4g} .. {float(beta.max()):.4g}")
    assert err <= bar
    assert res <= 4 * ref["res32"]


def test_cond_p_one_point_past_the_lds_row(dev, lt):
    """N = DTS_LDS_ROW + 1: the plan itself puts the distances into the rows of P; three rows against float64 at the kernel's own
    beta, at the floor of test_cond_p (4e-6: D = 2 leaves the distances themselves exact to a few ulp).  The entropy bar is the
    search's tolerance of 1e-5 times four, as there; a row's f32 sum of 8193 terms is good to far better than 1e-5."""
    n, u = lt.LDS_ROW + 1, 30
    assert lt.plan(n - 1)["row_in_lds"] and not lt.plan(n)["row_in_lds"]
    X = 5.0 * torch.randn(n, 2, generator=torch.Generator().manual_seed(11))
    P, beta = _empty(dev, n, n), _empty(dev, n)
    lt.cond_p(X.to(dev), u, P, beta)
    sums = P.sum(1).cpu()
    assert float((sums - 1).abs().max()) <= 1e-5 and float(P.diagonal().abs().max()) == 0.0
    X64 = X.to(F64)
    for r in (0, n // 2, n - 1):
        d = cases.T.shifted_sq_distances(X64, r, r + 1)
        H, E, sp = cases.T.entropy_at(d, beta[r:r + 1].cpu().to(F64), r)
        row64 = (E / sp[:, None])[0]
        assert abs(float(H) - math.log(u)) <= 4e-5
        assert float((P[r].cpu().to(F64) - row64).abs().max() / row64.max()) <= 4e-6


# ---- dts_symmetrize ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_symmetrize(dev, lt, case):
    n = case[0]
    ref = cases.sym_reference(*case)
    P = ref["P"].to(dev).clone()
    lt.symmetrize(P, _empty(dev, lt.plan(n)["sym_groups"]))
    P = P.cpu()
    err = cases.rel_max(P, ref["S64"])
    print(f"symmetrize {cases.case_id(case)}: err {err:.3e} (e32 {ref['e32']:.3e})")
    assert torch.equal(P, P.T)
    assert err <= 4 * ref["e32"]


# ---- dts_zsum, dts_gradient, KL ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ex", (4.0, 1.0))
@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_zsum_gradient_kl(dev, lt, case, ex):
    n = case[0]
    P, Y = cases.grad_state(*case)
    ref, plan = cases.grad_reference(*case, ex), lt.plan(n)
    Pd, Yd = P.to(dev), Y.to(dev)
    zpart, klpart, dY, z_out, kl_out = (_empty(dev, k) for k in (plan["z_parts"], plan["grad_groups"], 2 * n, 1, 1))
    dY = dY.view(n, 2)
    lt.zsum(Yd, zpart)
    lt.gradient(Pd, Yd, ex, zpart, dY, klpart, z_out)
    plain = _empty(dev, n, 2)
    lt.gradient(Pd, Yd, ex, zpart, plain)                                               # without the KL partials: the same dY
    scratch = [torch.zeros(n, 2, device=dev) for _ in range(3)]
    lt.update(dY.clone(), *scratch, 0.5, _empty(dev, 2 * plan["upd_groups"]), klpart, kl_out)
    assert torch.equal(Yd.cpu(), Y), "dts_zsum / dts_gradient wrote to Y"
    e_dY = cases.rel_max(dY, ref["dY"])
    e_Z, e_KL = abs(float(z_out) - ref["Z"]) / abs(ref["Z"]), abs(float(kl_out) - ref["KL"]) / abs(ref["KL"])
    fl = cases.floor(n)
    print(f"gradient {cases.case_id(case)} ex {ex}: dY {e_dY:.3e} (e32 {ref['e_dY']:.3e}); Z {e_Z:.3e} (e32 {ref['e_Z']:.3e}); "
          f"KL {e_KL:.3e} (e32 {ref['e_KL']:.3e}); floor {fl:.3e}")
    assert torch.equal(plain, dY)
    assert abs(float(zpart.double().sum()) - float(z_out)) <= 1e-6 * float(z_out)
    assert e_dY <= max(4 * ref["e_dY"], fl)
    assert e_Z <= max(4 * ref["e_Z"], fl)
    assert e_KL <= max(4 * ref["e_KL"], fl)


def test_zsum_gradient_past_one_column_chunk(dev, lt):
    """N = 1300: two column chunks and six row blocks, so dts_zsum skips the blocks below the diagonal and doubles their mirrors,
    and a gradient workgroup walks its rows in two steps; the same bars as above"""
    from mscs_amd.utils import tsne as T
    n = 1300
    g = torch.Generator().manual_seed(13)
    P = torch.rand(n, n, generator=g) ** 8
    P = T.symmetrize_(P.fill_diagonal_(0))
    Y = 3 * torch.randn(n, 2, generator=g)
    d64, z64, _ = T.gradient(P.to(F64), Y.to(F64), 1.0)
    d32, z32, _ = T.gradient(P, Y, 1.0)
    plan = lt.plan(n)
    assert plan["z_parts"] == 12
    zpart, dY, z_out = _empty(dev, plan["z_parts"]), _empty(dev, n, 2), _empty(dev, 1)
    lt.zsum(Y.to(dev), zpart)
    lt.gradient(P.to(dev), Y.to(dev), 1.0, zpart, dY, None, z_out)
    zp = zpart.cpu().view(6, 2)
    assert float(zp[4, 0]) == 0.0 and float(zp[5, 0]) == 0.0 and bool((zp[:4] > 0).all()) and bool((zp[4:, 1] > 0).all())
    e_Z, e_dY, fl = abs(float(z_out) - float(z64)) / float(z64), cases.rel_max(dY, d64), cases.floor(n)
    e32_Z, e32_dY = abs(float(z32) - float(z64)) / float(z64), cases.rel_max(d32, d64)
    print(f"N 1300: Z {e_Z:.3e} (e32 {e32_Z:.3e}); dY {e_dY:.3e} (e32 {e32_dY:.3e}); floor {fl:.3e}")
    assert e_Z <= max(4 * e32_Z, fl) and e_dY <= max(4 * e32_dY, fl)


# ---- dts_update --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mom", (0.5, 0.8))
@pytest.mark.parametrize("n", cases.NS + (700,))
def test_update(dev, lt, n, mom):
    ref = cases.update_reference(n, mom)
    dY, iY, gains, Y = (t.to(dev).clone() for t in cases.update_inputs(n))
    lt.update(dY, iY, gains, Y, mom, _empty(dev, 2 * lt.plan(n)["upd_groups"]))
    iY32, g32, Y32 = ref[F32]
    iY64, _, Y64 = ref[F64]
    assert torch.equal(gains.cpu(), g32), "gains differ from the float32 composition"
    assert bool(g32.min() == torch.tensor(0.01)) and bool((g32 > 1.0).any())                        # the clamp and the additive branch were taken
    e_iY, e_Y, fl = cases.rel_max(iY, iY64), cases.rel_max(Y, Y64), cases.floor(n)
    print(f"update N{n} mom {mom}: iY {e_iY:.3e} (e32 {ref['e_iY']:.3e}); Y {e_Y:.3e} (e32 {ref['e_Y']:.3e}); floor {fl:.3e}")
    assert e_iY <= max(4 * ref["e_iY"], fl)
    assert e_Y <= max(4 * ref["e_Y"], fl)
    assert float(Y.double().mean(0).abs().max()) <= 1e-6 * float(Y64.abs().max())


# ---- one whole iteration, determinism, outcome --------------------------------------------------------------------------------------
def _state_on(dev, st):
    return [st[k].to(F32).to(dev).clone() for k in ("P", "Y", "iY", "gains")]


def test_one_iteration_from_a_midrun_state(dev, lt):
    st, n = cases.midrun_state(), cases.CLUSTER_N
    P, Y, iY, gains = _state_on(dev, st)
    lt.run(P, Y, iY, gains, _empty(dev, n, 2), _empty(dev, lt.plan(n)["ws_floats"]), 30, 31)
    keep = st["dY64"].abs() >= 1e-4 * st["dY64"].abs().max()
    left_out = 1.0 - float(keep.float().mean())
    scale = float(st["Y64"].abs().max())
    err = float(((Y.cpu().to(F64) - st["Y64"]).abs() * keep).max()) / scale
    e32 = float(((st["Y32"].to(F64) - st["Y64"]).abs() * keep).max()) / scale
    print(f"iteration 30: err {err:.3e} (e32 {e32:.3e}, floor {cases.floor(n):.3e}); left out {left_out:.4f}")
    assert left_out <= 0.01
    assert err <= max(4 * e32, cases.floor(n))


def _run_clusters(dev, lt, n_iter):
    X, _ = cases.clusters()
    n = X.shape[0]
    plan = lt.plan(n)
    P, beta = _empty(dev, n, n), _empty(dev, n)
    lt.cond_p(X.to(dev), 30, P, beta)
    lt.symmetrize(P, _empty(dev, plan["sym_groups"]))
    from mscs_amd.utils.tsne import initial_embedding
    Y = initial_embedding(n, 0).to(dev)
    iY, gains, kl = torch.zeros_like(Y), torch.ones_like(Y), _empty(dev, n_iter // 10)
    lt.run(P, Y, iY, gains, _empty(dev, n, 2), _empty(dev, plan["ws_floats"]), 0, n_iter // 2, kl)
    lt.run(P, Y, iY, gains, _empty(dev, n, 2), _empty(dev, plan["ws_floats"]), n_iter // 2, n_iter, kl)
    return Y.cpu(), kl.cpu()


def test_sixty_iterations_twice_bitwise(dev, lt):
    (Y1, kl1), (Y2, kl2) = _run_clusters(dev, lt, 60), _run_clusters(dev, lt, 60)
    assert bool(torch.isfinite(Y1).all()) and bool(torch.isfinite(kl1).all())
    assert torch.equal(Y1, Y2) and torch.equal(kl1, kl2)


def test_outcome_on_the_clusters(dev, lt):
    from mscs_amd.utils import tsne_exact
    X, labels = cases.clusters()
    before = dict(lt.calls)
    Y, kl = tsne_exact(X.to(dev), 30, 250, 0)
    assert Y.is_cuda and Y.dtype == F32 and kl.shape == (25,)
    assert lt.calls["cond_p"] == before["cond_p"] + 1 and lt.calls["symmetrize"] == before["symmetrize"] + 1
    assert lt.calls["run"] == before["run"] + 1
    pur = cases.purity(Y, labels)
    print(f"outcome: KL(110) {float(kl[10]):.4f} KL(250) {float(kl[24]):.4f} purity {pur:.4f}")
    assert bool(torch.isfinite(Y).all()) and bool(torch.isfinite(kl).all())
    assert float(kl[24]) < float(kl[10])
    assert pur >= 0.98


# ---- path selection ----------------------------------------------------------------------------------------------------------------
def test_path_selection(dev, lt, monkeypatch):
    from mscs_amd.utils import tsne as T
    X, _ = cases.clusters()
    X = X[:64].to(dev)
    before = dict(lt.calls)
    Y64, _ = T.tsne_exact(X.double(), 10, 10, 0)                                         # float64: the composition, on the GPU
    assert Y64.dtype == F64 and Y64.is_cuda and lt.calls == before
    monkeypatch.setattr(T._dbg, "tsne_hip", False)                                       # DCL_TSNE_HIP=0
    Y0, _ = T.tsne_exact(X, 10, 10, 0)
    assert lt.calls == before and Y0.dtype == F32
    monkeypatch.setattr(T._dbg, "tsne_hip", True)
    with pytest.raises(ValueError, match="perplexity"):
        T.tsne_exact(X, 63, 10, 0)                                                       # N - 1 <= perplexity
    assert lt.calls == before
    Y1, _ = T.tsne_exact(X, 10, 10, 0)
    assert lt.calls["run"] == before["run"] + 1
    assert all(bool(torch.isfinite(t).all()) for t in (Y0, Y1, Y64))                    # (the trajectories part: nothing is compared)
    W = torch.randn(64, 80, generator=torch.Generator().manual_seed(2)).to(dev)          # D > 50: the PCA, then the kernels
    T.tsne_exact(W, 10, 10, 0)
    assert lt.calls["run"] == before["run"] + 2


# ---- the manager -------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_demo_tsne_on_the_gpu(dev, lt, tmp_path):
    import os
    before = lt.calls["run"]
    md, Y, png = cases.run_demo(tmp_path, cuda=True)
    assert os.path.exists(png) and os.path.exists(png[:-4] + ".npz")
    z = np.load(png[:-4] + ".npz")
    assert z["Y"].shape == (len(z["labels"]), 2) and np.isfinite(z["Y"]).all() and np.array_equal(z["Y"], Y)
    assert z["kl"].shape == (2,) and np.isfinite(z["kl"]).all() and int(z["counts"].sum()) == len(z["labels"]) > 7
    assert lt.calls["run"] > before
