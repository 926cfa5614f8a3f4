"""What a kernel touches besides its result, and the absmax tags it hands on.

Every entry point of include/dcl_hip.h that launches device work is called straight at the C ABI with EVERY pointer argument in
the middle of a larger allocation (tests/_footprint.py).  Each case checks
  (i)   bands: nothing outside an output, workspace, ticket or absmax buffer was written;
  (ii)  body: no sentinel is left in an output; workspaces have exactly the size their size function returned;
  (iii) fill independence: the outputs are finite and bitwise equal whether NaN or 1e30 lies next to the inputs;
  (iv)  values: the float64 bar of the kernel's own parity test (the constant is quoted beside each use);
and, for every entry that writes an absmax tag, that the tag EQUALS the true maximum of the tensor bit for bit (a tag that is too
small overflows the f16 split of the consumer, one that is too large gives away mantissa bits).
``COVERED`` / ``EXEMPT`` are read by tests/test_host_logic.py: a new entry point needs a case here."""
import math

import pytest
import torch
import torch.nn.functional as F

from _footprint import NAN_BITS, SENTINEL, all_sentinel, run_both

pytestmark = pytest.mark.gpu

COVERED = (
    "dcl_conv3x3_pack", "dcl_conv3x3_f16x3", "dcl_conv1x1_f16x3", "dcl_conv3x3_s2_smallcin", "dcl_conv3x3_pre_f16x3",
    "dcl_conv3x3_pack_multi",
    "dcl_wgrad3x3_f16x3", "dcl_wgrad1x1_f16x3", "dcl_wgrad3x3_s2_smallcin", "dcl_wgrad3x3_pre_f16x3",
    "dcl_bn_stats", "dcl_bn_finalize", "dcl_bn_apply", "dcl_bn_stats_finalize", "dcl_bn_bwd_reduce", "dcl_bn_bwd_apply",
    "dcl_bn_stats_part", "dcl_bn_apply_fused", "dcl_bn_apply_parts", "dcl_bn_bwd_reduce_part", "dcl_bn_bwd_apply_fused",
    "dcl_bn_stats_minmax_part", "dcl_bn_finalize_pre", "dcl_bn_stats_pre",
    "dcl_upsample_bilinear_fwd", "dcl_upsample_bilinear_bwd", "dcl_upsample_bilinear_fwd_slice", "dcl_upsample_bilinear_bwd_slice",
    "dcl_gemm_f16x3", "dcl_gemm_f16x3_ep", "dcl_gemm_f16x3_ascaled",
    "dcl_layernorm_fwd", "dcl_layernorm_bwd",
    "dcl_add_n", "dcl_absmax", "dcl_absmax_multi", "dcl_amax_sum2",
    "dcl_confusion_matrix", "dcl_confusion_matrix_pred", "dcl_metrics_from_cm",
    "dcl_label_hist", "dcl_rank_select", "dcl_gather_raw", "dcl_scatter_raw", "dcl_gather_normalize",
    "dcl_winattn_fwd", "dcl_winattn_bwd",
    "dcl_upsample_ce_fwd", "dcl_upsample_ce_bwd", "dcl_head_norm_dz", "dcl_tapup_fwd", "dcl_tapup_bwd", "dcl_tapup_bwd_amax",
    "dcl_infonce_fwd", "dcl_infonce_zsweep", "dcl_infonce_possweep", "dcl_infonce_loss", "dcl_infonce_zsweep_keep",
    "dcl_infonce_pos_finish", "dcl_infonce_prep_stats", "dcl_infonce_bwd", "dcl_infonce_bwd_streamk", "dcl_normalize_bwd_scatter",
)

_HOST = "host only: no device work"
EXEMPT = {
    **{n: _HOST + " (a switch read by later launches)" for n in (
        "dcl_infonce_set_streamk_slices", "dcl_infonce_set_streamk", "dcl_infonce_set_streamk_timeout_ms", "dcl_tapup_set_bwd_form",
        "dcl_gemm_set_tile", "dcl_wgrad3x3_set_stride2", "dcl_wgrad3x3_set_splits", "dcl_wgrad3x3_set_workgroup_target",
        "dcl_wgrad3x3_set_wave_mode", "dcl_wgrad3x3_set_strip_group", "dcl_wgrad3x3_set_wave_band", "dcl_conv3x3_set_up2_phases",
        "dcl_conv3x3_set_min_workgroups", "dcl_conv3x3_set_interleave", "dcl_upsample_ce_set_bwd_chunk", "dcl_upsample_ce_set_fwd_lds",
        "dcl_wgrad3x3_set_tile", "dcl_wgrad3x3_set_variant", "dcl_winattn_set_mfma")},
    **{n: _HOST + " (a support query)" for n in (
        "dcl_conv3x3_pre_supported", "dcl_wgrad3x3_pre_supported", "dcl_tapup_supported", "dcl_gemm_supported",
        "dcl_layernorm_supported")},
    **{n: _HOST + " (a size or plan query)" for n in (
        "dcl_infonce_bwd_streamk_workgroups", "dcl_infonce_bwd_streamk_slabs", "dcl_bn_num_slices", "dcl_wgrad3x3_s2_smallcin_workspace",
        "dcl_gemm_workspace_floats", "dcl_gemm_suggest_splitk", "dcl_wgrad1x1_splits", "dcl_wgrad3x3_splits", "dcl_winattn_npad",
        "dcl_winattn_bwd_waves", "dcl_layernorm_bwd_parts", "dcl_suggest_nsplit")},
    "dcl_version": _HOST,
    "dcl_trace_kernels": _HOST,
    "dcl_host_randperm_select": _HOST + " (host pointers throughout; its last pointer is the result array sel_host, not a stream)",
}

SLOTS = 64            # DCL_AMAX_SLOTS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _lib_():
    from mscs_amd import _lib
    return _lib, _lib.lib()


def _p(t):
    return None if t is None else t.data_ptr()


def _rel(got, want):
    return ((got.double() - want.double()).abs().max() / want.double().abs().max()).item()


def _same_bits(a, b):
    return torch.equal(a.reshape(1).view(torch.int32), b.reshape(1).view(torch.int32))


def _tag_in(ar, t, count=1):
    """the absmax tag a producer would have left for ``t``: ``count`` floats whose maximum is max|t| exactly"""
    m = t.abs().max().reshape(1)
    if count == 1:
        return ar.inp(m), 1
    v = torch.rand(count, device=t.device) * m
    v[41 % count] = m
    return ar.inp(v), count


def _tag_exact(buf, out, what):
    """section C: the emitted tag equals the true maximum bit for bit"""
    got, want = buf.max(), out.abs().max()
    assert _same_bits(got, want), (what, "absmax tag", got.item(), "true maximum", want.item(), "ratio", (got / want).item())


def _plant(t, where, big=37.0):
    """moves the maximum of |t| to the first element, the last element (of a ragged tail), or onto a negative value"""
    f = t.reshape(-1)
    m = f.abs().max() * 1.5 + big
    if where == "first":
        f[0] = m
    elif where == "last":
        f[-1] = m
    elif where == "neg":
        f[f.numel() // 2] = -m
    return t


# ---------------------------------------------------------------------------------------------------------------------------------
# 3x3 / 1x1 convolution

def _pack_bytes(m, k, taps):
    return ((m + 31) // 32) * ((k + 15) // 16) * taps * 2 * 64 * 16


def _conv_run(dev, x, wt, want, *, transposed=False, stride=1, in_up=1, out_hw=None, addend=None, bias=None, tile=(0, 0),
              xcount=1, taps=9, tol=3e-6, what=""):
    """pack + convolution, every pointer guarded; ``want`` float64 (None: the result must be exactly zero)"""
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    co, ci = wt.shape[0], wt.shape[1]
    m, k = (ci, co) if transposed else (co, ci)
    n, cin, h, w = x.shape
    assert cin == k
    oh, ow = out_hw if out_hw else (((h - 1) // stride + 1, (w - 1) // stride + 1))

    def body(ar):
        xg, wg = ar.inp(x, "x"), ar.inp(wt, "w")
        wam, _ = _tag_in(ar, wt)
        wp = ar.out(_pack_bytes(m, k, taps), torch.uint8, "wp")
        _lib.check(L.dcl_conv3x3_pack(_p(wg), m, k, (1 if transposed else 0) | (2 if taps == 1 else 0), _p(wam), _p(wp), st), "pack")
        xam, xc = _tag_in(ar, x, xcount)
        y = ar.out((n, m, oh, ow), name="y")
        ad = ar.inp(addend, "addend") if addend is not None else None
        b = ar.inp(bias, "bias") if bias is not None else None
        if taps == 1:
            _lib.check(L.dcl_conv1x1_f16x3(_p(xg), n, cin, h, w, _p(wp), m, _p(xam), xc, _p(wam), _p(ad), _p(b), _p(y),
                                           tile[0], tile[1], st), "dcl_conv1x1_f16x3")
        else:
            _lib.check(L.dcl_conv3x3_f16x3(_p(xg), n, cin, h, w, _p(wp), m, _p(xam), xc, _p(wam), _p(ad), _p(b), _p(y), stride, in_up,
                                           oh, ow, tile[0], tile[1], st), "dcl_conv3x3_f16x3")
        return {"wp": wp, "y": y}
    got = run_both(dev, body, what)
    if want is None:
        assert bool((got["y"] == 0).all()), (what, "an all-zero operand must give an exactly-zero result")
    else:
        err = _rel(got["y"], want)
        assert err < tol, (what, err)          # 3e-6 of max: test_direct_conv3x3_forward_dgrad_match_fp64
    return got


def _conv_data(shape, dev, seed):
    n, ci, co, h, w = shape
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(n, ci, h, w, device=dev, generator=g).relu_() * 2.5
    wt = torch.randn(co, ci, 3, 3, device=dev, generator=g) * (2.0 / (9 * ci)) ** 0.5
    return x, wt, g


@pytest.mark.parametrize("shape", [(2, 40, 24, 19, 33), (1, 16, 16, 1, 8), (1, 48, 96, 20, 33)], ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_stride1_footprint(dev, shape):
    """dcl_conv3x3_pack + dcl_conv3x3_f16x3, stride 1: automatic, (1, 4) and (3, 4) tiles, the three staging forms, with and
    without addend and bias, the operand tag as 1 and as 64 partial maxima."""
    _lib, L = _lib_()
    n, ci, co, h, w = shape
    x, wt, g = _conv_data(shape, dev, sum(shape))
    addend = torch.randn(n, co, h, w, device=dev, generator=g)
    bias = torch.randn(co, device=dev, generator=g)
    ref = F.conv2d(x.double(), wt.double(), padding=1)
    ref_ab = ref + addend.double() + bias.double().view(1, -1, 1, 1)
    try:
        for il in (2, 1, 0):
            L.dcl_conv3x3_set_interleave(il)
            for tile in ((0, 0), (1, 4), (3, 4)):
                _conv_run(dev, x, wt, ref, tile=tile, xcount=1, what=("plain", shape, il, tile))
                _conv_run(dev, x, wt, ref_ab, tile=tile, addend=addend, bias=bias, xcount=SLOTS, what=("addend+bias", shape, il, tile))
    finally:
        L.dcl_conv3x3_set_interleave(2)
    # the data gradient: transposed, tap-flipped fragments of the same weights
    gy = torch.randn(n, co, h, w, device=dev, generator=g) * 3e-5
    gref = F.conv_transpose2d(gy.double(), wt.double(), padding=1)
    _conv_run(dev, gy, wt, gref, transposed=True, what=("dgrad", shape))
    _conv_run(dev, torch.zeros_like(x), wt, None, what=("zero x", shape))
    _conv_run(dev, x, torch.zeros_like(wt), None, what=("zero w", shape))


@pytest.mark.parametrize("shape", [(1, 16, 32, 7, 40), (1, 48, 96, 9, 24)], ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_stride2_and_its_data_gradient_footprint(dev, shape):
    """dcl_conv3x3_f16x3 with stride 2, and in_up = 2 (the data gradient of that convolution) in its three forms."""
    _lib, L = _lib_()
    n, ci, co, h, w = shape
    x, wt, g = _conv_data(shape, dev, sum(shape) + 1)
    bias = torch.randn(co, device=dev, generator=g)
    ref = F.conv2d(x.double(), wt.double(), stride=2, padding=1)
    _conv_run(dev, x, wt, ref, stride=2, what=("s2", shape))
    _conv_run(dev, x, wt, ref + bias.double().view(1, -1, 1, 1), stride=2, bias=bias, xcount=SLOTS, what=("s2 bias", shape))
    ho, wo = ref.shape[2:]
    gy = torch.randn(n, co, ho, wo, device=dev, generator=g) * 3e-5
    addend = torch.randn(n, ci, h, w, device=dev, generator=g) * 1e-5
    gref = F.conv_transpose2d(gy.double(), wt.double(), stride=2, padding=1,
                              output_padding=(h - ((ho - 1) * 2 + 1), w - ((wo - 1) * 2 + 1)))
    try:
        for ph in (2, 1, 0):
            L.dcl_conv3x3_set_up2_phases(ph)
            _conv_run(dev, gy, wt, gref, transposed=True, in_up=2, out_hw=(h, w), what=("up2", shape, ph))
            _conv_run(dev, gy, wt, gref + addend.double(), transposed=True, in_up=2, out_hw=(h, w), addend=addend, xcount=SLOTS,
                      what=("up2 addend", shape, ph))
    finally:
        L.dcl_conv3x3_set_up2_phases(2)
    _conv_run(dev, torch.zeros_like(gy), wt, None, transposed=True, in_up=2, out_hw=(h, w), what=("up2 zero", shape))


@pytest.mark.parametrize("shape", [(2, 40, 24, 19, 33), (1, 48, 96, 5, 8)], ids=lambda s: "x".join(map(str, s)))
def test_conv1x1_footprint(dev, shape):
    """dcl_conv1x1_f16x3 (one-tap mode of the tile kernel): forward with addend and bias, data gradient."""
    n, ci, co, h, w = shape
    g = torch.Generator(device=dev).manual_seed(sum(shape) + 3)
    x = torch.randn(n, ci, h, w, device=dev, generator=g).relu_() * 1.5
    wt = torch.randn(co, ci, 1, 1, device=dev, generator=g) * (2.0 / ci) ** 0.5
    addend = torch.randn(n, co, h, w, device=dev, generator=g)
    bias = torch.randn(co, device=dev, generator=g)
    ref = F.conv2d(x.double(), wt.double())
    for tile in ((0, 0), (1, 4), (3, 4)):
        _conv_run(dev, x, wt, ref, taps=1, tile=tile, what=("1x1", shape, tile))      # 3e-6: test_direct_conv1x1_matches_fp64
    _conv_run(dev, x, wt, ref + addend.double() + bias.double().view(1, -1, 1, 1), taps=1, addend=addend, bias=bias, xcount=SLOTS,
              what=("1x1 addend+bias", shape))
    gy = torch.randn(n, co, h, w, device=dev, generator=g) * 2e-4
    _conv_run(dev, gy, wt, F.conv_transpose2d(gy.double(), wt.double()), taps=1, transposed=True, what=("1x1 dgrad", shape))


def test_small_cin_stem_footprint(dev):
    """dcl_conv3x3_s2_smallcin and dcl_wgrad3x3_s2_smallcin at (2, 3, 64, 9, 7)."""
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    n, ci, co, h, w = 2, 3, 64, 9, 7
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(n, ci, h, w, device=dev, generator=g)
    wt = torch.randn(co, ci, 3, 3, device=dev, generator=g) * 0.2
    bias = torch.randn(co, device=dev, generator=g)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    gy = torch.randn(n, co, ho, wo, device=dev, generator=g)
    for b in (None, bias):
        def body(ar):
            y = ar.out((n, co, ho, wo), name="y")
            _lib.check(L.dcl_conv3x3_s2_smallcin(_p(ar.inp(x)), n, ci, h, w, _p(ar.inp(wt)), co, _p(ar.inp(b)) if b is not None else None,
                                                 _p(y), st), "dcl_conv3x3_s2_smallcin")
            return {"y": y}
        got = run_both(dev, body, ("smallcin", b is not None))
        ref = F.conv2d(x.double(), wt.double(), None if b is None else b.double(), 2, 1)
        assert _rel(got["y"], ref) <= 2e-6                  # test_stem_small_cin_stride2_convolution_against_fp64
    nws = L.dcl_wgrad3x3_s2_smallcin_workspace(co)
    assert nws > 0

    def body(ar):
        part, dw = ar.out(nws, name="part"), ar.out((co, ci, 3, 3), name="dw")
        _lib.check(L.dcl_wgrad3x3_s2_smallcin(_p(ar.inp(x)), n, ci, h, w, _p(ar.inp(gy)), co, _p(part), _p(dw), st),
                   "dcl_wgrad3x3_s2_smallcin")
        return {"dw": dw}
    got = run_both(dev, body, "smallcin wgrad")
    ref = torch.ops.aten.convolution_backward(gy.double(), x.double(), wt.double(), None, [2, 2], [1, 1], [1, 1], False, [0, 0], 1,
                                              [False, True, False])[1]
    assert _rel(got["dw"], ref) < 2e-6                      # test_stem_weight_gradient_matches_fp64_and_is_reproducible


def test_conv3x3_pack_multi_footprint(dev):
    """dcl_absmax_multi + dcl_conv3x3_pack_multi: three weights of ragged sizes in one launch each; every job's absmax is its
    own guarded float, every fragment buffer its own guarded allocation; bitwise the single-tensor calls."""
    import numpy as np
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(9)
    ws = [torch.randn(24, 40, 3, 3, device=dev, generator=g), torch.randn(16, 16, 1, 1, device=dev, generator=g) * 3,
          torch.randn(96, 48, 3, 3, device=dev, generator=g) * 0.01]
    _plant(ws[0], "last"), _plant(ws[1], "first"), _plant(ws[2], "neg")

    def body(ar):
        absjobs = np.zeros(len(ws), dtype=[("x", "<u8"), ("out", "<u8"), ("n", "<i8"), ("fb", "<i4"), ("pad", "<i4")])
        packjobs = np.zeros(2 * len(ws), dtype=[("w", "<u8"), ("wp", "<u8"), ("amax", "<u8"), ("M", "<i4"), ("K", "<i4"),
                                                ("tr", "<i4"), ("fb", "<i4")])
        ab2j, pb2j, outs, ams = [], [], {}, []
        for i, w in enumerate(ws):
            wg, am = ar.inp(w), ar.zeros(1, name=f"amax{i}")
            ams.append(am)
            absjobs[i] = (wg.data_ptr(), am.data_ptr(), w.numel(), len(ab2j), 0)
            ab2j += [i] * ((w.numel() + 4095) // 4096)
            co, ci, taps = w.shape[0], w.shape[1], w.shape[2] * w.shape[3]
            for tr in (0, 1):
                mm, kk = (ci, co) if tr else (co, ci)
                frags = ((mm + 31) // 32) * ((kk + 15) // 16) * taps
                buf = ar.out(frags * 2048, torch.uint8, f"wp{i}{tr}")
                packjobs[2 * i + tr] = (wg.data_ptr(), buf.data_ptr(), am.data_ptr(), mm, kk, tr | (2 if taps == 1 else 0), len(pb2j))
                pb2j += [2 * i + tr] * ((frags * 64 + 255) // 256)
                outs[f"wp{i}{tr}"] = buf
        to_dev = lambda a: ar.inp(torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev))
        aj, pj = to_dev(absjobs), to_dev(packjobs)
        ab, pb = ar.inp(torch.tensor(ab2j, dtype=torch.int32, device=dev)), ar.inp(torch.tensor(pb2j, dtype=torch.int32, device=dev))
        _lib.check(L.dcl_absmax_multi(_p(aj), _p(ab), len(ab2j), st), "dcl_absmax_multi")
        _lib.check(L.dcl_conv3x3_pack_multi(_p(pj), _p(pb), len(pb2j), st), "dcl_conv3x3_pack_multi")
        for i, w in enumerate(ws):
            assert _same_bits(ams[i], w.abs().max()), ("dcl_absmax_multi job", i, ams[i].item(), w.abs().max().item())
            outs[f"amax{i}"] = ams[i]
        return outs
    got = run_both(dev, body, "pack_multi")
    for i, w in enumerate(ws):
        co, ci, taps = w.shape[0], w.shape[1], w.shape[2] * w.shape[3]
        for tr in (0, 1):
            mm, kk = (ci, co) if tr else (co, ci)
            def sbody(ar):
                single = ar.out(_pack_bytes(mm, kk, taps), torch.uint8, "wp")
                _lib.check(L.dcl_conv3x3_pack(_p(ar.inp(w, "w")), mm, kk, tr | (2 if taps == 1 else 0), _p(_tag_in(ar, w)[0]), _p(single), st),
                           "dcl_conv3x3_pack")
                return {"wp": single}
            assert torch.equal(run_both(dev, sbody, ("single pack", i, tr))["wp"], got[f"wp{i}{tr}"]), (i, tr)


# ---------------------------------------------------------------------------------------------------------------------------------
# weight gradients

def _wgrad_run(dev, x, gy, want, stride, k, tol, what, pre=None, counts=(1, SLOTS)):
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    n, ci, h, w = x.shape
    co = gy.shape[1]
    splits = L.dcl_wgrad3x3_splits(n, ci, co, h, w, stride) if k == 3 else L.dcl_wgrad1x1_splits(n, ci, co, h, w)
    assert splits > 0, (what, "unsupported")

    def body(ar):
        part = ar.out(splits * k * k * co * ci, name="slabs")       # sized by the *_splits function alone
        dw = ar.out((co, ci, k, k), name="dw")
        xg, gg = ar.inp(x, "x"), ar.inp(gy, "dy")
        if pre is not None:
            sc, sh, mapped = pre
            xam, xc = _tag_in(ar, mapped, counts[0])
            gam, gc = _tag_in(ar, gy, counts[1])
            _lib.check(L.dcl_wgrad3x3_pre_f16x3(_p(xg), _p(gg), n, ci, co, h, w, _p(xam), xc, _p(gam), gc, _p(ar.inp(sc)), _p(ar.inp(sh)),
                                                stride, _p(part), _p(dw), st), "dcl_wgrad3x3_pre_f16x3")
            return {"dw": dw}
        xam, xc = _tag_in(ar, x, counts[0])
        gam, gc = _tag_in(ar, gy, counts[1])
        if k == 3:
            _lib.check(L.dcl_wgrad3x3_f16x3(_p(xg), _p(gg), n, ci, co, h, w, _p(xam), xc, _p(gam), gc, stride, _p(part), _p(dw), st),
                       "dcl_wgrad3x3_f16x3")
        else:
            _lib.check(L.dcl_wgrad1x1_f16x3(_p(xg), _p(gg), n, ci, co, h, w, _p(xam), xc, _p(gam), gc, _p(part), _p(dw), st),
                       "dcl_wgrad1x1_f16x3")
        return {"dw": dw}
    got = run_both(dev, body, (what, "splits", splits))
    if want is None:
        assert bool((got["dw"] == 0).all()), (what, "an all-zero operand must give an exactly-zero result")
    else:
        err = _rel(got["dw"], want)
        assert err < tol, (what, splits, err)
    return got["dw"]


def _wgrad_ref(x, gy, stride, k):
    co, ci = gy.shape[1], x.shape[1]
    return torch.ops.aten.convolution_backward(gy.double(), x.double(), torch.zeros(co, ci, k, k, device=x.device, dtype=torch.float64),
                                               None, [stride, stride], [k // 2, k // 2], [1, 1], False, [0, 0], 1,
                                               [False, True, False])[1]


@pytest.mark.parametrize("shape,stride", [((2, 48, 48, 20, 48), 1), ((1, 16, 32, 7, 40), 1), ((1, 32, 96, 7, 16), 2)],
                         ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else f"s{s}")
def test_wgrad3x3_footprint(dev, shape, stride):
    """dcl_wgrad3x3_f16x3: both kernel variants, wave mode and strip grouping on and off, one forced split and the planned count,
    the three stride-2 forms; the slab workspace has exactly dcl_wgrad3x3_splits(...) slabs under each of these switches (the
    tile, wave-band and workgroup-target hooks stay at their defaults)."""
    _lib, L = _lib_()
    n, ci, co, h, w = shape
    g = torch.Generator(device=dev).manual_seed(sum(shape) + 1)
    x = torch.randn(n, ci, h, w, device=dev, generator=g).relu_() * 2.5
    ho, wo = ((h - 1) // 2 + 1, w // 2) if stride == 2 else (h, w)
    gy = torch.randn(n, co, ho, wo, device=dev, generator=g) * 3e-5
    ref = _wgrad_ref(x, gy, stride, 3)
    tol = 3e-6 if stride == 1 else 2e-6     # test_direct_conv3x3_wgrad_matches_fp64 / test_stride2_weight_gradient_lds_dma_form_...
    try:
        for variant in (2, 0):
            L.dcl_wgrad3x3_set_variant(variant)
            for wave in (2, 0):
                L.dcl_wgrad3x3_set_wave_mode(wave)
                for strip in (1, 0):
                    L.dcl_wgrad3x3_set_strip_group(strip)
                    for forced in (0, 1):
                        L.dcl_wgrad3x3_set_splits(forced)
                        _wgrad_run(dev, x, gy, ref, stride, 3, tol, ("wgrad3x3", shape, stride, variant, wave, strip, forced))
        L.dcl_wgrad3x3_set_variant(-1), L.dcl_wgrad3x3_set_wave_mode(2), L.dcl_wgrad3x3_set_strip_group(1), L.dcl_wgrad3x3_set_splits(0)
        if stride == 2:
            for native in (2, 0):
                L.dcl_wgrad3x3_set_stride2(native)
                _wgrad_run(dev, x, gy, ref, stride, 3, tol, ("wgrad3x3 stride-2 form", shape, native))
            L.dcl_wgrad3x3_set_stride2(1)
        _wgrad_run(dev, torch.zeros_like(x), gy, None, stride, 3, tol, ("wgrad3x3 zero x", shape))
        _wgrad_run(dev, x, torch.zeros_like(gy), None, stride, 3, tol, ("wgrad3x3 zero dy", shape))
    finally:
        L.dcl_wgrad3x3_set_variant(-1), L.dcl_wgrad3x3_set_wave_mode(2), L.dcl_wgrad3x3_set_strip_group(1), L.dcl_wgrad3x3_set_splits(0)
        L.dcl_wgrad3x3_set_stride2(1)


@pytest.mark.parametrize("shape", [(2, 48, 48, 20, 48), (1, 16, 32, 7, 40)], ids=lambda s: "x".join(map(str, s)))
def test_wgrad1x1_footprint(dev, shape):
    """dcl_wgrad1x1_f16x3, slabs sized by dcl_wgrad1x1_splits."""
    n, ci, co, h, w = shape
    g = torch.Generator(device=dev).manual_seed(sum(shape) + 2)
    x = torch.randn(n, ci, h, w, device=dev, generator=g).relu_() * 1.5
    gy = torch.randn(n, co, h, w, device=dev, generator=g) * 2e-4
    ref = torch.einsum("nohw,nihw->oi", gy.double(), x.double()).view(co, ci, 1, 1)
    _wgrad_run(dev, x, gy, ref, 1, 1, 3e-6, ("wgrad1x1", shape))                  # test_direct_conv1x1_matches_fp64
    _wgrad_run(dev, x, gy, ref, 1, 1, 3e-6, ("wgrad1x1 tags 64/1", shape), counts=(SLOTS, 1))
    _wgrad_run(dev, torch.zeros_like(x), gy, None, 1, 1, 3e-6, ("wgrad1x1 zero x", shape))


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm

_BN_EPS, _BN_MOM = 1e-5, 0.1


def _bn_close(got, want, what):
    scale = max(want.abs().max().item(), 1e-6)
    err = (got.double() - want.double()).abs().max().item()
    assert err <= 2e-5 * scale + 1e-6, (what, err, scale)           # test_fused_batchnorm_matches_fp64_reference


def _bn_ref(x, res, gamma, beta, rm, rv, relu, dy, xmask=False):
    """float64 training-mode norm (+ residual) (+ ReLU) and its gradients"""
    xd = x.double().requires_grad_(True)
    rd = res.double().requires_grad_(True) if res is not None else None
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm2, rv2 = rm.double().clone(), rv.double().clone()
    y = F.batch_norm(xd, rm2, rv2, gd, bd, True, _BN_MOM, _BN_EPS)
    if rd is not None:
        y = y + rd
    if relu:
        y = torch.relu(y)
    y.backward(dy.double())
    mean = x.double().mean((0, 2, 3))
    invstd = 1.0 / torch.sqrt(x.double().var((0, 2, 3), unbiased=False) + _BN_EPS)
    dx = xd.grad * (x > 0) if xmask else xd.grad
    return dict(y=y.detach(), dx=dx, dres=rd.grad if rd is not None else None, dgamma=gd.grad, dbeta=bd.grad, rm=rm2, rv=rv2,
                mean=mean, invstd=invstd)


def _bn_data(shape, dev, where, seed=3):
    n, c, h, w = shape
    g = torch.Generator(device=dev).manual_seed(seed + sum(shape))
    x = torch.randn(shape, device=dev, generator=g) * 2 + 0.7
    _plant(x, where, big=9.0)
    return dict(x=x, res=torch.randn(shape, device=dev, generator=g), dy=torch.randn(shape, device=dev, generator=g),
                gamma=torch.rand(c, device=dev, generator=g) + 0.5, beta=torch.rand(c, device=dev, generator=g) - 0.5,
                rm=torch.randn(c, device=dev, generator=g), rv=torch.rand(c, device=dev, generator=g) * 1.5 + 0.5)


_BN_SHAPES = [((5, 7, 5, 3), "first"), ((3, 48, 33, 47), "last"), ((2, 16, 16, 16), "neg")]


@pytest.mark.parametrize("shape,where", _BN_SHAPES, ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))
@pytest.mark.parametrize("relu,use_res", [(0, False), (1, False), (1, True), (0, True)])
def test_bn_plain_entries_footprint(dev, shape, where, relu, use_res):
    """dcl_bn_stats -> dcl_bn_finalize -> dcl_bn_apply -> dcl_bn_bwd_reduce -> dcl_bn_bwd_apply, and dcl_bn_stats_finalize: part
    sized by dcl_bn_num_slices, the absmax buffers exactly 64 floats, both tags exact."""
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    n, c, h, w = shape
    hw = h * w
    d = _bn_data(shape, dev, where)
    res = d["res"] if use_res else None
    ref = _bn_ref(d["x"], res, d["gamma"], d["beta"], d["rm"], d["rv"], relu, d["dy"])
    ns = L.dcl_bn_num_slices(n, c)
    count = float(n * hw)

    def body(ar):
        x, dy, gamma, beta = ar.inp(d["x"], "x"), ar.inp(d["dy"], "dy"), ar.inp(d["gamma"]), ar.inp(d["beta"])
        r = ar.inp(res, "res") if use_res else None
        part, sums = ar.out(c * ns * 2, name="part"), ar.out((c, 2), name="sums")
        _lib.check(L.dcl_bn_stats(_p(x), n, c, hw, _p(part), _p(sums), st), "dcl_bn_stats")
        mean, invstd = ar.out(c, name="mean"), ar.out(c, name="invstd")
        rm, rv = ar.io(d["rm"], "running_mean"), ar.io(d["rv"], "running_var")
        _lib.check(L.dcl_bn_finalize(_p(sums), c, count, _BN_EPS, _BN_MOM, _p(mean), _p(invstd), _p(rm), _p(rv), st), "dcl_bn_finalize")
        y, amax = ar.out(shape, name="y"), ar.zeros(SLOTS, name="amax y")
        _lib.check(L.dcl_bn_apply(_p(x), _p(r), _p(mean), _p(invstd), _p(gamma), _p(beta), n, c, hw, relu, _p(y), _p(amax), st),
                   "dcl_bn_apply")
        _tag_exact(amax, y, ("dcl_bn_apply", shape, relu, use_res))
        # the single-rank form of the first two calls
        part2, sums2, mean2, invstd2 = ar.out(c * ns * 2, name="part2"), ar.out((c, 2)), ar.out(c), ar.out(c)
        rm2, rv2, nbt = ar.io(d["rm"]), ar.io(d["rv"]), ar.io(torch.full((1,), 6, dtype=torch.int64, device=dev), "nbt")
        _lib.check(L.dcl_bn_stats_finalize(_p(x), n, c, hw, _BN_EPS, _BN_MOM, _p(part2), _p(sums2), _p(mean2), _p(invstd2), _p(rm2),
                                           _p(rv2), _p(nbt), st), "dcl_bn_stats_finalize")
        assert nbt.item() == 7
        # backward; y may be NULL with relu and no residual (the mask is recomputed)
        for ygiven in ((True, False) if (relu and not use_res) else (True,)):
            part3, bsums = ar.out(c * ns * 2, name="part3"), ar.out((c, 2), name="bwd sums")
            dbeta, dgamma = ar.out(c, name="dbeta"), ar.out(c, name="dgamma")
            yin = ar.inp(y) if ygiven else None
            _lib.check(L.dcl_bn_bwd_reduce(_p(dy), _p(x), _p(yin), _p(mean), _p(invstd), _p(gamma), _p(beta), n, c, hw, relu, _p(part3),
                                           _p(bsums), _p(dbeta), _p(dgamma), st), "dcl_bn_bwd_reduce")
            dx, dres, amax2 = ar.out(shape, name="dx"), (ar.out(shape, name="dres") if use_res else None), ar.zeros(SLOTS, name="amax dx")
            _lib.check(L.dcl_bn_bwd_apply(_p(dy), _p(x), _p(yin), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(bsums), count, n, c, hw,
                                          relu, _p(dx), _p(dres), _p(amax2), st), "dcl_bn_bwd_apply")
            _tag_exact(amax2, dx, ("dcl_bn_bwd_apply", shape, relu, use_res, ygiven))
        outs = dict(sums=sums, mean=mean, invstd=invstd, rm=rm, rv=rv, y=y, amax=amax, mean2=mean2, invstd2=invstd2, rm2=rm2, rv2=rv2,
                    sums2=sums2, bsums=bsums, dbeta=dbeta, dgamma=dgamma, dx=dx, amax2=amax2)
        if use_res:
            outs["dres"] = dres
        return outs
    got = run_both(dev, body, ("bn plain", shape, relu, use_res))
    what = ("bn plain", shape, relu, use_res)
    for k in ("mean", "invstd", "rm", "rv", "y", "dx", "dgamma", "dbeta"):
        _bn_close(got[k], ref[k], what + (k,))
    for k in ("mean", "invstd", "rm", "rv"):
        _bn_close(got[k + "2"], ref[k], what + (k, "stats_finalize"))
    _bn_close(got["sums"][:, 0], d["x"].double().sum((0, 2, 3)), what + ("sum x",))
    _bn_close(got["bsums"][:, 0], ref["dbeta"], what + ("sums dbeta",))
    _bn_close(got["bsums"][:, 1], ref["dgamma"], what + ("sums dgamma",))
    if use_res:
        _bn_close(got["dres"], ref["dres"], what + ("dres",))


@pytest.mark.parametrize("shape,where", _BN_SHAPES, ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))
@pytest.mark.parametrize("relu,use_res,xmask", [(0, False, False), (1, False, False), (1, True, False), (0, True, False), (1, False, True)])
def test_bn_fused_entries_footprint(dev, shape, where, relu, use_res, xmask):
    """dcl_bn_stats_part -> dcl_bn_apply_parts / dcl_bn_apply_fused -> dcl_bn_bwd_reduce_part -> dcl_bn_bwd_apply_fused, with the
    packed ReLU mask (relu = 2) where HW % 256 == 0 and with relu + 4 (the norm's input is a ReLU output)."""
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    n, c, h, w = shape
    hw = h * w
    d = _bn_data(shape, dev, where, seed=4)
    if xmask:
        d["x"] = d["x"].relu()
    res = d["res"] if use_res else None
    ref = _bn_ref(d["x"], res, d["gamma"], d["beta"], d["rm"], d["rv"], relu, d["dy"], xmask)
    ns = L.dcl_bn_num_slices(n, c)
    count = float(n * hw)
    packed = bool(relu and use_res and hw % 256 == 0)

    def body(ar):
        x, dy, gamma, beta = ar.inp(d["x"], "x"), ar.inp(d["dy"], "dy"), ar.inp(d["gamma"]), ar.inp(d["beta"])
        r = ar.inp(res, "res") if use_res else None
        part, pivot = ar.out(c * ns * 2, name="part"), ar.out(c, name="pivot")
        _lib.check(L.dcl_bn_stats_part(_p(x), n, c, hw, _p(part), _p(ar.inp(d["rm"])), _p(pivot), st), "dcl_bn_stats_part")
        outs = {"pivot": pivot}
        for form in ("parts", "fused"):
            y, mean, invstd = ar.out(shape, name="y " + form), ar.out(c, name="mean"), ar.out(c, name="invstd")
            rm, rv = ar.io(d["rm"], "running_mean"), ar.io(d["rv"], "running_var")
            nbt, amax = ar.io(torch.zeros(1, dtype=torch.int64, device=dev), "nbt"), ar.zeros(SLOTS, name="amax y")
            mask = ar.out(n * c * hw // 8, torch.uint8, "relu mask") if packed else None
            if form == "parts":
                _lib.check(L.dcl_bn_apply_parts(_p(x), _p(r), _p(part), ns, count, _BN_EPS, _BN_MOM, _p(gamma), _p(beta), n, c, hw, relu,
                                                _p(y), _p(mean), _p(invstd), _p(rm), _p(rv), _p(nbt), _p(amax), _p(pivot), _p(mask), st),
                           "dcl_bn_apply_parts")
            else:
                _lib.check(L.dcl_bn_apply_fused(_p(x), _p(r), _p(part), count, _BN_EPS, _BN_MOM, _p(gamma), _p(beta), n, c, hw, relu,
                                                _p(y), _p(mean), _p(invstd), _p(rm), _p(rv), _p(nbt), _p(amax), _p(pivot), _p(mask), st),
                           "dcl_bn_apply_fused")
            _tag_exact(amax, y, ("dcl_bn_apply_" + form, shape, relu, use_res))
            assert nbt.item() == 1
            outs.update({"y_" + form: y, "mean_" + form: mean, "invstd_" + form: invstd, "rm_" + form: rm, "rv_" + form: rv,
                         "amax_" + form: amax})
            if packed:
                outs["mask_" + form] = mask
        modes = [relu] + ([2] if packed else [])
        for mode in modes:
            yin = None
            if mode == 2:
                yin = ar.inp(mask, "packed mask")
            elif use_res or not relu:
                yin = ar.inp(y, "y")
            bpart = ar.out(c * ns * 2, name="bwd part")
            _lib.check(L.dcl_bn_bwd_reduce_part(_p(dy), _p(x), _p(yin), _p(mean), _p(invstd), _p(gamma), _p(beta), n, c, hw, mode,
                                                _p(bpart), st), "dcl_bn_bwd_reduce_part")
            dx, dres = ar.out(shape, name="dx"), (ar.out(shape, name="dres") if use_res else None)
            dbeta, dgamma, amax2 = ar.out(c, name="dbeta"), ar.out(c, name="dgamma"), ar.zeros(SLOTS, name="amax dx")
            bp_all, bp_loc = ar.inp(bpart, "part (all ranks)"), ar.inp(bpart, "part (this rank)")
            _lib.check(L.dcl_bn_bwd_apply_fused(_p(dy), _p(x), _p(yin), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(bp_all), _p(bp_loc),
                                                count, n, c, hw, mode + (4 if xmask else 0), _p(dx), _p(dres), _p(dbeta), _p(dgamma),
                                                _p(amax2), st), "dcl_bn_bwd_apply_fused")
            _tag_exact(amax2, dx, ("dcl_bn_bwd_apply_fused", shape, mode, use_res, xmask))
            outs.update({f"dx{mode}": dx, f"dbeta{mode}": dbeta, f"dgamma{mode}": dgamma, f"amax_dx{mode}": amax2})
            if use_res:
                outs[f"dres{mode}"] = dres
        return outs
    got = run_both(dev, body, ("bn fused", shape, relu, use_res, xmask))
    what = ("bn fused", shape, relu, use_res, xmask)
    for form in ("parts", "fused"):
        for k in ("y", "mean", "invstd", "rm", "rv"):
            _bn_close(got[k + "_" + form], ref[k], what + (k, form))
    assert torch.equal(got["y_parts"], got["y_fused"])
    for mode in [relu] + ([2] if packed else []):
        for k in ("dx", "dbeta", "dgamma") + (("dres",) if use_res else ()):
            _bn_close(got[f"{k}{mode}"], ref[k], what + (k, mode))
    if packed:
        assert torch.equal(got["dx2"], got[f"dx{relu}"])


@pytest.mark.parametrize("shape,where", _BN_SHAPES + [((2, 16, 9, 8), "last")],
                         ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))
def test_bn_deferred_entries_footprint(dev, shape, where):
    """dcl_bn_stats_minmax_part -> dcl_bn_finalize_pre, and dcl_bn_stats_pre (one launch): mm sized by dcl_bn_num_slices, tickets
    exactly C words, amax exactly 64 floats; the tag, derived from the slices' extrema, equals the maximum of
    relu(fma(x, pre_sc, pre_sh)) formed in fp32.  Where the consumers take the shape: dcl_conv3x3_pre_f16x3 and
    dcl_wgrad3x3_pre_f16x3 on the map."""
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    n, c, h, w = shape
    hw = h * w
    d = _bn_data(shape, dev, where, seed=6)
    ref = _bn_ref(d["x"], None, d["gamma"], d["beta"], d["rm"], d["rv"], 1, d["dy"])
    ns = L.dcl_bn_num_slices(n, c)
    count = float(n * hw)

    def mapped(x, sc, sh):
        return torch.relu(torch.addcmul(sh.view(1, -1, 1, 1), x, sc.view(1, -1, 1, 1)))

    def body(ar):
        x, gamma, beta = ar.inp(d["x"], "x"), ar.inp(d["gamma"]), ar.inp(d["beta"])
        outs = {}
        for form in ("two", "one"):
            part, mm = ar.out(c * ns * 2, name="part"), ar.out(c * ns * 2, name="mm")
            mean, invstd, sc, sh = ar.out(c, name="mean"), ar.out(c, name="invstd"), ar.out(c, name="pre_sc"), ar.out(c, name="pre_sh")
            rm, rv = ar.io(d["rm"], "running_mean"), ar.io(d["rv"], "running_var")
            nbt, amax = ar.io(torch.zeros(1, dtype=torch.int64, device=dev), "nbt"), ar.zeros(SLOTS, name="amax")
            if form == "two":
                pivot = ar.out(c, name="pivot")
                _lib.check(L.dcl_bn_stats_minmax_part(_p(x), n, c, hw, _p(part), _p(mm), _p(ar.inp(d["rm"])), _p(pivot), st),
                           "dcl_bn_stats_minmax_part")
                _lib.check(L.dcl_bn_finalize_pre(_p(ar.inp(part)), _p(ar.inp(mm)), ns, count, _BN_EPS, _BN_MOM, _p(gamma), _p(beta), c,
                                                 _p(mean), _p(invstd), _p(rm), _p(rv), _p(nbt), _p(ar.inp(pivot)), _p(sc), _p(sh), _p(amax),
                                                 st), "dcl_bn_finalize_pre")
            else:
                tickets = ar.zeros(c, torch.int32, "tickets")
                _lib.check(L.dcl_bn_stats_pre(_p(x), n, c, hw, _p(part), _p(mm), _p(tickets), count, _BN_EPS, _BN_MOM, _p(gamma), _p(beta),
                                              _p(mean), _p(invstd), _p(rm), _p(rv), _p(nbt), _p(sc), _p(sh), _p(amax), st),
                           "dcl_bn_stats_pre")
            _tag_exact(amax, mapped(x, sc, sh), ("dcl_bn_finalize_pre" if form == "two" else "dcl_bn_stats_pre", shape))
            assert nbt.item() == 1
            outs.update({k + form: v for k, v in dict(mean=mean, invstd=invstd, sc=sc, sh=sh, rm=rm, rv=rv, amax=amax).items()})
        return outs
    got = run_both(dev, body, ("bn deferred", shape))
    for form in ("two", "one"):
        for k in ("mean", "invstd", "rm", "rv"):
            _bn_close(got[k + form], ref[k], ("bn deferred", shape, k, form))
        _bn_close(mapped(d["x"], got["sc" + form], got["sh" + form]), ref["y"], ("bn deferred", shape, "map", form))
    for k in ("mean", "invstd", "sc", "sh", "rm", "rv", "amax"):
        assert torch.equal(got[k + "two"], got[k + "one"]), k          # the header: bitwise the two-call form
    # the consumers of the map, at the shapes they take
    co = 32
    sc, sh = got["scone"], got["shone"]
    act = mapped(d["x"], sc, sh)
    g = torch.Generator(device=dev).manual_seed(8)
    wt = torch.randn(co, c, 3, 3, device=dev, generator=g) * (2.0 / (9 * c)) ** 0.5
    for stride in (1, 2):
        if c % 16 == 0 and L.dcl_conv3x3_pre_supported(n, c, co, h, w, stride) == 1:
            want = F.conv2d(act.double(), wt.double(), stride=stride, padding=1)

            def cbody(ar):
                wam, _ = _tag_in(ar, wt)
                wp = ar.out(_pack_bytes(co, c, 9), torch.uint8, "wp")
                _lib.check(L.dcl_conv3x3_pack(_p(ar.inp(wt)), co, c, 0, _p(wam), _p(wp), st), "pack")
                y = ar.out(tuple(want.shape), name="y")
                _lib.check(L.dcl_conv3x3_pre_f16x3(_p(ar.inp(d["x"], "x")), n, c, h, w, _p(wp), co, _p(ar.inp(got["amaxone"])), SLOTS,
                                                   _p(wam), _p(ar.inp(sc)), _p(ar.inp(sh)), None, _p(y), stride, 0, 0, st),
                           "dcl_conv3x3_pre_f16x3")
                return {"y": y}
            err = _rel(run_both(dev, cbody, ("conv pre", shape, stride))["y"], want)
            assert err < 3e-6, ("dcl_conv3x3_pre_f16x3", shape, stride, err)       # tests/test_pre_norm_conv.py holds it bitwise to the
            #                                                                          two-step form, whose bar is 3e-6
        if c % 16 == 0 and w % (8 if stride == 1 else 16) == 0 and L.dcl_wgrad3x3_pre_supported(n, c, co, h, w, stride) == 1:
            ho, wo = ((h - 1) // 2 + 1, w // 2) if stride == 2 else (h, w)
            gy = torch.randn(n, co, ho, wo, device=dev, generator=g) * 3e-5
            _wgrad_run(dev, d["x"], gy, _wgrad_ref(act, gy, stride, 3), stride, 3, 3e-6 if stride == 1 else 2e-6,
                       ("dcl_wgrad3x3_pre_f16x3", shape, stride), pre=(sc, sh, act), counts=(SLOTS, 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# bilinear resize

@pytest.mark.parametrize("align", [1, 0])
@pytest.mark.parametrize("shape,size", [((3, 7, 9, 13), (36, 52)), ((2, 3, 1, 5), (4, 20))])
def test_upsample_bilinear_footprint(dev, shape, size, align):
    """dcl_upsample_bilinear_fwd / _bwd (with and without addend, ReLU) and the two slice forms with ctot = 11, c0 = 3, C = 5: the
    channels of y_wide outside [c0, c0 + C) stay as they were."""
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    n, c, h, w = shape
    H, W = size
    g = torch.Generator(device=dev).manual_seed(1 + h)
    x = torch.randn(shape, device=dev, generator=g)
    add = torch.randn(n, c, H, W, device=dev, generator=g)
    dy = torch.randn(n, c, H, W, device=dev, generator=g)
    xd = x.double().requires_grad_(True)
    up = F.interpolate(xd, size=size, mode="bilinear", align_corners=bool(align))
    up.backward(dy.double())

    def body(ar):
        xg = ar.inp(x, "x")
        y0, y1, dx = ar.out((n, c, H, W), name="y"), ar.out((n, c, H, W), name="y addend relu"), ar.out(shape, name="dx")
        _lib.check(L.dcl_upsample_bilinear_fwd(_p(xg), None, n * c, h, w, H, W, align, 0, _p(y0), st), "fwd")
        _lib.check(L.dcl_upsample_bilinear_fwd(_p(xg), _p(ar.inp(add, "addend")), n * c, h, w, H, W, align, 1, _p(y1), st), "fwd")
        _lib.check(L.dcl_upsample_bilinear_bwd(_p(ar.inp(dy, "dy")), n * c, h, w, H, W, align, _p(dx), st), "bwd")
        return {"y0": y0, "y1": y1, "dx": dx}
    got = run_both(dev, body, ("upsample", shape, size, align))
    # 1e-5 / 1e-4 of max(1, max): test_upsample_bilinear_matches_torch
    assert (got["y0"].double() - up.detach()).abs().max().item() <= 1e-5 * max(1.0, up.abs().max().item())
    want1 = torch.relu(up.detach() + add.double())
    assert (got["y1"].double() - want1).abs().max().item() <= 1e-5 * max(1.0, want1.abs().max().item())
    assert (got["dx"].double() - xd.grad).abs().max().item() <= 1e-4 * max(1.0, xd.grad.abs().max().item())

    ctot, c0, C = 11, 3, 5
    xs = torch.randn(n, C, h, w, device=dev, generator=g)
    dyw = torch.randn(n, ctot, H, W, device=dev, generator=g)
    xsd = xs.double().requires_grad_(True)
    ups = F.interpolate(xsd, size=size, mode="bilinear", align_corners=bool(align))
    ups.backward(dyw[:, c0:c0 + C].double())

    def sbody(ar):
        wide, dxs = ar.out((n, ctot, H, W), name="y_wide"), ar.out((n, C, h, w), name="dx")
        _lib.check(L.dcl_upsample_bilinear_fwd_slice(_p(ar.inp(xs, "x")), n, C, h, w, H, W, align, _p(wide), ctot, c0, st), "fwd_slice")
        assert all_sentinel(wide[:, :c0]) and all_sentinel(wide[:, c0 + C:]), "channels outside [c0, c0 + C) of y_wide were written"
        # the gradient's other channels carry the run's poison: they must not enter dx
        poisoned = dyw.clone()
        poisoned[:, :c0] = float("nan") if ar.fill != NAN_BITS else 1e30
        poisoned[:, c0 + C:] = float("nan") if ar.fill != NAN_BITS else 1e30
        _lib.check(L.dcl_upsample_bilinear_bwd_slice(_p(ar.inp(poisoned, "dy_wide")), ctot, c0, n, C, h, w, H, W, align, _p(dxs), st),
                   "bwd_slice")
        return {"y": wide[:, c0:c0 + C], "dx": dxs}
    got = run_both(dev, sbody, ("upsample slice", shape, size, align))
    assert (got["y"].double() - ups.detach()).abs().max().item() <= 1e-5 * max(1.0, ups.abs().max().item())
    assert (got["dx"].double() - xsd.grad).abs().max().item() <= 1e-4 * max(1.0, xsd.grad.abs().max().item())


# ---------------------------------------------------------------------------------------------------------------------------------
# split-f16 GEMM

_GEMM_SHAPES = [(100, 36, 32, 1), (260, 520, 96, 1), (36, 700, 416, 3)]
_GAP = 4


def _gemm_operands(M, N, K, batch, akm, bkm, dev, g, where=None):
    A = torch.randn((batch, M, K) if akm else (batch, K, M), device=dev, generator=g)
    B = torch.randn((batch, N, K) if bkm else (batch, K, N), device=dev, generator=g) * 0.03
    if where:
        _plant(A, where, big=3.0)
    Ad = A.double() if akm else A.double().transpose(1, 2)
    Bd = B.double() if bkm else B.double().transpose(1, 2)
    return A, B, Ad @ Bd.transpose(1, 2)


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5])
def test_gemm_f16x3_footprint(dev, tile):
    """dcl_gemm_f16x3 with ldc = N + 4: the four gap columns of every row stay untouched; every legal layout, split-k with the
    workspace of dcl_gemm_workspace_floats, c_amax exactly one float and exact, operand tags as 1 and as 64 floats, a_rowsum."""
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(5 + tile)
    ran = 0
    try:
        L.dcl_gemm_set_tile(tile)
        for ci, (M, N, K, batch) in enumerate(_GEMM_SHAPES):
            ldc = N + _GAP
            for akm in (1, 0):
                for bkm in (1, 0):
                    lda, ldb = (K if akm else M), (K if bkm else N)
                    if L.dcl_gemm_supported(M, N, K, lda, akm, ldb, bkm) != 1:
                        continue
                    A, B, ref = _gemm_operands(M, N, K, batch, akm, bkm, dev, g, ("first", "last", "neg")[(ci + akm + bkm) % 3])
                    bias = torch.randn(N, device=dev, generator=g)
                    C0 = torch.randn(batch, M, N, device=dev, generator=g)
                    for splitk in ((1, 2) if K >= 64 else (1,)):
                        for acc in (0, 1):
                            count = SLOTS if (splitk + acc) % 2 else 1
                            rowsum = (not akm) and batch == 1 and not acc
                            nws = int(L.dcl_gemm_workspace_floats(M, N, batch, splitk)) if splitk > 1 else 0
                            what = ("gemm", tile, M, N, K, batch, akm, bkm, splitk, acc)

                            def body(ar):
                                Ag, Bg = ar.inp(A, "A"), ar.inp(B, "B")
                                aam, ac = _tag_in(ar, A, count)
                                bam, bc = _tag_in(ar, B, count)
                                C = ar.out((batch, M, ldc), name="C")
                                if acc:
                                    C[:, :, :N] = C0
                                ca = ar.zeros(1, name="c_amax")
                                ws = ar.out(nws, name="ws") if nws else None
                                rs = ar.out(M, name="a_rowsum") if rowsum else None
                                _lib.check(L.dcl_gemm_f16x3(_p(Ag), lda, akm, M * K, _p(Bg), ldb, bkm, N * K, M, N, K, batch, _p(aam), ac,
                                                            _p(bam), bc, _p(ar.inp(bias, "bias")), _p(C), ldc, M * ldc, acc, _p(ca), splitk,
                                                            _p(ws), _p(rs), st), "dcl_gemm_f16x3")
                                assert all_sentinel(C[:, :, N:]), (what, "gap columns of C written")
                                _tag_exact(ca, C[:, :, :N], what)
                                outs = {"C": C[:, :, :N], "c_amax": ca}
                                if rowsum:
                                    outs["rowsum"] = rs
                                return outs
                            got = run_both(dev, body, what)
                            ran += 1
                            want = ref + bias.double() + (C0.double() if acc else 0)
                            err = ((got["C"].double() - want).abs().max() / ref.abs().max()).item()
                            assert err < 3e-6, (what, err)                  # test_gemm_f16x3_every_layout_matches_fp64
                            if rowsum:
                                want_rs = A.double().sum(1)[0]
                                assert _rel(got["rowsum"], want_rs) < 1e-5, what
        assert ran == 4 * 1 * 2 + 2 * 4 * 2 * 2, ran          # every layout of every shape is legal and ran
        # an all-zero operand: tag 0, scale 1, exactly zero
        M, N, K = 100, 36, 32
        A, B, _ = _gemm_operands(M, N, K, 1, 1, 1, dev, g)

        def zbody(ar):
            C, ca = ar.out((M, N + _GAP), name="C"), ar.zeros(1, name="c_amax")
            _lib.check(L.dcl_gemm_f16x3(_p(ar.inp(torch.zeros_like(A))), K, 1, 0, _p(ar.inp(B)), K, 1, 0, M, N, K, 1,
                                        _p(ar.inp(torch.zeros(1, device=dev))), 1, _p(_tag_in(ar, B)[0]), 1, None, _p(C), N + _GAP, 0, 0,
                                        _p(ca), 1, None, None, st), "gemm zero")
            return {"C": C[:, :N], "c_amax": ca}
        got = run_both(dev, zbody, ("gemm zero A", tile))
        assert bool((got["C"] == 0).all()) and got["c_amax"].item() == 0.0
    finally:
        L.dcl_gemm_set_tile(0)


def _gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def _dgelu64(v):
    return 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5])
def test_gemm_f16x3_epilogues_footprint(dev, tile):
    """dcl_gemm_f16x3_ep (ep 1, 2, 3) and dcl_gemm_f16x3_ascaled with ldc = N + 4: the gap columns of C, C2 and aux stay untouched
    (aux's carry poison that must not enter C); c_amax exact."""
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(15 + tile)
    try:
        L.dcl_gemm_set_tile(tile)
        for (M, N, K, _) in _GEMM_SHAPES[:2]:
            ldc = N + _GAP
            for ep in (1, 2, 3):
                bkm = 0 if ep == 2 else 1
                A, B, ref = _gemm_operands(M, N, K, 1, 1, bkm, dev, g, ("first", "last", "neg")[ep - 1])
                A, B, ref = A[0], B[0], ref[0]
                bias = torch.randn(N, device=dev, generator=g)
                aux = torch.randn(M, N, device=dev, generator=g)
                rows_per = max(32, M // 4)                       # the entry's floor: a tile row group spans at most two samples
                rowscale = torch.rand((M + rows_per - 1) // rows_per, device=dev, generator=g) + 0.5
                v = ref + bias.double()
                if ep == 1:
                    want, want2 = v, _gelu64(v)
                elif ep == 2:
                    want = v * _dgelu64(aux.double())
                else:
                    want = aux.double() + rowscale.double().repeat_interleave(rows_per)[:M, None] * v
                what = ("gemm ep", tile, M, N, K, ep)

                def body(ar):
                    aam, ac = _tag_in(ar, A, SLOTS if ep == 2 else 1)
                    bam, bc = _tag_in(ar, B, 1 if ep == 2 else SLOTS)
                    C, ca = ar.out((M, ldc), name="C"), ar.zeros(1, name="c_amax")
                    C2 = ar.out((M, ldc), name="C2") if ep == 1 else None
                    auxg = None
                    if ep > 1:
                        wide = torch.full((M, ldc), float("nan") if ar.fill != NAN_BITS else 1e30, device=dev)
                        wide[:, :N] = aux
                        auxg = ar.inp(wide, "aux")
                    _lib.check(L.dcl_gemm_f16x3_ep(_p(ar.inp(A, "A")), K, 1, _p(ar.inp(B, "B")), K if bkm else N, bkm, M, N, K, _p(aam), ac,
                                                   _p(bam), bc, _p(ar.inp(bias, "bias")), _p(C), ldc, _p(ca), ep, _p(C2), _p(auxg),
                                                   _p(ar.inp(rowscale, "rowscale")) if ep == 3 else None, rows_per, st), "dcl_gemm_f16x3_ep")
                    assert all_sentinel(C[:, N:]), (what, "gap columns of C written")
                    _tag_exact(ca, C[:, :N], what)
                    outs = {"C": C[:, :N], "c_amax": ca}
                    if ep == 1:
                        assert all_sentinel(C2[:, N:]), (what, "gap columns of C2 written")
                        outs["C2"] = C2[:, :N]
                    return outs
                got = run_both(dev, body, what)
                den = want.abs().max()
                assert ((got["C"].double() - want).abs().max() / den).item() < 3e-6, what        # tests/test_fused_mlp.py
                if ep == 1:
                    assert ((got["C2"].double() - want2).abs().max() / den).item() < 3e-6, what
            # per-token factor on A: a Linear's data gradient (A k-major) and weight gradient (A row-contiguous, split-k, row sums)
            for akm in (1, 0):
                A, B, _ = _gemm_operands(M, N, K, 1, akm, 0, dev, g, "neg")
                A, B = A[0], B[0]
                tokens = M if akm else K
                group = 32 if not akm else (M // 4 if M % 4 == 0 else M)
                nsc = (tokens + group - 1) // group
                scale = torch.rand(nsc, device=dev, generator=g) + 0.5
                f = scale.double().repeat_interleave(group)[:tokens]
                Ad = (A.double() * f[:, None]) if akm else (A.double() * f[:, None]).t()
                want = Ad @ B.double()
                for splitk in ((1, 2) if (K >= 64 and not akm) else (1,)):
                    nws = int(L.dcl_gemm_workspace_floats(M, N, 1, splitk)) if splitk > 1 else 0
                    what = ("gemm ascaled", tile, M, N, K, akm, splitk)

                    def body(ar):
                        aam, ac = _tag_in(ar, A, SLOTS)
                        bam, bc = _tag_in(ar, B, 1)
                        C, ca = ar.out((M, ldc), name="C"), ar.zeros(1, name="c_amax")
                        ws = ar.out(nws, name="ws") if nws else None
                        rs = ar.out(M, name="a_rowsum") if not akm else None
                        _lib.check(L.dcl_gemm_f16x3_ascaled(_p(ar.inp(A, "A")), K if akm else M, akm, _p(ar.inp(B, "B")), N, 0, M, N, K,
                                                            _p(aam), ac, _p(bam), bc, _p(C), ldc, _p(ca), splitk, _p(ws), _p(rs),
                                                            _p(ar.inp(scale, "a_scale")), group, 0, None, st), "dcl_gemm_f16x3_ascaled")
                        assert all_sentinel(C[:, N:]), (what, "gap columns of C written")
                        _tag_exact(ca, C[:, :N], what)
                        outs = {"C": C[:, :N], "c_amax": ca}
                        if rs is not None:
                            outs["rowsum"] = rs
                        return outs
                    got = run_both(dev, body, what)
                    assert _rel(got["C"], want) < 3e-6, what                                   # tests/test_fused_mlp.py
                    if not akm:
                        assert _rel(got["rowsum"], Ad.sum(1)) < 1e-5, what
    finally:
        L.dcl_gemm_set_tile(0)


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm

@pytest.mark.parametrize("M,C,where", [(777, 384, "last"), (50, 32, "first"), (9, 2048, "neg")])
def test_layernorm_footprint(dev, M, C, where):
    """dcl_layernorm_fwd / _bwd: parts sized by dcl_layernorm_bwd_parts, both absmax buffers exactly 64 floats and exact."""
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    assert L.dcl_layernorm_supported(C) == 1
    g = torch.Generator(device=dev).manual_seed(11)
    gamma, beta = torch.rand(C, device=dev, generator=g) + 0.5, torch.randn(C, device=dev, generator=g)
    x = _plant(torch.randn(M, C, device=dev, generator=g) * 2.0 + 3.0, where)
    gy = _plant(torch.randn(M, C, device=dev, generator=g), where)
    addend = torch.randn(M, C, device=dev, generator=g)
    xd, gd, bd = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    yd = F.layer_norm(xd, (C,), gd, bd, 1e-5)
    yd.backward(gy.double())
    nparts = L.dcl_layernorm_bwd_parts(M, C)
    assert nparts > 0

    def body(ar):
        xg, gam = ar.inp(x, "x"), ar.inp(gamma, "gamma")
        y, mean, rstd, yam = ar.out((M, C), name="y"), ar.out(M, name="mean"), ar.out(M, name="rstd"), ar.zeros(SLOTS, name="yamax")
        _lib.check(L.dcl_layernorm_fwd(_p(xg), _p(gam), _p(ar.inp(beta, "beta")), M, C, 1e-5, _p(y), _p(mean), _p(rstd), _p(yam), st),
                   "dcl_layernorm_fwd")
        _tag_exact(yam, y, ("dcl_layernorm_fwd", M, C))
        outs = {"y": y, "mean": mean, "rstd": rstd, "yamax": yam}
        for k, ad in (("", None), ("_add", addend)):
            gx, parts, gwb = ar.out((M, C), name="gx"), ar.out((nparts, 2, C), name="parts"), ar.out((2, C), name="dgamma_dbeta")
            gxam = ar.zeros(SLOTS, name="gxamax")
            _lib.check(L.dcl_layernorm_bwd(_p(ar.inp(gy, "gy")), _p(xg), _p(gam), _p(ar.inp(mean)), _p(ar.inp(rstd)), M, C, _p(gx),
                                           _p(parts), _p(gwb), _p(ar.inp(ad, "addend")) if ad is not None else None, _p(gxam), st),
                       "dcl_layernorm_bwd")
            _tag_exact(gxam, gx, ("dcl_layernorm_bwd", M, C, k))
            outs.update({"gx" + k: gx, "gwb" + k: gwb, "gxamax" + k: gxam})
        return outs
    got = run_both(dev, body, ("layernorm", M, C))
    # 3e-6 of max: test_fused_layernorm_matches_fp64
    assert _rel(got["y"], yd.detach()) < 3e-6
    assert _rel(got["gx"], xd.grad) < 3e-6
    assert ((got["gx_add"].double() - (xd.grad + addend.double())).abs().max() / xd.grad.abs().max()).item() < 3e-6
    assert _rel(got["gwb"][0], gd.grad) < 3e-6 and _rel(got["gwb"][1], bd.grad) < 3e-6
    assert torch.equal(got["gwb"], got["gwb_add"])


# ---------------------------------------------------------------------------------------------------------------------------------
# element-wise helpers and the absmax reductions

@pytest.mark.parametrize("n", [1, 3, 4097])
def test_add_n_and_absmax_footprint(dev, n):
    """dcl_add_n (2, 3, 4 operands) and dcl_absmax at ragged lengths, the maximum at the first element, at the last element of
    the ragged tail and on a negative value; dcl_absmax max-es INTO out[0]."""
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(n)
    ts = [torch.randn(n, device=dev, generator=g) for _ in range(4)]
    for k in (2, 3, 4):
        def body(ar):
            ins = [ar.inp(t) for t in ts[:k]] + [None] * (4 - k)
            out = ar.out(n, name="out")
            _lib.check(L.dcl_add_n(_p(ins[0]), _p(ins[1]), _p(ins[2]), _p(ins[3]), n, _p(out), st), "dcl_add_n")
            return {"out": out}
        got = run_both(dev, body, ("add_n", n, k))
        want = sum(t.double() for t in ts[:k])
        # k - 1 fp32 additions, each rounding by at most 2^-24 of a partial sum that is at most sum |t_i|
        bound = (k - 1) * 2.0 ** -24 * sum(t.double().abs() for t in ts[:k])
        assert bool(((got["out"].double() - want).abs() <= bound).all()), ("dcl_add_n", n, k)
    for where in ("first", "last", "neg"):
        x = _plant(torch.randn(n, device=dev, generator=g), where)
        for prior in (0.0, 1e9):
            def body(ar):
                out = ar.io(torch.full((1,), prior, device=dev), "out")
                _lib.check(L.dcl_absmax(_p(ar.inp(x)), n, _p(out), st), "dcl_absmax")
                return {"out": out}
            got = run_both(dev, body, ("absmax", n, where, prior))
            want = torch.maximum(x.abs().max(), torch.tensor(prior, device=dev))
            assert _same_bits(got["out"], want), ("dcl_absmax", n, where, prior, got["out"].item(), want.item())

    def zbody(ar):
        out = ar.zeros(1, name="out")
        _lib.check(L.dcl_absmax(_p(ar.inp(torch.zeros(n, device=dev))), n, _p(out), st), "dcl_absmax")
        return {"out": out}
    assert run_both(dev, zbody, ("absmax zero", n))["out"].item() == 0.0


def test_absmax_multi_footprint(dev):
    """dcl_absmax_multi: three jobs of ragged length (1, 4097, 3 + 2 * 4096), each job's out its own guarded float; exact."""
    import numpy as np
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(2)
    xs = [_plant(torch.randn(n, device=dev, generator=g), w) for n, w in ((1, "first"), (4097, "last"), (3 + 2 * 4096, "neg"))]

    def body(ar):
        jobs = np.zeros(len(xs), dtype=[("x", "<u8"), ("out", "<u8"), ("n", "<i8"), ("fb", "<i4"), ("pad", "<i4")])
        b2j, outs = [], {}
        for i, x in enumerate(xs):
            outs[f"out{i}"] = ar.zeros(1, name=f"out{i}")
            jobs[i] = (ar.inp(x).data_ptr(), outs[f"out{i}"].data_ptr(), x.numel(), len(b2j), 0)
            b2j += [i] * ((x.numel() + 4095) // 4096)
        jd = ar.inp(torch.from_numpy(jobs.view(np.uint8).reshape(-1).copy()).to(dev), "jobs")
        _lib.check(L.dcl_absmax_multi(_p(jd), _p(ar.inp(torch.tensor(b2j, dtype=torch.int32, device=dev), "blk2job")), len(b2j), st),
                   "dcl_absmax_multi")
        return outs
    got = run_both(dev, body, "absmax_multi")
    for i, x in enumerate(xs):
        assert _same_bits(got[f"out{i}"], x.abs().max()), ("dcl_absmax_multi", i, got[f"out{i}"].item(), x.abs().max().item())


@pytest.mark.parametrize("na,nb", [(1, 1), (64, 1), (1, 64), (64, 64), (3, 5)])
def test_amax_sum2_footprint(dev, na, nb):
    """dcl_amax_sum2: out[0] = max(a) + max(b) bounds max|A + B|; exactly one float is written, exactly na / nb are read."""
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(na * 100 + nb)
    A, B = torch.randn(4097, device=dev, generator=g) * 3, torch.randn(4097, device=dev, generator=g)
    true = (A + B).abs().max()

    def parts(t, n):
        v = torch.rand(n, device=dev, generator=g) * t.abs().max()
        v[n - 1] = t.abs().max()
        return v
    a, b = parts(A, na), parts(B, nb)

    def body(ar):
        out = ar.out(1, name="out")
        _lib.check(L.dcl_amax_sum2(_p(ar.inp(a, "a")), na, _p(ar.inp(b, "b")), nb, _p(out), st), "dcl_amax_sum2")
        return {"out": out}
    got = run_both(dev, body, ("amax_sum2", na, nb))["out"]
    assert got.item() >= true.item(), ("dcl_amax_sum2 bound / true maximum", got.item() / true.item())
    assert _same_bits(got, a.max() + b.max()), ("dcl_amax_sum2 bound / true maximum", got.item() / true.item())
    print(f"dcl_amax_sum2 na={na} nb={nb}: bound / true maximum = {got.item() / true.item():.4f}")


# ---------------------------------------------------------------------------------------------------------------------------------
# per-step metrics

@pytest.mark.parametrize("tbytes", [8, 4, 1])
def test_confusion_matrix_and_metrics_footprint(dev, tbytes):
    """dcl_confusion_matrix, dcl_confusion_matrix_pred (cols = C + 1: the ignore column) and dcl_metrics_from_cm with ld > C; cm and
    oob are accumulated into, integer arithmetic: exact."""
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    N, C, HW = 2, 19, 777
    cols = C + 1
    g = torch.Generator(device=dev).manual_seed(tbytes)
    logits = torch.randn(N, C, HW, device=dev, generator=g)
    target = torch.randint(0, cols + 2, (N, HW), device=dev, generator=g)          # two ids out of range
    tdt = {8: torch.int64, 4: torch.int32, 1: torch.uint8}[tbytes]
    prior = torch.randint(0, 5, (C, cols), device=dev, generator=g).to(torch.int32)
    pred = logits.argmax(1).reshape(-1)
    ok = target.reshape(-1) < cols
    want_cm = prior + torch.bincount(pred[ok] * cols + target.reshape(-1)[ok], minlength=C * cols).view(C, cols).to(torch.int32)
    want_oob = 3 + int((~ok).sum())

    def body(ar):
        outs = {}
        for form in ("logits", "pred"):
            cm, oob = ar.io(prior, "cm"), ar.io(torch.full((1,), 3, dtype=torch.int32, device=dev), "oob")
            tg = ar.inp(target.to(tdt), "target")
            if form == "logits":
                _lib.check(L.dcl_confusion_matrix(_p(ar.inp(logits, "logits")), N, C, HW, _p(tg), tbytes, cols, _p(cm), _p(oob), st),
                           "dcl_confusion_matrix")
            else:
                _lib.check(L.dcl_confusion_matrix_pred(_p(ar.inp(pred.to(torch.uint8), "pred")), N * HW, _p(tg), tbytes, C, cols, _p(cm),
                                                       _p(oob), st), "dcl_confusion_matrix_pred")
            outs["cm_" + form], outs["oob_" + form] = cm, oob
        out3 = ar.out(3, name="out3")
        _lib.check(L.dcl_metrics_from_cm(_p(ar.inp(want_cm, "cm [C, C + 1]")), C, cols, _p(out3), st), "dcl_metrics_from_cm")
        outs["out3"] = out3
        return outs
    got = run_both(dev, body, ("metrics", tbytes))
    for form in ("logits", "pred"):
        assert torch.equal(got["cm_" + form], want_cm) and got["oob_" + form].item() == want_oob, form
    cm = want_cm[:, :C].double()
    diag = cm.diag()
    rows = cm.sum(1)
    rows[rows == 0] = 1
    iou = torch.nan_to_num(diag / (cm.sum(0) + cm.sum(1) - diag), nan=0.0)
    want3 = torch.stack([diag.sum() / cm.sum(), (diag / rows).mean(), iou.mean()])
    assert torch.allclose(got["out3"].double(), want3, rtol=2e-6, atol=0), (got["out3"], want3)         # tests/test_metrics.py


# ---------------------------------------------------------------------------------------------------------------------------------
# loss side: label histogram, rank select, gathers

def test_label_hist_rank_select_gather_scatter_footprint(dev):
    """dcl_label_hist, dcl_rank_select, dcl_gather_raw, dcl_scatter_raw, dcl_gather_normalize at sizes that are no multiple of
    the stride, of DCL_SEG = 256 or of DCL_ROW_TILE = 128 (the sizes of test_k1_k2_direct_odd_sizes); integer results exact,
    the raw gather / scatter exact copies."""
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    n, H, W, K, scale = 3, 101, 203, 7, 3
    g = torch.Generator(device=dev).manual_seed(11)
    label = torch.randint(0, K + 2, (n, H, W), device=dev, generator=g)
    label[0, :5, :5] = -1
    h, w = H // scale, W // scale
    hw = h * w
    nseg = (hw + 255) // 256
    # nearest down-sampling as F.interpolate(mode='nearest') does it
    lbl_ref = F.interpolate(label.double().unsqueeze(1), size=(h, w), mode="nearest").squeeze(1).long().reshape(n, hw)
    bad = (lbl_ref < 0) | (lbl_ref >= K)
    counts_ref = torch.stack([torch.bincount(lbl_ref[b][~bad[b]], minlength=K) for b in range(n)]).to(torch.int32)
    lbl_u8 = torch.where(bad, torch.full_like(lbl_ref, 255), lbl_ref).to(torch.uint8)
    pairs = [(0, 1), (2, 6), (1, 0)]
    T = len(pairs)
    V = int(min(counts_ref[b, k] for b, k in pairs))
    sel = torch.stack([torch.randperm(int(counts_ref[b, k]), device=dev, generator=g)[:V] for b, k in pairs]).to(torch.int32)
    pb = torch.tensor([b for b, _ in pairs], dtype=torch.int32, device=dev)
    pk = torch.tensor([k for _, k in pairs], dtype=torch.int32, device=dev)
    want_pix = torch.stack([torch.nonzero(lbl_ref[b] == k).flatten()[sel[t].long()] for t, (b, k) in enumerate(pairs)]).to(torch.int32)
    C = 37
    feat = torch.randn(n, C, hw, device=dev, generator=g)
    dX = torch.randn(T, C, V, device=dev, generator=g)
    slot = torch.tensor([2, 0, 1], dtype=torch.int32, device=dev)
    Npad = (T * V + 127) // 128 * 128

    def body(ar):
        lbl_s, seg = ar.out((n, hw), torch.uint8, "lbl_s"), ar.out((n, nseg, K), torch.int32, "seg_hist")
        counts = ar.zeros((n, K), torch.int32, "counts")
        _lib.check(L.dcl_label_hist(_p(ar.inp(label, "label")), n, H, W, scale, K, _p(lbl_s), _p(seg), _p(counts), st), "dcl_label_hist")
        pix = ar.out((T, V), torch.int32, "pix")
        pbg, pkg = ar.inp(pb, "pair_b"), ar.inp(pk, "pair_k")
        _lib.check(L.dcl_rank_select(_p(ar.inp(lbl_s)), _p(ar.inp(seg)), n, hw, K, _p(pbg), _p(pkg), T, V, _p(ar.inp(sel, "sel")), _p(pix),
                                     st), "dcl_rank_select")
        fg, pixg = ar.inp(feat, "feat"), ar.inp(pix, "pix")
        X = ar.out((T, C, V), name="X")
        _lib.check(L.dcl_gather_raw(_p(fg), C * hw, hw, 1, C, _p(pixg), _p(pbg), T, V, _p(X), st), "dcl_gather_raw")
        dfeat = ar.zeros((n, C, hw), name="dfeat")
        _lib.check(L.dcl_scatter_raw(_p(ar.inp(dX, "dX")), C * hw, hw, 1, C, _p(pixg), _p(pbg), T, V, _p(dfeat), st), "dcl_scatter_raw")
        bank, nrm = ar.out((Npad, 256), name="bank"), ar.out(Npad, name="nrm")
        bank_h = ar.out((Npad, 512), torch.float16, "bank_h")
        _lib.check(L.dcl_gather_normalize(_p(fg), C * hw, hw, 1, C, _p(pixg), _p(pbg), _p(ar.inp(slot, "slot_pair")), T, V, _p(bank),
                                          _p(nrm), _p(bank_h), st), "dcl_gather_normalize")
        return dict(lbl_s=lbl_s, seg=seg, counts=counts, pix=pix, X=X, dfeat=dfeat, bank=bank, nrm=nrm[:T * V], bank_h=bank_h)
    got = run_both(dev, body, "loss sampling")
    assert torch.equal(got["lbl_s"], lbl_u8) and torch.equal(got["counts"], counts_ref)
    assert torch.equal(got["seg"].sum(1).to(torch.int32), counts_ref)
    assert torch.equal(got["pix"], want_pix)
    bidx = pb.long()[:, None].expand(T, V)
    wantX = feat[bidx, :, want_pix.long()].permute(0, 2, 1)                     # [T, C, V]
    assert torch.equal(got["X"], wantX)
    want_d = torch.zeros(n, C, hw, device=dev)
    want_d[bidx, :, want_pix.long()] = dX.permute(0, 2, 1)
    assert torch.equal(got["dfeat"], want_d)
    rows = wantX[slot.long()].permute(0, 2, 1).reshape(T * V, C).double()       # bank row u * V + v = pixel v of pair slot_pair[u]
    nr = rows.norm(dim=1)
    bank = got["bank"]
    assert bool((bank[T * V:] == 0).all()) and bool((bank[:, C:] == 0).all()), "bank padding is not zero"
    # unit rows in fp32: the 1e-5 relative bar the loss built on them is held to (LOSS_RTOL of tests/test_hip_parity.py)
    assert (bank[:T * V, :C].double() - rows / nr[:, None]).abs().max().item() <= 1e-5
    assert torch.allclose(got["nrm"].double(), nr, rtol=1e-5, atol=0)
    halves = got["bank_h"].double()
    assert (halves[:, :256] + halves[:, 256:] - bank.double() * 1024.0).abs().max().item() <= 1024.0 * 2.0 ** -21      # hi + lo: 22 bits


# ---------------------------------------------------------------------------------------------------------------------------------
# Swin window attention

def _attn_ref64(qkv, qkv_bias, bias, B, H, W, heads, shift, scale):
    """the reference data flow of tests/test_window_attention.py on given qkv rows; padded tokens carry qkv_bias"""
    from test_window_attention import _partition, _reverse, _shift_mask
    C = qkv.shape[-1] // 3
    pad_r, pad_b = (7 - W % 7) % 7, (7 - H % 7) % 7
    Hp, Wp = H + pad_b, W + pad_r
    x = F.pad(qkv.view(B, H, W, 3 * C) - qkv_bias, (0, 0, 0, pad_r, 0, pad_b)) + qkv_bias
    if shift:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    win = _partition(x, 7)
    B_, N, _ = win.shape
    q, k, v = win.reshape(B_, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    attn = (q * scale) @ k.transpose(-2, -1) + bias.unsqueeze(0)
    if shift:
        mask = _shift_mask(Hp, Wp, 7, shift, qkv.device, qkv.dtype)
        nW = mask.shape[0]
        attn = (attn.view(B_ // nW, nW, heads, N, N) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, N, N)
    out = (attn.softmax(-1) @ v).transpose(1, 2).reshape(B_, N, C)
    x = _reverse(out, 7, Hp, Wp)
    if shift:
        x = torch.roll(x, shifts=(shift, shift), dims=(1, 2))
    return x[:, :H, :W, :].reshape(B, H * W, C)


@pytest.mark.parametrize("mfma", [3, 0])
@pytest.mark.parametrize("B,H,W,heads,shift", [(2, 9, 5, 1, 3), (2, 14, 21, 3, 3)])
def test_window_attention_footprint(dev, B, H, W, heads, shift, mfma):
    """dcl_winattn_fwd / _bwd on both kernel families: dpad sized by dcl_winattn_npad, dbias_part by dcl_winattn_bwd_waves, the
    absmax buffer exactly 64 floats and equal to max(|dqkv|, |dpad|)."""
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    C = 32 * heads
    g = torch.Generator(device=dev).manual_seed(H * 100 + W + shift)
    qkv = torch.randn(B, H * W, 3 * C, device=dev, generator=g)
    qb = torch.randn(3 * C, device=dev, generator=g) * 0.5
    bias = torch.randn(heads, 49, 49, device=dev, generator=g)
    dout = torch.randn(B, H * W, C, device=dev, generator=g)
    scale = 32 ** -0.5
    rq, rb, rbias = [t.double().requires_grad_(True) for t in (qkv, qb, bias)]
    ref = _attn_ref64(rq, rb, rbias, B, H, W, heads, shift, scale)
    ref.backward(dout.double())
    npad, nwaves = L.dcl_winattn_npad(H, W), L.dcl_winattn_bwd_waves(B, H, W, heads)
    nW = ((H + 6) // 7) * ((W + 6) // 7)
    assert nwaves > 0 and nwaves % heads == 0 and (npad > 0) == bool(H % 7 or W % 7)
    try:
        L.dcl_winattn_set_mfma(mfma)

        def body(ar):
            qg, bg, biasg = ar.inp(qkv, "qkv"), ar.inp(qb, "qkv_bias"), ar.inp(bias, "bias")
            out, lse = ar.out((B, H * W, C), name="out"), ar.out((B, nW, heads, 49), name="lse")
            _lib.check(L.dcl_winattn_fwd(_p(qg), _p(bg), _p(biasg), B, H, W, C, heads, shift, scale, _p(out), _p(lse), st), "dcl_winattn_fwd")
            dqkv, dpad = ar.out((B, H * W, 3 * C), name="dqkv"), (ar.out((B, npad, 3 * C), name="dpad") if npad else None)
            part, gam = ar.out((nwaves, 49, 49), name="dbias_part"), ar.zeros(SLOTS, name="dqkv_amax")
            _lib.check(L.dcl_winattn_bwd(_p(qg), _p(bg), _p(biasg), _p(ar.inp(lse, "lse")), _p(ar.inp(dout, "dout")), B, H, W, C, heads,
                                         shift, scale, _p(dqkv), _p(dpad), _p(part), _p(gam), st), "dcl_winattn_bwd")
            _tag_exact(gam, torch.cat([dqkv.reshape(-1)] + ([dpad.reshape(-1)] if npad else [])), ("dcl_winattn_bwd", B, H, W, heads, mfma))
            outs = dict(out=out, lse=lse, dqkv=dqkv, part=part, gam=gam)
            if npad:
                outs["dpad"] = dpad
            return outs
        got = run_both(dev, body, ("winattn", B, H, W, heads, shift, mfma))
    finally:
        L.dcl_winattn_set_mfma(3)

    def close(a, want, tol, what):          # 2e-6 / 1e-5 of max(1, max): tests/test_window_attention.py
        err = (a.double() - want).abs().max().item()
        assert err <= tol * max(1.0, want.abs().max().item()), (what, err)
    close(got["out"], ref.detach(), 2e-6, "out")
    close(got["dqkv"], rq.grad, 1e-5, "dqkv")
    if npad:
        close(got["dpad"].sum((0, 1)), rb.grad, 1e-5, "dpad")
    close(got["part"].view(nwaves // heads, heads, 49, 49).sum(0), rbias.grad, 1e-5, "dbias")


# ---------------------------------------------------------------------------------------------------------------------------------
# the deferred norm's consumers at the smallest shapes they take

def _pre_conv_run(dev, x, sc, sh, wt, stride, zero, what):
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    n, c, h, w = x.shape
    co = wt.shape[0]
    act = torch.relu(torch.addcmul(sh.view(1, -1, 1, 1), x, sc.view(1, -1, 1, 1)))
    want = F.conv2d(act.double(), wt.double(), stride=stride, padding=1)

    def body(ar):
        wam, _ = _tag_in(ar, wt)
        wp = ar.out(_pack_bytes(co, c, 9), torch.uint8, "wp")
        _lib.check(L.dcl_conv3x3_pack(_p(ar.inp(wt, "w")), co, c, 0, _p(wam), _p(wp), st), "pack")
        xam, xc = _tag_in(ar, act, SLOTS)
        y = ar.out(tuple(want.shape), name="y")
        _lib.check(L.dcl_conv3x3_pre_f16x3(_p(ar.inp(x, "x")), n, c, h, w, _p(wp), co, _p(xam), xc, _p(wam), _p(ar.inp(sc, "pre_sc")),
                                           _p(ar.inp(sh, "pre_sh")), None, _p(y), stride, 0, 0, st), "dcl_conv3x3_pre_f16x3")
        return {"y": y}
    got = run_both(dev, body, what)["y"]
    if zero:
        assert bool((act == 0).all()) and bool((got == 0).all()), (what, "an all-zero operand must give an exactly-zero result")
    else:
        err = _rel(got, want)
        assert err < 3e-6, (what, err)      # bitwise the two-step form (tests/test_pre_norm_conv.py), whose bar is 3e-6
    return act


@pytest.mark.parametrize("stride,shape,both", [(1, (1, 16, 16, 1, 8), True), (1, (2, 16, 32, 9, 40), True), (1, (1, 16, 16, 3, 7), False),
                                               (2, (1, 16, 16, 1, 16), True), (2, (2, 16, 32, 7, 48), True), (2, (1, 16, 16, 3, 7), False)],
                         ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))
def test_pre_norm_consumers_footprint(dev, stride, shape, both):
    """dcl_conv3x3_pre_f16x3 and dcl_wgrad3x3_pre_f16x3 at the smallest shapes *_pre_supported answers 1 for (asserted, so that
    neither entry can drop out unnoticed), at a ragged multi-block shape, and -- the forward alone -- at a width that is no
    multiple of anything; both strides; a map that sends everything to zero gives tag 0 and exactly zero."""
    _lib, L = _lib_()
    n, c, co, h, w = shape
    assert L.dcl_conv3x3_pre_supported(n, c, co, h, w, stride) == 1, shape
    if both:
        assert L.dcl_wgrad3x3_pre_supported(n, c, co, h, w, stride) == 1, shape
        if (h, w) == (1, 8 * stride):       # nothing smaller is taken
            assert L.dcl_wgrad3x3_pre_supported(n, c, co, h, w - 8 * stride, stride) != 1
    g = torch.Generator(device=dev).manual_seed(sum(shape) + stride)
    x = torch.randn(n, c, h, w, device=dev, generator=g) * 2 + 0.7
    sc, sh = torch.rand(c, device=dev, generator=g) + 0.5, torch.randn(c, device=dev, generator=g)
    wt = torch.randn(co, c, 3, 3, device=dev, generator=g) * (2.0 / (9 * c)) ** 0.5
    act = _pre_conv_run(dev, x, sc, sh, wt, stride, False, ("conv pre", shape, stride))
    _pre_conv_run(dev, x, torch.zeros_like(sc), -sh.abs(), wt, stride, True, ("conv pre zero", shape, stride))
    if both:
        ho, wo = ((h - 1) // 2 + 1, w // 2) if stride == 2 else (h, w)
        gy = torch.randn(n, co, ho, wo, device=dev, generator=g) * 3e-5
        tol = 3e-6 if stride == 1 else 2e-6
        _wgrad_run(dev, x, gy, _wgrad_ref(act, gy, stride, 3), stride, 3, tol, ("wgrad pre", shape, stride), pre=(sc, sh, act),
                   counts=(SLOTS, 1))
        zsc, zsh = torch.zeros_like(sc), -sh.abs()
        _wgrad_run(dev, x, gy, None, stride, 3, tol, ("wgrad pre zero", shape, stride), pre=(zsc, zsh, torch.zeros_like(x)),
                   counts=(SLOTS, 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# fused up-sampling + cross-entropy

@pytest.mark.parametrize("n,C,h,w,H,W,align,weighted", [(2, 7, 9, 13, 36, 52, 1, True), (3, 19, 5, 6, 20, 24, 0, False)])
def test_upsample_ce_footprint(dev, n, C, h, w, H, W, align, weighted):
    """dcl_upsample_ce_fwd / _bwd at the two smallest ragged shapes of tests/test_upsample_ce.py: partial is [N * H, 2], out2 two
    floats, pred one byte per pixel."""
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(n * 1000 + C + h)
    z = torch.randn(n, C, h, w, device=dev, generator=g) * 3
    target = torch.randint(0, C + 1, (n, H, W), device=dev, generator=g)           # class C = ignore id
    weight = (torch.rand(C, device=dev, generator=g) + 0.5) if weighted else None
    zr = z.double().requires_grad_(True)
    full = F.interpolate(zr, size=(H, W), mode="bilinear", align_corners=bool(align))
    ref = F.cross_entropy(full, target, weight=None if weight is None else weight.double(), ignore_index=C)
    ref.backward()

    def body(ar):
        zg, tg = ar.inp(z, "z"), ar.inp(target, "target")
        wg = ar.inp(weight, "weight") if weighted else None
        lse, pred = ar.out((n, H, W), name="lse"), ar.out((n, H, W), torch.uint8, "pred")
        partial, out2 = ar.out((n * H, 2), name="partial"), ar.out(2, name="out2")
        _lib.check(L.dcl_upsample_ce_fwd(_p(zg), n, C, h, w, H, W, align, _p(tg), _p(wg), C, _p(lse), _p(pred), _p(partial), _p(out2), st),
                   "dcl_upsample_ce_fwd")
        gscale = ar.inp((1.7 / out2[1:2]).contiguous(), "gscale")
        dz = ar.out((n, C, h, w), name="dz")
        _lib.check(L.dcl_upsample_ce_bwd(_p(zg), n, C, h, w, H, W, align, _p(tg), _p(wg), C, _p(ar.inp(lse, "lse")), _p(gscale), _p(dz), st),
                   "dcl_upsample_ce_bwd")
        return dict(lse=lse, pred=pred, out2=out2, dz=dz)
    got = run_both(dev, body, ("upsample_ce", n, C, h, w))
    # 2e-6 of the loss, 1e-5 of max for the gradient: tests/test_upsample_ce.py
    assert abs(got["out2"][0].item() - ref.item()) <= 2e-6 * abs(ref.item())
    gd, r = got["dz"].double() / 1.7, zr.grad
    assert (gd - r).abs().max().item() <= 1e-5 * r.abs().max().item()
    top2 = full.detach().float().topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-4
    assert torch.equal(got["pred"].long()[clear], full.detach().argmax(1)[clear])


# ---------------------------------------------------------------------------------------------------------------------------------
# the HRNet head: folded norm, tap products

@pytest.mark.parametrize("shape,k,where", [((3, 37, 10, 12), 19, "first"), ((2, 150, 6, 20), 5, "last"), ((1, 10, 1, 4), 32, "neg")])
def test_head_norm_dz_footprint(dev, shape, k, where):
    """dcl_head_norm_dz: dz = wt^T dl + c1 z + c0 in one pass; the absmax buffer is exactly 64 floats and exact."""
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    n, c, h, w = shape
    hw = h * w
    g = torch.Generator(device=dev).manual_seed(sum(shape) + k)
    z = _plant(torch.randn(n, c, hw, device=dev, generator=g) * 2 + 0.7, where)
    dl = torch.randn(n, k, hw, device=dev, generator=g) * 1e-3
    kp = (k + 3) // 4 * 4
    wt = torch.zeros(c, kp, device=dev)
    wt[:, :k] = torch.randn(c, k, device=dev, generator=g)
    c0, c1 = torch.randn(c, device=dev, generator=g) * 1e-3, torch.randn(c, device=dev, generator=g) * 1e-3
    want = torch.einsum("ck,nkp->ncp", wt[:, :k].double(), dl.double()) + c1.double().view(1, c, 1) * z.double() + c0.double().view(1, c, 1)

    def body(ar):
        dz, am = ar.out((n, c, hw), name="dz"), ar.zeros(SLOTS, name="amax")
        _lib.check(L.dcl_head_norm_dz(_p(ar.inp(dl, "dl")), _p(ar.inp(z, "z")), _p(ar.inp(wt, "wt")), _p(ar.inp(c0, "c0")),
                                      _p(ar.inp(c1, "c1")), n, k, c, hw, _p(dz), _p(am), st), "dcl_head_norm_dz")
        _tag_exact(am, dz, ("dcl_head_norm_dz", shape, k))
        return {"dz": dz, "amax": am}
    got = run_both(dev, body, ("head_norm_dz", shape, k))
    assert _rel(got["dz"], want) <= 2e-5, (shape, k)           # tests/test_head_norm_fold.py


def _tapup_ref64(zs, N, Co, H, W, align, channel_major):
    """sum over sources and taps of the shifted bilinear up-sampling of map tap * Co + co (zero outside the image)"""
    y = 0
    for z in zs:
        zz = z.transpose(0, 1) if channel_major else z                       # [N, 9 Co, h, w]
        up = F.pad(F.interpolate(zz, size=(H, W), mode="bilinear", align_corners=bool(align)), (1, 1, 1, 1))
        for tap in range(9):
            ky, kx = tap // 3, tap % 3
            y = y + up[:, tap * Co:(tap + 1) * Co, ky:ky + H, kx:kx + W]
    return y


@pytest.mark.parametrize("align", [1, 0])
@pytest.mark.parametrize("srcs,H,W", [(((1, 1),), 1, 1), (((3, 5), (2, 3)), 12, 20), (((4, 7),), 9, 13)])
def test_tapup_footprint(dev, srcs, H, W, align):
    """dcl_tapup_fwd (one and two sources, plain and accumulating), dcl_tapup_bwd and dcl_tapup_bwd_amax (both backward forms), both
    channel_major layouts, from the smallest size dcl_tapup_supported accepts; dz_amax is exactly one float and exact."""
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    N, Co = 2, 3
    (h0, w0), (h1, w1) = srcs[0], (srcs[1] if len(srcs) > 1 else (0, 0))
    assert L.dcl_tapup_supported(h0, w0, h1, w1, H, W, align) == 1
    g = torch.Generator(device=dev).manual_seed(H * 10 + W)
    dy = _plant(torch.randn(N, Co, H, W, device=dev, generator=g), ("first", "last", "neg")[(H + align) % 3])
    y0 = torch.randn(N, Co, H, W, device=dev, generator=g)
    try:
        for cm in (0, 1):
            zs = [torch.randn((9 * Co, N, h, w) if cm else (N, 9 * Co, h, w), device=dev, generator=g) for (h, w) in srcs]
            zd = [z.double().requires_grad_(True) for z in zs]
            want = _tapup_ref64(zd, N, Co, H, W, align, cm)
            want.backward(dy.double())

            def body(ar):
                zg = [ar.inp(z, "z") for z in zs] + [None]
                y, ya = ar.out((N, Co, H, W), name="y"), ar.io(y0, "y (accumulate)")
                for buf, acc in ((y, 0), (ya, 1)):
                    _lib.check(L.dcl_tapup_fwd(_p(zg[0]), h0, w0, _p(zg[1]), h1, w1, N, Co, H, W, align, cm, _p(buf), acc, st), "dcl_tapup_fwd")
                outs = {"y": y, "ya": ya}
                dyg = ar.inp(dy, "dy")
                for form in (2, 1):
                    L.dcl_tapup_set_bwd_form(form)
                    for i, (h, w) in enumerate(srcs):
                        dz, dz2, am = ar.out(tuple(zs[i].shape), name="dz"), ar.out(tuple(zs[i].shape), name="dz"), ar.zeros(1, name="dz_amax")
                        _lib.check(L.dcl_tapup_bwd(_p(dyg), N, Co, H, W, h, w, align, cm, _p(dz), st), "dcl_tapup_bwd")
                        _lib.check(L.dcl_tapup_bwd_amax(_p(dyg), N, Co, H, W, h, w, align, cm, _p(dz2), _p(am), st), "dcl_tapup_bwd_amax")
                        _tag_exact(am, dz2, ("dcl_tapup_bwd_amax", srcs, H, W, align, cm, form, i))
                        assert torch.equal(dz, dz2)
                        outs[f"dz{form}{i}"], outs[f"am{form}{i}"] = dz, am
                return outs
            got = run_both(dev, body, ("tapup", srcs, H, W, align, cm))
            # 3e-6 / 1e-5 of max: test_head_conv_over_upsampled_matches_fp64
            assert _rel(got["y"], want.detach()) < 3e-6, (srcs, cm)
            assert ((got["ya"].double() - want.detach() - y0.double()).abs().max() / want.detach().abs().max()).item() < 3e-6, (srcs, cm)
            for form in (2, 1):
                for i in range(len(srcs)):
                    assert _rel(got[f"dz{form}{i}"], zd[i].grad) < 1e-5, (srcs, cm, form, i)
    finally:
        L.dcl_tapup_set_bwd_form(2)


# ---------------------------------------------------------------------------------------------------------------------------------
# the InfoNCE sweeps

def _halves(b):
    """(hi | lo) f16 halves of a bank times 2^10: dcl_gather_normalize's bank_h"""
    x = b.double() * 1024.0
    hi = x.to(torch.float16)
    return torch.cat([hi, (x - hi.double()).to(torch.float16)], 1).contiguous()


def _check_grad(got, ref):
    import numpy as np
    scale = max(float(np.abs(ref).max()), 1e-30)
    np.testing.assert_allclose(got, ref, atol=1e-4 * scale, rtol=1e-3)          # GRAD_ATOL_REL of tests/test_hip_parity.py


@pytest.mark.parametrize("f16x3", [False, True])
def test_infonce_sweeps_footprint(dev, oracle, f16x3):
    """Every dcl_infonce_* launch at the sizes of test_c_abi_direct_infonce_cross (N1 = 49, N2 = 30: no multiple of DCL_ROW_TILE or
    DCL_SEG, a class absent from the contrast bank): the fused forward, its three stages, the one-sweep pair, the statistics, the
    slab backward in both directions and -- with f16x3 banks -- the stream-K backward with the slabs of
    dcl_infonce_bwd_streamk_slabs and the workspace of dcl_infonce_bwd_streamk_workgroups."""
    import numpy as np
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    rs = np.random.RandomState(3)
    V1, V2 = 7, 5
    cls1, cls2 = np.array([0, 0, 2, 5, 5, 5, 9]), np.array([0, 2, 2, 9, 9, 11])
    N1, N2 = len(cls1) * V1, len(cls2) * V2
    F1 = rs.randn(N1, 256).astype(np.float32); F1 /= np.linalg.norm(F1, axis=1, keepdims=True)
    F2 = rs.randn(N2, 256).astype(np.float32); F2 /= np.linalg.norm(F2, axis=1, keepdims=True)
    tau = 0.1
    ref_loss, d1, d2 = oracle.cross_loss(F1.astype(np.float64), np.repeat(cls1, V1), F2.astype(np.float64), np.repeat(cls2, V2), tau)

    def ranges(ca, cb, Vb):
        lo = np.array([np.flatnonzero(cb == c)[0] * Vb if (cb == c).any() else 0 for c in ca], np.int32)
        hi = np.array([(np.flatnonzero(cb == c)[-1] + 1) * Vb if (cb == c).any() else 0 for c in ca], np.int32)
        return torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev)
    lo, hi = ranges(cls1, cls2, V2)
    rlo, rhi = ranges(cls2, cls1, V1)

    def bank(Fm):
        return torch.from_numpy(np.concatenate([Fm, np.zeros(((-Fm.shape[0]) % 128, 256), np.float32)])).to(dev)
    A, B = bank(F1), bank(F2)
    N1pad, N2pad = A.shape[0], B.shape[0]
    ns = 2
    ld = (int((hi - lo).max()) + 3) & ~3
    G = int(L.dcl_infonce_bwd_streamk_workgroups(N2, N1)), int(L.dcl_infonce_bwd_streamk_workgroups(N1, N2))
    nsl = int(L.dcl_infonce_bwd_streamk_slabs(N2, N1)), int(L.dcl_infonce_bwd_streamk_slabs(N1, N2))

    def body(ar):
        Ag, Bg = ar.inp(A, "A"), ar.inp(B, "B")
        Ah, Bh = (ar.inp(_halves(A), "Ah"), ar.inp(_halves(B), "Bh")) if f16x3 else (None, None)
        log, hig, rlog, rhig = ar.inp(lo, "rng_lo"), ar.inp(hi, "rng_hi"), ar.inp(rlo, "rev_lo"), ar.inp(rhi, "rev_hi")
        outs = {}
        # the fused forward (f32 banks only)
        zpart, Z, rl, Wt, loss = ar.out(ns * N1pad, name="zpart"), ar.out(N1pad), ar.out(N1pad), ar.out(N1pad), ar.out(1, name="loss")
        _lib.check(L.dcl_infonce_fwd(_p(Ag), N1, V1, _p(Bg), N2, _p(log), _p(hig), 1 / tau, 0, ns, _p(zpart), _p(Z), _p(rl), _p(Wt), _p(loss),
                                     st), "dcl_infonce_fwd")
        outs.update(loss=loss, Z=Z[:N1], rl=rl[:N1], W=Wt[:N1])
        # its three stages
        zp2, Z2, rl2, W2, loss2 = ar.out(ns * N1pad, name="zpart"), ar.out(N1pad), ar.out(N1pad), ar.out(N1pad), ar.out(1, name="loss")
        _lib.check(L.dcl_infonce_zsweep(_p(Ag), N1, V1, _p(Bg), N2, _p(log), _p(hig), 1 / tau, ns, _p(zp2), _p(Ah), _p(Bh), st), "zsweep")
        _lib.check(L.dcl_infonce_possweep(_p(Ag), N1, V1, _p(Bg), N2, _p(log), _p(hig), 1 / tau, 0, _p(ar.inp(zp2, "zpart")), ns, 0, _p(Z2),
                                          _p(rl2), _p(W2), _p(Ah), _p(Bh), st), "possweep")
        _lib.check(L.dcl_infonce_loss(_p(ar.inp(rl2, "rowloss")), _p(log), _p(hig), None, N1, V1, 0, _p(loss2), st), "dcl_infonce_loss")
        outs.update(loss2=loss2, Z2=Z2[:N1], rl2=rl2[:N1], W2=W2[:N1])
        # one sweep that keeps the positives
        zp3, spos = ar.out(ns * N1pad, name="zpart"), ar.out((N1pad, ld), name="spos")
        Z3, rl3, W3 = ar.out(N1pad), ar.out(N1pad), ar.out(N1pad)
        _lib.check(L.dcl_infonce_zsweep_keep(_p(Ag), N1, V1, _p(Bg), N2, _p(log), _p(hig), 1 / tau, ns, _p(zp3), _p(Ah), _p(Bh), _p(spos), ld,
                                             st), "zsweep_keep")
        span = torch.repeat_interleave(hi - lo, V1)
        written = (spos.view(torch.int32) != SENTINEL)
        assert torch.equal(written[:N1], torch.arange(ld, device=dev).view(1, -1) < span.view(-1, 1)) and not bool(written[N1:].any()), \
            "dcl_infonce_zsweep_keep wrote spos outside the positive ranges"
        _lib.check(L.dcl_infonce_pos_finish(_p(spos), ld, N1, V1, _p(log), _p(hig), 1 / tau, 0, int(f16x3), _p(ar.inp(zp3, "zpart")), ns, _p(Z3),
                                            _p(rl3), _p(W3), st), "pos_finish")
        assert torch.equal(zp2, zp3) and torch.equal(Z2, Z3)
        outs.update(Z3=Z3[:N1], rl3=rl3[:N1], W3=W3[:N1])
        # statistics and the slab backward, both directions
        stat = ar.out((N1pad + 1, 4), name="stat")
        _lib.check(L.dcl_infonce_prep_stats(_p(ar.inp(Z2, "Z")), _p(ar.inp(W2, "W")), _p(log), _p(hig), None, N1, V1, 0, 1.0, 1 / tau, None,
                                            _p(stat), st), "dcl_infonce_prep_stats")
        statg = ar.inp(stat, "stat")
        dp1, dp2 = ar.out((ns, N1pad, 256), name="dpart 1"), ar.out((ns, N2pad, 256), name="dpart 2")
        _lib.check(L.dcl_infonce_bwd(_p(Ag), N1, V1, _p(Bg), N2, _p(log), _p(hig), 1 / tau, 0, 1, 0, _p(statg), None, ns, _p(dp1), _p(Ah),
                                     _p(Bh), st), "dcl_infonce_bwd")
        _lib.check(L.dcl_infonce_bwd(_p(Bg), N2, V2, _p(Ag), N1, _p(rlog), _p(rhig), 1 / tau, 0, 0, 1, None, _p(statg), ns, _p(dp2), _p(Bh),
                                     _p(Ah), st), "dcl_infonce_bwd")
        outs.update(stat=stat[:N1], d1=dp1[:, :N1], d2=dp2[:, :N2])
        if f16x3:
            assert G[0] > 0 and G[1] > 0 and nsl[0] in (1, 4, 8) and nsl[1] in (1, 4, 8)
            for name, (X, Xh, n1, v, Y, Yh, n2, l, h_, ur, uc, rstat, cstat, npad, gg, sl) in dict(
                    s1=(Ag, Ah, N1, V1, Bg, Bh, N2, log, hig, 1, 0, statg, None, N1pad, G[1], nsl[1]),
                    s2=(Bg, Bh, N2, V2, Ag, Ah, N1, rlog, rhig, 0, 1, None, statg, N2pad, G[0], nsl[0])).items():
                dout, ws = ar.out((sl, npad, 256), name="dout"), ar.out((gg, 128, 256), name="streamk ws")
                flags = ar.zeros(gg + 1, torch.int32, "flags")
                _lib.check(L.dcl_infonce_bwd_streamk(_p(X), n1, v, _p(Y), n2, _p(l), _p(h_), 1 / tau, 0, ur, uc, _p(rstat), _p(cstat), _p(dout),
                                                     _p(ws), _p(flags), _p(Xh), _p(Yh), st), "dcl_infonce_bwd_streamk")
                assert int(flags[0].item()) == 0, "a stream-K hand-over timed out"
                outs[name] = dout[:, :n1]
        return outs
    got = run_both(dev, body, ("infonce", f16x3))
    import numpy.testing as npt
    npt.assert_allclose(got["loss"].item(), ref_loss, rtol=1e-5)                    # LOSS_RTOL of tests/test_hip_parity.py
    npt.assert_allclose(got["loss2"].item(), ref_loss, rtol=1e-5)
    # the one-sweep pair against the two-sweep pair: test_one_sweep_forward_equals_two_sweep_forward
    assert torch.allclose(got["rl2"], got["rl3"], rtol=2e-6, atol=2e-5) and torch.allclose(got["W2"], got["W3"], rtol=2e-6, atol=1e-9)
    _check_grad(got["d1"].sum(0).cpu().numpy(), d1)
    _check_grad(got["d2"].sum(0).cpu().numpy(), d2)
    if f16x3:
        for name, slab in (("s1", got["d1"]), ("s2", got["d2"])):
            want = slab.sum(0)
            assert (got[name].sum(0) - want).abs().max().item() <= 2e-6 * want.abs().max().item(), name     # test_streamk_backward_...


@pytest.mark.parametrize("where", ["first", "last", "neg"])
def test_normalize_bwd_scatter_footprint(dev, where):
    """dcl_normalize_bwd_scatter on the bank of a guarded dcl_gather_normalize: two slabs summed, the VJP of the normalisation,
    the scatter into a zero-filled map; the absmax buffer is exactly 64 floats and equals max|dfeat|."""
    import ctypes
    _lib, L = _lib_()
    st = _lib.stream_ptr(dev)
    n, C, hw, T, V = 2, 37, 50, 3, 7
    g = torch.Generator(device=dev).manual_seed(4)
    feat = torch.randn(n, C, hw, device=dev, generator=g)
    pb = torch.tensor([0, 1, 1], dtype=torch.int32, device=dev)
    perm = torch.randperm(hw, device=dev, generator=g)
    pix = torch.stack([perm[:V], perm[:V], perm[V:2 * V]]).to(torch.int32)         # unique within an image
    slot = torch.tensor([2, 0, 1], dtype=torch.int32, device=dev)
    Npad = 128
    slabs = [torch.randn(Npad, 256, device=dev, generator=g) for _ in range(2)]
    big = slabs[0].abs().max() * 1.5 + 37.0                     # the largest gradient row: first / last sampled row, or negative
    r, cc, sign = {"first": (0, 0, 1.0), "last": (T * V - 1, C - 1, 1.0), "neg": (T * V // 2, C // 2, -1.0)}[where]
    slabs[0][r, cc] = sign * big
    rows_b = pb.long()[slot.long()][:, None].expand(T, V).reshape(-1)
    rows_p = pix.long()[slot.long()].reshape(-1)
    x = feat.double()[rows_b, :, rows_p]                                           # [T V, C]
    nr = x.norm(dim=1, keepdim=True)
    f = x / nr
    dF = (slabs[0].double() + slabs[1].double())[:T * V, :C]
    dx = (dF - f * (f * dF).sum(1, keepdim=True)) / nr.clamp_min(1e-12)
    want = torch.zeros(n, C, hw, device=dev, dtype=torch.float64)
    want[rows_b, :, rows_p] = dx

    def body(ar):
        fg, pixg, pbg, slg = ar.inp(feat, "feat"), ar.inp(pix, "pix"), ar.inp(pb, "pair_b"), ar.inp(slot, "slot_pair")
        bank, nrm = ar.out((Npad, 256), name="bank"), ar.out(Npad, name="nrm")
        _lib.check(L.dcl_gather_normalize(_p(fg), C * hw, hw, 1, C, _p(pixg), _p(pbg), _p(slg), T, V, _p(bank), _p(nrm), None, st),
                   "dcl_gather_normalize")
        sg = [ar.inp(s, "slab") for s in slabs]
        host = (ctypes.c_void_p * 2)(*[s.data_ptr() for s in sg])
        dfeat, am = ar.zeros((n, C, hw), name="dfeat"), ar.zeros(SLOTS, name="amax")
        _lib.check(L.dcl_normalize_bwd_scatter(host, 2, _p(ar.inp(bank, "bank")), _p(ar.inp(nrm, "nrm")), _p(pixg), _p(pbg), _p(slg), T, V, C,
                                               _p(dfeat), C * hw, hw, 1, _p(am), st), "dcl_normalize_bwd_scatter")
        _tag_exact(am, dfeat, ("dcl_normalize_bwd_scatter", where))
        return {"dfeat": dfeat, "amax": am}
    got = run_both(dev, body, ("normalize_bwd_scatter", where))
    _check_grad(got["dfeat"].cpu().numpy(), want.cpu().numpy())
    assert bool((got["dfeat"][want == 0] == 0).all()), "pixels that were not sampled received a gradient"
