"""Host entries of libdcl_convbwd.so (include/dcl_convbwd.h), no GPU: which shapes the fused convolution backward serves, and its
launch plan -- data-gradient grid padded to a multiple of 8, weight gradient planned for the compute units that remain."""
import os
import re

import pytest

import mscs_amd  # noqa: F401
from mscs_amd import _lib
from mscs_amd import _lib_convbwd as cb                                    # (the feature: this import fails without it)

# the two shapes of the HRNet-W48 step at batch 12 x 512 x 1024 the launch is for: (N, C, H, W), C -> C
BENCH = [(12, 192, 32, 64), (12, 384, 16, 32)]


def test_library_and_makefile_entry():
    assert os.path.exists(cb.LIB_PATH) and os.path.basename(cb.LIB_PATH) == "libdcl_convbwd.so"
    assert cb.lib().dcb_version() == 1
    mk = open(os.path.join(_lib.CSRC_DIR, "Makefile")).read()
    assert "CB.convbwd" in re.search(r"^SATELLITES = (.*)$", mk, re.M).group(1)
    assert "$(OUT_CB)" in re.search(r"^all: (.*)$", mk, re.M).group(1) and "$(OUT_CB)" in re.search(r"^\trm -rf (.*)$", mk, re.M).group(1)
    hdr = open(os.path.join(os.path.dirname(_lib.CSRC_DIR), "..", "include", "dcl_convbwd.h")).read()
    assert set(re.findall(r"\b(dcb_\w+)\s*\(", hdr)) == set(cb.SIGNATURES) | {"dcb_last_error"}


@pytest.mark.parametrize("pre", [False, True])
def test_supported_shapes(pre):
    for n, c, h, w in BENCH:
        assert cb.supported(n, c, c, h, w, pre)


def test_refused_shapes():
    assert cb.lib().dcb_supported(12, 192, 192, 32, 64, 0) == 1
    # stride 2: the entries carry no stride (3x3 / stride 1 / pad 1 is all they do), and the dispatch asks for stride 1 only
    from mscs_amd.models import ops_conv
    src = open(ops_conv.__file__).read()
    assert re.search(r"ctx\.stride == 1\s*\\?\s*and conv3x3_bwd_fused_applies", src)
    assert not cb.supported(12, 200, 192, 32, 64)              # Cin % 16 != 0
    assert not cb.supported(12, 192, 200, 32, 64)              # Cout % 16 != 0
    assert not cb.supported(12, 192, 192, 32, 60)              # W % 8 != 0
    assert not cb.supported(12, 48, 48, 128, 256)              # the 48-channel branch: (2, 2) tiles, two workgroups per CU
    assert not cb.supported(12, 96, 96, 64, 128)               # the 96-channel branch: 192 data-gradient tiles
    assert not cb.supported(0, 192, 192, 32, 64) and not cb.supported(12, 192, 192, 0, 64)
    assert cb.plan(12, 192, 192, 32, 64, 2, 2) is None         # a forced tile the fused kernel is not built for
    assert cb.plan(12, 192, 192, 32, 64, 0, 0, 100) is None    # workgroup target: multiples of 8 in [32, 256]
    assert cb.plan(12, 192, 192, 32, 64, 0, 0, 264) is None
    assert b"not taken" in cb.lib().dcb_last_error()


@pytest.mark.parametrize("shape", BENCH, ids=lambda s: "x".join(map(str, s)))
def test_automatic_plan_fits_one_round(shape):
    n, c, h, w = shape
    p = cb.plan(n, c, c, h, w)
    assert p["nd"] == 96 and p["nd8"] % 8 == 0 and p["nd"] <= p["nd8"] < p["nd"] + 8
    assert (p["tile_r"], p["tile_p"]) == ((3, 4) if c == 192 else (3, 2))
    assert p["wg_target"] == cb.CUS - p["nd8"] >= cb.CUS // 2
    assert p["nd8"] + p["wgrad_grid"] <= cb.CUS
    assert p["wgrad_grid"] > cb.CUS // 2                       # and the weight gradient does use what is left
    assert cb.wgrad_splits(n, c, c, h, w) == p["slabs"] > 0
    assert bool(p["wave_mode"]) == (c == 384)
    # slabs: one per workgroup of a pair (flat form: 160 // 48 pairs), one per wave-level split (wave form: 80 waves of an XCD
    # over its 24 pairs)
    assert p["slabs"] == 3
    assert p["wgrad_grid"] == (144 if c == 192 else 160)


@pytest.mark.parametrize("shape", BENCH + [(3, 96, 20, 40), (1, 384, 8, 16)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("tile_p", [4, 2])
def test_target_256_is_the_separate_plan(shape, tile_p):
    n, c, h, w = shape
    p = cb.plan(n, c, c, h, w, 3, tile_p, 256)
    assert p is not None and p["wg_target"] == 256 and p["nd8"] % 8 == 0
    assert p["slabs"] == cb.wgrad_splits(n, c, c, h, w, 3, tile_p, 256) == _lib.lib().dcl_wgrad3x3_splits(n, c, c, h, w, 1)
    q = cb.plan(n, c, c, h, w, 3, tile_p, 0)                   # automatic target with the same forced tile
    assert q["slabs"] == cb.wgrad_splits(n, c, c, h, w, 3, tile_p, 0) and q["wg_target"] in (cb.CUS - q["nd8"], cb.CUS)


def test_small_test_shapes_have_padding_workgroups():
    """the shapes of tests/test_convbwd.py: data-gradient grids that are no multiple of 8, 6 x 2 tile pairs / the wave form"""
    for tp, nd in ((4, 12), (2, 18)):
        p = cb.plan(3, 96, 96, 20, 40, 3, tp)
        assert p["nd"] == nd and p["nd8"] == (nd + 7) // 8 * 8 != nd and not p["wave_mode"]
        assert p["wgrad_grid"] % 12 == 0 and p["slabs"] == p["wgrad_grid"] // 12
    p = cb.plan(1, 384, 384, 8, 16, 3, 2)
    assert p["nd"] == 4 and p["nd8"] == 8 and p["wave_mode"] == 2 and p["wgrad_grid"] == 2 * (p["wg_target"] // 2)


def test_missing_library_raises(monkeypatch):
    monkeypatch.setattr(cb, "LIB_PATH", os.path.join(os.path.dirname(cb.LIB_PATH), "no_such_dir", "libdcl_convbwd.so"))
    monkeypatch.setattr(cb, "_lib", None)
    assert not cb.built()
    with pytest.raises(Exception, match="libdcl_convbwd"):
        cb.lib()
