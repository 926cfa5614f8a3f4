"""The split-f16 pieces have one definition each (csrc/dcl_f16x3.h, csrc/dcl_common.h), and the wait states between a split and
the MFMA that reads it are checked at build time: tools/split_wait_states.py on hand-written assembly, its place in the Makefile."""
import glob
import importlib.util
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

import mscs_amd  # noqa: F401
from mscs_amd import _lib

TOOL = os.path.join(ROOT, "tools", "split_wait_states.py")
_spec = importlib.util.spec_from_file_location("split_wait_states", TOOL)
sws = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sws)

WRITE = "\tv_fma_mixhi_f16 v7, v19, v88, 0\n"
MFMA = "\tv_mfma_f32_16x16x32_f16 a[0:3], v[20:23], v[4:7], a[0:3]\n"


def kernel(body):
    return "\t.text\n\t.globl\tk\n\t.type\tk,@function\nk:\n" + body + "\ts_endpgm\n.Lfunc_end0:\n"


# (snippet, the distances the scanner must report, in line order)
CASES = {
    "nothing between": (WRITE + MFMA, [0]),
    "s_nop 0 between": (WRITE + "\ts_nop 0\n" + MFMA, [1]),
    "s_nop 1 between": (WRITE + "\ts_nop 1\n" + MFMA, []),
    "two unrelated VALU between": (WRITE + "\tv_add_u32_e32 v30, v31, v32\n\tv_lshl_add_u64 v[92:93], v[48:49], 0, v[92:93]\n" + MFMA, []),
    "one unrelated VALU between": (WRITE + "\tv_lshl_add_u64 v[92:93], v[48:49], 0, v[92:93]\n" + MFMA, [1]),
    "another VGPR range": (WRITE + "\tv_mfma_f32_16x16x32_f16 a[0:3], v[20:23], v[8:11], a[0:3]\n", []),
    "single-register operand": ("\tv_fma_mixlo_f16 v9, v1, v2, 0\n\tv_mfma_f32_32x32x2_f32 a[0:15], v9, v10, a[0:15]\n", [0]),
    "only in the AGPR and C operands": (WRITE + "\tv_mfma_f32_16x16x32_f16 v[4:7], a[4:7], v[8:11], v[4:7]\n", []),
    "branch to the MFMA": (WRITE + "\ts_branch .LBB0_2\n.LBB0_1:\n\tv_mov_b32_e32 v1, v2\n\ts_endpgm\n.LBB0_2:\n" + MFMA, [1]),
    "paths meet: the branch is the shorter one": (WRITE + "\ts_cbranch_vccnz .LBB0_2\n\ts_nop 7\n\ts_nop 7\n.LBB0_2:\n" + MFMA, [1]),
    "back edge": ("\tv_mov_b32_e32 v4, 0\n\ts_nop 7\n.LBB0_1:\n" + MFMA + "\ts_nop 7\n\ts_nop 7\n" + WRITE +
                  "\ts_cbranch_scc1 .LBB0_1\n", [1]),
    "back edge, padded": ("\tv_mov_b32_e32 v4, 0\n.LBB0_1:\n" + MFMA + WRITE + "\ts_nop 0\n\ts_cbranch_scc1 .LBB0_1\n", []),
    "forgotten after the horizon": (WRITE + "\ts_nop 7\n\ts_nop 7\n\ts_nop 0\n" + MFMA, []),
    "nothing carried into the next kernel": (WRITE + "\ts_endpgm\n\t.type\tk2,@function\nk2:\n" + MFMA, []),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_scanner_on_handwritten_assembly(name):
    body, want = CASES[name]
    got = sws.scan(kernel(body))
    assert [f[2] for f in got] == want, got
    lines = kernel(body).splitlines()
    for symbol, line, distance, reg, at in got:
        assert symbol == "k" and lines[line - 1].lstrip().startswith("v_mfma") and lines[at - 1].lstrip().startswith("v_fma_mix")


def test_scanner_as_a_program(tmp_path):
    """symbol, line and distance on stdout, exit status 1 with a finding and 0 without; the threshold is the guide's two states"""
    assert sws.MIN_STATES == 2
    bad, good = tmp_path / "bad.s", tmp_path / "good.s"
    bad.write_text(kernel(WRITE + "\ts_nop 0\n" + MFMA))
    good.write_text(kernel(WRITE + "\ts_nop 1\n" + MFMA))
    r = subprocess.run([sys.executable, TOOL, str(bad)], capture_output=True, text=True)
    assert r.returncode == 1 and re.search(r"bad\.s:7: k: .* 1 wait state", r.stdout), (r.stdout, r.stderr)
    r = subprocess.run([sys.executable, TOOL, str(good)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "", (r.stdout, r.stderr)


DEFINITION = r"^[ \t]*(?:template[^\n]*\n)?[ \t]*__device__[^\n;(]*\b%s\s*\("


def test_one_definition_of_each_split_piece():
    files = sorted(glob.glob(os.path.join(_lib.CSRC_DIR, "*.h")) + glob.glob(os.path.join(_lib.CSRC_DIR, "*.hip")) +
                   glob.glob(os.path.join(_lib.CSRC_DIR, "*.cpp")))
    assert len(files) > 40
    code = {os.path.basename(p): re.sub(r"//[^\n]*|/\*.*?\*/", "", open(p).read(), flags=re.S) for p in files}
    home = {"split8": "dcl_f16x3.h", "split_to_mfma_fence": "dcl_f16x3.h", "split_to_mfma_pad": "dcl_f16x3.h",
            "pow2_scale": "dcl_f16x3.h", "split2": "dcl_f16x3.h", "wave_max": "dcl_common.h"}
    for name, where in home.items():
        # (\w* behind the name: a copy under a suffixed name, as pow2_scale_w and split2w were, counts as a second definition)
        pat = re.compile(DEFINITION % (name + r"\w*"), re.M)
        found = [f for f, c in code.items() for _ in pat.finditer(c) if not (name == "wave_max" and "wave_max_i" in _.group(0))]
        assert found == [where], f"{name}: defined in {found}"
    for f, c in code.items():
        assert f == "dcl_f16x3.h" or "v_fma_mix" not in c, f"{f} writes a split out again"
        assert f == "dcl_f16x3.h" or not re.search(r"exp2f\(fminf\(fmaxf\(floorf\(log2f\(", c), f"{f} writes the operand scale out again"
    # the pattern does find the old private copies
    pat = re.compile(DEFINITION % r"split8\w*", re.M)
    assert pat.search("__device__ __forceinline__ void split8(const float (&v)[8], float s, h8 &hi, h8 &lo)\n{")
    assert re.search(DEFINITION % r"pow2_scale\w*", "__device__ __forceinline__ float pow2_scale_w(float amax)\n{", re.M)
    assert not pat.search("        split8(v, sx, bhi, blo);")


def test_both_compile_rules_run_the_scanner():
    mk = open(os.path.join(_lib.CSRC_DIR, "Makefile")).read()
    assert re.search(r"^SPLIT_CHECK = .*\.\./\.\./tools/split_wait_states\.py$", mk, re.M)
    packed = mk[mk.index("define packed_rule"):mk.index("endef", mk.index("define packed_rule"))]
    generic = mk[mk.index("$(OBJDIR)/%.o: %.hip"):mk.index("$(OBJDIR)/%.o: %.cpp")]
    # each on the assembly the rule writes anyway, the generic one before its temporaries go
    assert re.search(r"^\t@\$\(SPLIT_CHECK\) \$\(OBJDIR\)/\$\(1\)\.pk\.s", packed, re.M) and packed.count("-S --cuda-device-only") == 1
    check = re.search(r"^\t@\$\(SPLIT_CHECK\) \$\(OBJDIR\)/\$\*-hip-amdgcn-amd-amdhsa-\$\(ARCH\)\.s", generic, re.M)
    assert check and generic.count("$(HIPCC)") == 1 and check.start() < generic.index("@rm -f $(OBJDIR)/$*-hip-amdgcn-*")
    assert os.path.join(ROOT, "tools", "split_wait_states.py") == os.path.normpath(os.path.join(_lib.CSRC_DIR, "../../tools/split_wait_states.py"))
