"""The bilinear index arithmetic has one home, csrc/dcl_bilinear.h: a stand-alone sanitized host program holds its source index,
its gather weight and the coverage of its output range to their invariants, and no other file under csrc/ writes the arithmetic
out again."""
import glob
import os
import re
import shutil
import subprocess

from conftest import ROOT

import mscs_amd  # noqa: F401
from mscs_amd import _lib


def test_standalone_bilinear_program_under_sanitizers(tmp_path):
    gxx = shutil.which("g++") or shutil.which("c++")
    cxx = gxx or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    # the sanitizer runtimes inside the program (clang's default): it runs as it is, whatever else the loader brings along
    static = ["-static-libasan", "-static-libubsan"] if gxx else []
    exe = str(tmp_path / "bilinear_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static +
                       ["-I", _lib.CSRC_DIR, os.path.join(ROOT, "tests", "bilinear_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "bilinear ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


# the names the copies went by (and ATen's): outside comments none of them may be defined -- or, which needs a definition, called
LOCAL_COPY = re.compile(r"(?<![\w.>])(src_index|axis_weight|out_range|area_pixel_compute\w*)\s*\(")


def test_no_second_copy_of_the_index_arithmetic():
    files = sorted(glob.glob(os.path.join(_lib.CSRC_DIR, "*.h")) + glob.glob(os.path.join(_lib.CSRC_DIR, "*.hip")) +
                   glob.glob(os.path.join(_lib.CSRC_DIR, "*.cpp")))
    assert os.path.join(_lib.CSRC_DIR, "dcl_bilinear.h") in files and len(files) > 40
    for path in files:
        if os.path.basename(path) == "dcl_bilinear.h":
            continue
        code = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(path).read(), flags=re.S)
        assert not LOCAL_COPY.findall(code), f"{os.path.basename(path)} writes the bilinear index arithmetic out again"
    # the pattern does find a definition and a call of the old form, and not the shared names
    assert LOCAL_COPY.search("__device__ void src_index(const Axis a") and LOCAL_COPY.search("w = axis_weight (ax, o, w, i);")
    assert LOCAL_COPY.search("void out_range(") and LOCAL_COPY.search("float area_pixel_compute_scale(int a")
    assert not LOCAL_COPY.search("dcl_bilinear_src_index(a.scale") and not LOCAL_COPY.search("dcl_bilinear_out_range(")
