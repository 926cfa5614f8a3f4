#!/usr/bin/env python3
"""Per-kernel resource and instruction-mix table of device assembly files, for before / after comparisons of a refactor.

    make -C <pkg>/csrc dcl_wgrad3x3.s            (at both commits; PACKED units: build/<unit>.pk.s)
    tools/isa_table.py OLD_DIR NEW_DIR unit.s [unit.s ...]

One row per kernel symbol: vgpr / sgpr / scratch bytes / LDS bytes / kernarg bytes, then the counts of v_mfma*, global_load*,
ds_read* + ds_write*, v_fma_mix* and all instructions -- old value, and "-> new" where it differs.  Exit status 1 if a resource
count or one of the four instruction classes differs anywhere (kernarg size and the total are reported, not judged).
The parser relies on the metadata layout of the ROCm 7 hipcc it was written against (.wavefront_size closes a kernel's entry)."""
import re
import subprocess
import sys

CLASSES = (("mfma", r"v_mfma"), ("gload", r"global_load"), ("ds", r"ds_(read|write)"), ("mix", r"v_fma_mix"))
META = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "kernarg_segment_size")


def parse(path):
    kernels, cur = {}, None
    meta, name_of = {}, {}
    m_cur = {}
    for line in open(path, errors="replace"):
        s = line.strip()
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", s)
        if m and not s.startswith("."):
            cur = m.group(1)
            kernels[cur] = dict.fromkeys([c for c, _ in CLASSES] + ["insts"], 0)
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur and s and s[0] not in ".;" and not s.endswith(":"):
            kernels[cur]["insts"] += 1
            for c, rx in CLASSES:
                if re.match(rx, s):
                    kernels[cur][c] += 1
        m = re.match(r"^-?\s*\.(\w+):\s+(\S+)$", s)
        if m:
            k, v = m.groups()
            if k == "name":
                m_cur["name"] = v
            elif k in META:
                m_cur[k] = int(v)
            elif k == "wavefront_size":       # last key of a kernel's metadata entry
                if "name" in m_cur:
                    meta[m_cur["name"]] = m_cur
                m_cur = {}
    return {k: {**v, **{f: meta.get(k, {}).get(f, -1) for f in META}} for k, v in kernels.items() if k in meta}


def main():
    old_dir, new_dir, units = sys.argv[1], sys.argv[2], sys.argv[3:]
    cols = list(META) + [c for c, _ in CLASSES] + ["insts"]
    judged = set(cols) - {"kernarg_segment_size", "insts"}
    bad = 0
    print("# kernel | " + " | ".join(c.replace("_segment_fixed_size", "").replace("_segment_size", "") for c in cols))
    for u in units:
        a, b = parse(f"{old_dir}/{u}"), parse(f"{new_dir}/{u}")
        print(f"## {u}: {len(a)} kernels before, {len(b)} after" + ("" if a.keys() == b.keys() else "  SYMBOLS DIFFER"))
        bad += a.keys() != b.keys()
        names = subprocess.run(["c++filt"], input="\n".join(sorted(a)), capture_output=True, text=True).stdout.split("\n")
        for sym, nm in zip(sorted(a), names):
            if sym not in b:
                continue
            nm = re.sub(r"^\(anonymous namespace\)::|\(.*\)$|^void ", "", nm.replace("void (anonymous namespace)::", ""))
            cells = []
            for c in cols:
                x, y = a[sym][c], b[sym][c]
                cells.append(str(x) if x == y else f"{x} -> {y}")
                bad += x != y and c in judged
            print(f"{nm} | " + " | ".join(cells))
    print("# resources and instruction classes identical" if not bad else f"# {bad} DIFFERENCES in judged columns")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
