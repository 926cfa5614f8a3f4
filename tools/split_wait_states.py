#!/usr/bin/env python3
"""Wait states between a split and the MFMA that reads it, checked on device assembly.

    python tools/split_wait_states.py build/dcl_dconv-hip-amdgcn-amd-amdhsa-gfx950.s

The split-f16 helpers (csrc/dcl_f16x3.h) are inline-asm v_fma_mix{lo,hi}_f16.  The compiler does not model what is inside an asm
statement, so it pads nothing between such a write and a v_mfma* that reads the register as its A or B operand.  This script
reports every v_mfma* that reads a VGPR a v_fma_mix* wrote fewer than MIN_STATES wait states earlier, and exits 1 if there is one.
The Makefile runs it on the assembly every compile rule already writes.

A wait state is one issued instruction; s_nop N is N + 1 of them.  Pending writes are carried across fall-through and along every
branch to its target (back edges included); where paths meet, the smallest distance holds.
"""
import re
import sys

# CDNA HIP kernel programming guide, section 5.7 ("what hipcc does not do for an asm statement"), item 2: "a just-written "v"
# operand or v_accvgpr_write -> MFMA operand (s_nop 1)", i.e. two wait states.
MIN_STATES = 2
HORIZON = 16            # a write this many states back is forgotten

_LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
_VGPR = re.compile(r"^v(?:(\d+)|\[(\d+):(\d+)\])$")


def _operands(rest):
    """Comma-separated operands, brackets kept whole; trailing modifiers stay glued to the last one."""
    out, depth, cur = [], 0, ""
    for ch in rest:
        depth += ch == "["
        depth -= ch == "]"
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    out.append(cur.strip())
    return out


def _vgprs(op):
    m = _VGPR.match(op.split()[0]) if op else None
    if not m:
        return ()                                   # an AGPR, an SGPR, a constant
    return (int(m.group(1)),) if m.group(1) else tuple(range(int(m.group(2)), int(m.group(3)) + 1))


def _parse(text):
    """-> [(line number, "label" | "insn", name, operands)]"""
    items = []
    for no, raw in enumerate(text.splitlines(), 1):
        line = raw.split(";")[0].split("//")[0].strip()
        if not line:
            continue
        m = _LABEL.match(line)
        if m:
            items.append((no, "label", m.group(1), ()))
            line = line[m.end():].strip()
            if not line:
                continue
        if line.startswith("."):
            continue                                # a directive
        name, _, rest = line.partition(" ")
        items.append((no, "insn", name, _operands(rest.strip()) if rest.strip() else []))
    return items


def _merge(into, state):
    """min-merge state into into; True if into changed"""
    changed = False
    for reg, (d, at) in state.items():
        if reg not in into or d < into[reg][0]:
            into[reg] = (d, at)
            changed = True
    return changed


def scan(text):
    """-> sorted [(symbol, line of the MFMA, distance, VGPR number, line of the write)], the smallest distance per MFMA."""
    items = _parse(text)
    arriving = {}                                   # label -> pending writes carried there by branches
    found = {}                                      # MFMA line -> finding
    changed = True
    while changed:
        changed = False
        symbol, state = "?", None                   # state: VGPR -> (states since the write, its line); None = not reachable
        for no, kind, name, ops in items:
            if kind == "label":
                if not name.startswith(".L"):       # a function: nothing is pending on entry
                    symbol, state = name, {}
                    continue
                merged = dict(state or {})
                _merge(merged, arriving.get(name, {}))
                state = merged if (state is not None or name in arriving) else None
                continue
            if state is None:
                continue
            if name.startswith("v_mfma") and len(ops) >= 3:
                hits = [(state[r][0], r, state[r][1]) for op in ops[1:3] for r in _vgprs(op) if r in state]
                if hits and min(hits)[0] < MIN_STATES:
                    d, reg, at = min(hits)
                    if no not in found or d < found[no][2]:
                        found[no] = (symbol, no, d, reg, at)
            states = int(ops[0], 0) + 1 if name == "s_nop" and ops else 1
            state = {r: (d + states, at) for r, (d, at) in state.items() if d + states <= HORIZON}
            if name.startswith("v_fma_mix") and ops:
                for r in _vgprs(ops[0]):
                    state[r] = (0, no)
            if name.startswith(("s_branch", "s_cbranch")) and ops:
                changed |= _merge(arriving.setdefault(ops[0], {}), state)
            if name.startswith(("s_branch", "s_endpgm", "s_setpc")):
                state = None
    return sorted(found.values(), key=lambda f: f[1])


def main(argv):
    if len(argv) != 2:
        print(__doc__)
        return 2
    findings = scan(open(argv[1]).read())
    for symbol, no, d, reg, at in findings:
        print(f"{argv[1]}:{no}: {symbol}: v_mfma reads v{reg} {d} wait state(s) after the v_fma_mix of line {at} "
              f"(minimum {MIN_STATES}: dcl_f16x3.h, split_to_mfma_fence / split_to_mfma_pad)")
    return 1 if findings else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
