"""Footprint of dve_evaluate at the C ABI (include/dcl_eval.h) on guarded buffers (tests/_footprint.py): every band around ids, the
matrix and the out-of-range counter intact, ids fully written, and nothing that depends on what lies outside the logits, the label
or the table; at widths that force the byte-wise stores, at one that takes the 4-byte stores, and on an ids map that starts 1, 2
and 3 bytes off a 4-byte boundary.  The values are those of utils/evaluate.py on torch-allocated buffers."""
import pytest
import torch

from _footprint import SENTINEL, bands_intact, fill_bits, first_damage, guarded, run_both

import _eval_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_eval
    _lib_eval.lib()
    return torch.device("cuda:0")


CASES = [cases.CASES[0],         # W0 = 55: byte by byte, a tail of three; C = 150: classes in slices, global atomics
         cases.CASES[5],         # W0 = 96: 4-byte stores; C = 19: the LDS histogram
         cases.CASES[2],         # dense input, W0 = 70: a tail of two
         cases.CASES[3],         # C = 256, W0 = 22
         cases.CASES[6],         # both stages the identity
         cases.CASES[8]]         # an output of one pixel


def _call(le, dev, case, z, label, lut, cols, cm, oob, ids):
    C, h, w, a1, Hp, Wp, rh, rw, H0, W0, a2 = case
    p = lambda t: None if t is None else t.data_ptr()                                   # noqa: E731
    le.check(le.lib().dve_evaluate(z.data_ptr(), C, h or Hp, w or Wp, Hp, Wp, a1, rh, rw, H0, W0, a2, p(label),
                                   label.element_size() if label is not None else 0, p(lut), cols, p(cm), p(oob), p(ids),
                                   le.stream_ptr(dev)), "dve_evaluate")


@pytest.mark.parametrize("case", CASES, ids=cases.case_id)
def test_evaluate_footprint(dev, case):
    from mscs_amd import _lib_eval as le
    from mscs_amd.utils import evaluate_at_original
    C, H0, W0 = case[0], case[8], case[9]
    cols = C + 1 if C in (19, 150) else C
    z = cases.logits(case).to(dev)
    table = cases.lut()
    table[:cols] = torch.arange(cols, dtype=torch.int64).to(torch.uint8)[:256]         # raw id v < cols is class v; the rest: random
    raw = torch.randint(0, 256, (H0, W0), generator=torch.Generator().manual_seed(H0 * W0), dtype=torch.uint8)
    wide = table[raw.long()].long()                                                     # the same targets as int64

    def body(ar):
        zg, rg, tg, wg = ar.inp(z, "z"), ar.inp(raw.to(dev), "label u8"), ar.inp(table.to(dev), "lut"), ar.inp(wide.to(dev), "label i64")
        ids = ar.out((H0, W0), torch.uint8, "ids")
        cm, oob = ar.zeros((C, cols), torch.int32, "cm"), ar.zeros((1,), torch.int32, "oob")
        _call(le, dev, case, zg, rg, tg, cols, cm, oob, ids)
        only = ar.out((H0, W0), torch.uint8, "ids alone")
        _call(le, dev, case, zg, None, None, cols, None, None, only)
        cm64, oob64 = ar.zeros((C, cols), torch.int32, "cm i64"), ar.zeros((1,), torch.int32, "oob i64")
        _call(le, dev, case, zg, wg, None, cols, cm64, oob64, None)
        return {"ids": ids, "cm": cm, "oob": oob, "only": only, "cm64": cm64, "oob64": oob64}
    got = run_both(dev, body, ("eval", case))

    assert torch.equal(got["only"], got["ids"]) and torch.equal(got["cm64"], got["cm"]) and torch.equal(got["oob64"], got["oob"])
    want, bad = cases.bincount_cm(got["ids"], wide, C, cols)
    assert torch.equal(got["cm"].cpu().long(), want) and int(got["oob"].item()) == bad
    cm, ids = evaluate_at_original(cases.wrap(z, case), raw.to(dev), case[6:8], (H0, W0), bool(case[10]), "ADE20K" if C == 150 else
                                   "CITYSCAPES", label_lut=table, return_ids=True)
    assert torch.equal(ids[0], got["ids"]) and torch.equal(cm, got["cm"][:, :C])


@pytest.mark.parametrize("shift", (1, 2, 3))
def test_ids_off_the_word_boundary(dev, shift):
    """W0 is a multiple of the run, but ids starts 1, 2 or 3 bytes off a 4-byte boundary: byte stores, the same values, and the
    bytes in front of and behind the map unchanged."""
    from mscs_amd import _lib_eval as le
    case = cases.CASES[5]
    C, H0, W0 = case[0], case[8], case[9]
    assert W0 % le.RUN == 0 and le.plan_runs(W0, 16) == (W0 // 4, True) and le.plan_runs(W0, 16 + shift) == (W0 // 4, False)
    z = cases.logits(case).to(dev)
    n = H0 * W0
    view, whole = guarded((n + 4,), torch.uint8, dev)
    fill_bits(whole, SENTINEL)
    body = view[shift:shift + n]
    _call(le, dev, case, z, None, None, C + 1, None, None, body)
    ref = torch.empty(H0, W0, dtype=torch.uint8, device=dev)
    _call(le, dev, case, z, None, None, C + 1, None, None, ref)                         # word stores
    torch.cuda.synchronize()
    pattern = torch.tensor([SENTINEL], dtype=torch.int32, device=dev).view(torch.uint8)
    assert bands_intact(whole, view), first_damage(whole, view)
    assert torch.equal(body, ref.reshape(-1))
    assert torch.equal(view[:shift], pattern[:shift])                                   # (the view starts on a 16-byte boundary)
    tail = view[shift + n:]
    assert torch.equal(tail, pattern.repeat(2)[(shift + n) % 4:][:tail.numel()])
