"""Guarded buffers for the footprint tests (tests/test_kernel_footprint.py): every tensor handed to a kernel sits in the
MIDDLE of one larger allocation, with a band of known bits in front of it and behind it, so that a store (or a load that
enters a result) a few elements outside the tensor is recorded instead of landing in a neighbour unnoticed.  Nothing is
placed at an allocation edge: an overrun of up to ``band`` elements stays inside the allocation and never faults."""
import struct

import torch

SENTINEL = 0x7FC5A5A5                                        # a quiet NaN with a recognisable payload (as int32)
NAN_BITS = 0x7FC00000                                        # input bands, first run: NaN
BIG_BITS = struct.unpack("<i", struct.pack("<f", 1e30))[0]   # input bands, second run: 1e30 (finite, poisons any sum)
BAND = 65536


def guarded(shape, dtype, dev, band=BAND):
    """(view, whole): ``view`` is a contiguous tensor of ``shape`` / ``dtype`` with ``band`` elements (rounded up to whole 16
    bytes, so that the view keeps 16-byte alignment) of the same allocation ``whole`` (int32 words) on either side."""
    item = torch.empty((), dtype=dtype).element_size()
    n = 1
    for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)):
        n *= int(s)
    lead = (band * item + 15) // 16 * 16
    body = n * item
    total = (lead + body + lead + 3) // 4 * 4
    whole = torch.empty(total // 4, dtype=torch.int32, device=dev)
    view = whole.view(torch.uint8)[lead:lead + body].view(dtype).view(shape)
    assert view.data_ptr() % 16 == 0 and view.is_contiguous()
    return view, whole


def fill_bits(t, bits):
    """every 32-bit word of ``t`` (an int32 ``whole``, or a view of 4-byte elements) := bits"""
    (t if t.dtype == torch.int32 else t.view(torch.int32)).fill_(bits)


def _bands(whole, view):
    """the two bands as int32 words (a body that does not end on a word boundary gives up its last partial word to the check of
    the bytes, below) and the up-to-three odd bytes behind such a body"""
    lead = view.data_ptr() - whole.data_ptr()
    end = lead + view.numel() * view.element_size()
    up = (end + 3) // 4 * 4
    return whole[:lead // 4], whole[up // 4:], whole.view(torch.uint8)[end:up], lead, end


def bands_intact(whole, view, bits=SENTINEL):
    """True when every byte of ``whole`` in front of and behind ``view`` still holds the fill pattern ``bits``"""
    front, back, odd, _, end = _bands(whole, view)
    ok = bool((front == bits).all()) and bool((back == bits).all())
    if odd.numel():
        want = torch.tensor([bits], dtype=torch.int32, device=whole.device).view(torch.uint8)[end % 4:]
        ok = ok and torch.equal(odd, want)
    return ok


def first_damage(whole, view, bits=SENTINEL):
    """[first, last damaged band byte as offsets from the view's start, damaged words] for the assertion message"""
    front, back, _, lead, end = _bands(whole, view)
    up = (end + 3) // 4 * 4
    bad = torch.cat([torch.nonzero(front != bits).flatten() * 4 - lead, torch.nonzero(back != bits).flatten() * 4 + up - lead])
    if bad.numel() == 0:
        return None if bands_intact(whole, view, bits) else [end - lead, end - lead + 3, 1]      # the partial word behind the body
    return [int(bad[0]), int(bad[-1]), int(bad.numel())]


def has_sentinel(t):
    """True when a 32-bit word of ``t`` (4- or 8-byte elements, or a byte count in fours) still holds SENTINEL"""
    c = t.contiguous().reshape(-1)
    if c.element_size() % 4:
        c = c.view(torch.uint8)
        c = c[:c.numel() // 4 * 4].clone()
    return bool((c.view(torch.int32) == SENTINEL).any())


def all_sentinel(t):
    return bool((t.contiguous().view(torch.int32) == SENTINEL).all())


class Arena:
    """The buffers of ONE kernel-call sequence.  ``fill`` = the bits of the input bands (NAN_BITS or BIG_BITS)."""

    def __init__(self, dev, fill):
        self.dev, self.fill = dev, fill
        self.items = []                         # (name, whole, view, band bits)

    def _new(self, name, shape, dtype, bits):
        view, whole = guarded(shape, dtype, self.dev)
        fill_bits(whole, bits)
        self.items.append((name or f"#{len(self.items)}", whole, view, bits))
        return view

    def inp(self, t, name=None):
        """an input: data in the body, the run's fill (NaN / 1e30) in the bands"""
        v = self._new(name, tuple(t.shape), t.dtype, self.fill)
        v.copy_(t)
        return v

    def out(self, shape, dtype=torch.float32, name=None):
        """an output or a workspace: sentinel everywhere"""
        return self._new(name, shape, dtype, SENTINEL)

    def io(self, t, name=None):
        """read AND written (accumulators, zero-initialised absmax slots / tickets / counters, running statistics): data in
        the body, sentinel bands"""
        v = self._new(name, tuple(t.shape), t.dtype, SENTINEL)
        v.copy_(t)
        return v

    def zeros(self, n, dtype=torch.float32, name=None):
        return self.io(torch.zeros(n, dtype=dtype, device=self.dev), name)

    def check(self, what=""):
        torch.cuda.synchronize()
        for name, whole, view, bits in self.items:
            assert bands_intact(whole, view, bits), \
                (what, name, tuple(view.shape), "band damaged: [first, last byte offset from the view, words]",
                 first_damage(whole, view, bits))


def run_both(dev, body, what=""):
    """``body(arena)`` issues the calls on buffers of ``arena`` and returns {name: written output (a view or a slice of one)}.
    Run once with NaN and once with 1e30 in the input bands: (i) every band intact, (ii) no sentinel left in an output,
    (iii) outputs finite and bitwise equal between the two runs.  Returns the outputs of the first run."""
    res = []
    for fill in (NAN_BITS, BIG_BITS):
        ar = Arena(dev, fill)
        outs = body(ar)
        ar.check(what)
        got = {}
        for k, v in outs.items():
            assert not has_sentinel(v), (what, k, "output not fully written")
            if v.is_floating_point():
                assert bool(torch.isfinite(v).all()), (what, k, "not finite", "NaN bands" if fill == NAN_BITS else "1e30 bands")
            got[k] = v.clone()
        res.append(got)
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), (what, k, "depends on what lies outside the inputs")
    return res[0]
