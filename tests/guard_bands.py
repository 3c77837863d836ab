"""Guard bands: a tensor argument placed inside a larger, poisoned arena, and the checks that look at the poison afterwards.

The library's loops hand it row blocks of larger allocations (helper.compress: h.encode(flat[s:e], out=out[s:e]); training.fit:
rows[a:b]).  A call must read and write nothing outside the block it was given.  `framed` builds such a block on purpose:

    view, arena = framed(t, lead, trail, fill)

`arena` is ONE contiguous allocation of lead + t.shape[0] + trail rows (elements, for a 1-D tensor), `view` the contiguous slice
arena[lead : lead + t.shape[0]] that holds a copy of `t` and is what the library is called with.  Every stray access a wrong kernel
could make within `trail` rows behind the block (or `lead` rows in front of it) stays inside the arena: it damages poison, it does
not fault.

fill:
    POISON   the byte 0x5A everywhere (through a uint8 view) -- OUTPUT arenas; assert_guards_intact finds any store to a guard.
    NAN      NaN of the tensor's type (float16: 0x7e00, bfloat16: 0x7fc0 -- torch's quiet NaN; uint8: 0xff) -- INPUT arenas: a
             guard value that reaches a result, even through a multiply by zero, turns it into NaN, which the bit-for-bit comparison
             with the unframed call sees; assert_inputs_untouched finds any store.
    an int   that value -- INDEX inputs (rows / cols of bamd_apply_deltas): the guard entries are VALID indices that point at a guard
             row of the framed output, so an over-read shows as a damaged guard there and never as an out-of-range store.

Guard sizes: `trail` must be at least min_trail(t) = max(160 rows, 4096 bytes), more than one 128-row group, the largest row
granularity of the kernels; framed() refuses less.  trail=None takes exactly that."""
import torch

GUARD_BYTE = 0x5A
POISON = "poison"
NAN = "nan"
MIN_TRAIL_ROWS = 160
MIN_TRAIL_BYTES = 4096


def row_bytes(t):
    n = 1
    for d in t.shape[1:]:
        n *= int(d)
    return n * t.element_size()


def min_trail(t):
    """Fewest trail rows (elements, for 1-D tensors) of a frame around `t`: >= 160 rows and >= 4096 bytes."""
    rb = row_bytes(t)
    return max(MIN_TRAIL_ROWS, -(-MIN_TRAIL_BYTES // rb))


def _bytes(t):
    """The tensor's memory as a flat uint8 view (the tensor must be contiguous)."""
    assert t.is_contiguous()
    return t.reshape(-1).view(torch.uint8)


def poisoned(shape, dtype, device):
    """A fresh tensor whose every byte is GUARD_BYTE: the block of a pure output."""
    t = torch.empty(shape, dtype=dtype, device=device)
    _bytes(t).fill_(GUARD_BYTE)
    return t


def framed(t, lead, trail=None, fill=POISON):
    assert t.dim() >= 1 and lead >= 0
    need = min_trail(t)
    trail = need if trail is None else trail
    assert trail >= need, f"trail of {trail} rows is below the guard minimum of {need} (160 rows and 4096 bytes)"
    n = t.shape[0]
    arena = torch.empty((lead + n + trail,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    if fill == POISON:
        _bytes(arena).fill_(GUARD_BYTE)
    elif fill == NAN:
        if t.dtype.is_floating_point:
            arena.fill_(float("nan"))
        else:
            assert t.dtype == torch.uint8, f"no NaN-like fill for {t.dtype}"
            arena.fill_(0xFF)
    else:
        assert not t.dtype.is_floating_point, "a numeric fill is for index tensors"
        arena.fill_(int(fill))
    view = arena[lead:lead + n]
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() == arena.data_ptr() + lead * row_bytes(t)
    return view, arena


def assert_guards_intact(arena, lead, n, what):
    """Every byte of the arena outside rows lead .. lead + n - 1 is still GUARD_BYTE."""
    rb = row_bytes(arena)
    b = _bytes(arena)
    lo, hi = lead * rb, (lead + n) * rb
    bad = b != GUARD_BYTE
    bad[lo:hi] = False
    count = int(bad.sum())
    if count:
        idx = torch.nonzero(bad).reshape(-1)
        first, last = int(idx[0]) - lo, int(idx[-1]) - lo
        raise AssertionError(f"{what}: {count} guard byte(s) damaged; first at byte offset {first}, last at byte offset {last} relative to the "
                             f"block's first byte (the block is {hi - lo} bytes, rows of {rb} bytes, {lead} lead rows)")


def assert_inputs_untouched(arena, snapshot, what="input"):
    """The whole arena -- guards and block -- equals its snapshot bit for bit (NaN guards compare by their bits)."""
    assert arena.dtype == snapshot.dtype and arena.shape == snapshot.shape, what
    a, s = _bytes(arena), _bytes(snapshot)
    if not torch.equal(a, s):
        idx = torch.nonzero(a != s).reshape(-1)
        es = arena.element_size()
        raise AssertionError(f"{what}: input arena changed: {int(idx.numel())} byte(s), first in element {int(idx[0]) // es}, "
                             f"last in element {int(idx[-1]) // es} of the arena")
