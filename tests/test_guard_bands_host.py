"""tests/guard_bands.py proved on CPU tensors before the GPU tests trust it: a single changed byte in a guard is found and located,
a change inside the block is not reported, and a one-element change anywhere in an input arena is found."""
import re

import pytest
import torch

import guard_bands as gb

# every dtype the GPU guard-band tests frame: tables, codes, int_mask / flags, the index inputs and the histogram counts
DTYPES = (torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.uint8, torch.int32, torch.int64)
SHAPES = ((17, 15), (1, 625), (129,), (1,))
LEADS = (0, 3)


def _block(shape, dtype):
    g = torch.Generator().manual_seed(3)
    if dtype.is_floating_point:
        return torch.rand(shape, generator=g, dtype=torch.float64).to(dtype)
    return torch.randint(0, 100, shape, generator=g).to(dtype)


def _flip(arena, byte):
    b = gb._bytes(arena)
    b[byte] = b[byte] ^ 0x01


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_one_flipped_guard_byte_is_found_and_located(dtype, shape, lead):
    t = _block(shape, dtype)
    n, rb = shape[0], gb.row_bytes(t)
    view, arena = gb.framed(t, lead, None, gb.POISON)
    trail = arena.shape[0] - lead - n
    assert trail >= 160 and trail * rb >= 4096
    assert torch.equal(gb._bytes(view.clone()), gb._bytes(t)) and view.data_ptr() == arena.data_ptr() + lead * rb
    gb.assert_guards_intact(arena, lead, n, "fresh frame")
    lo, hi, end = lead * rb, (lead + n) * rb, arena.numel() * arena.element_size()
    spots = {"first byte of the trail guard": hi, "the arena's last byte": end - 1}
    if lead:
        spots["last byte of the lead guard"] = lo - 1
    for name, byte in spots.items():
        _flip(arena, byte)
        with pytest.raises(AssertionError) as e:
            gb.assert_guards_intact(arena, lead, n, name)
        first, last = (int(v) for v in re.search(r"first at byte offset (-?\d+), last at byte offset (-?\d+)", str(e.value)).groups())
        assert first == last == byte - lo and "1 guard byte(s)" in str(e.value), (name, str(e.value))
        _flip(arena, byte)
        gb.assert_guards_intact(arena, lead, n, "restored")
    # two damaged bytes: the report spans them
    _flip(arena, hi)
    _flip(arena, end - 1)
    with pytest.raises(AssertionError, match=rf"2 guard byte\(s\) damaged; first at byte offset {hi - lo}, last at byte offset {end - 1 - lo} "):
        gb.assert_guards_intact(arena, lead, n, "two")
    _flip(arena, hi)
    _flip(arena, end - 1)
    # bytes of the block itself are the call's to write
    for byte in (lo, hi - 1):
        _flip(arena, byte)
    gb.assert_guards_intact(arena, lead, n, "block bytes changed")


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_one_changed_input_element_is_found(dtype, lead):
    t = _block((17, 15), dtype)
    fill = gb.NAN if dtype.is_floating_point or dtype == torch.uint8 else 5
    view, arena = gb.framed(t, lead, None, fill)
    snap = arena.clone()
    gb.assert_inputs_untouched(arena, snap)              # NaN guards equal their own snapshot (compared by bits)
    guard = arena[lead + 17:]
    if fill == gb.NAN:
        assert bool(torch.isnan(guard).all()) if dtype.is_floating_point else bool((guard == 0xFF).all())
        if dtype == torch.float16:
            assert bool((guard.view(torch.int16) == 0x7E00).all())
        if dtype == torch.bfloat16:
            assert bool((guard.view(torch.int16) == 0x7FC0).all())
    else:
        assert bool((guard == 5).all())
    flat = arena.reshape(-1)
    for el in (0, lead * 15, lead * 15 + 7, (lead + 17) * 15 - 1, (lead + 17) * 15, flat.numel() - 1):
        old = flat[el].clone()
        flat[el] = 1 if dtype == torch.uint8 else 3
        with pytest.raises(AssertionError, match=rf"first in element {el}, last in element {el} "):
            gb.assert_inputs_untouched(arena, snap)
        flat[el] = old
        gb.assert_inputs_untouched(arena, snap)


def test_framed_refuses_thin_guards_and_sizes_them_in_rows_and_bytes():
    assert gb.min_trail(torch.zeros(4, 625)) == 160                      # 2500-byte rows: the row rule decides
    assert gb.min_trail(torch.zeros(4, 15, dtype=torch.float16)) == 160  # 30-byte rows: 4800 bytes
    assert gb.min_trail(torch.zeros(9, dtype=torch.float32)) == 1024     # elements of 4 bytes: the byte rule decides
    assert gb.min_trail(torch.zeros(9, dtype=torch.uint8)) == 4096
    with pytest.raises(AssertionError, match="guard minimum"):
        gb.framed(torch.zeros(4, 24), 0, 159, gb.POISON)
    v, a = gb.framed(torch.zeros(4, 24), 3, 200, gb.POISON)
    assert a.shape == (207, 24) and v.shape == (4, 24)
    p = gb.poisoned((2, 3), torch.float64, "cpu")
    assert bool((gb._bytes(p) == 0x5A).all())
