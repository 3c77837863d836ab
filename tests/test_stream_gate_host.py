"""tests/stream_gate.py on CPU tensors, before the GPU tests trust it: placeholders are wrong but harmless, scrub inputs are finite and
different, blank outputs are recognised, and the comparison reports (b) and (c) under the run they belong to."""
import pytest
import torch

import stream_gate as sg

FLOATS = (torch.float32, torch.float64, torch.float16, torch.bfloat16)


@pytest.mark.parametrize("dtype", FLOATS, ids=str)
def test_data_placeholder_is_nan_and_scrub_is_finite_and_different(dtype):
    t = torch.rand((129, 7), dtype=torch.float64).to(dtype)
    p, s = sg.placeholder(t), sg.scrubbed(t)
    assert p.shape == t.shape and p.dtype == dtype and bool(torch.isnan(p).all())
    assert s.shape == t.shape and s.dtype == dtype and bool(torch.isfinite(s).all()) and not sg.same_bits(s, t)
    one = torch.full((1,), 0.25, dtype=dtype)
    assert not sg.same_bits(sg.scrubbed(one), one)


def test_harmless_placeholders():
    rows = torch.tensor([5, 128, 77], dtype=torch.int64)
    assert torch.equal(sg.placeholder(rows, "index"), torch.zeros(3, dtype=torch.int64))
    mask = torch.tensor([1, 0, 1], dtype=torch.uint8)
    assert torch.equal(sg.placeholder(mask, "mask"), torch.zeros(3, dtype=torch.uint8))
    with pytest.raises(AssertionError, match="must have ones"):
        sg.placeholder(torch.zeros(3, dtype=torch.uint8), "mask")
    f = torch.rand((2, 24), dtype=torch.float64) + 0.5
    p = sg.placeholder(f, "features")
    assert torch.equal(p[0], torch.zeros(24, dtype=torch.float64)) and torch.equal(p[1], torch.ones(24, dtype=torch.float64))
    for e in (torch.linspace(-60, 60, 41, dtype=torch.float64), torch.linspace(0, 3, 25, dtype=torch.float64).repeat(24, 1)):
        p = sg.placeholder(e, "edges")
        assert bool((p[..., 1:] > p[..., :-1]).all()) and not bool((p == e).any())
    with pytest.raises(AssertionError, match="explicit placeholder kind"):
        sg.placeholder(rows)
    assert sg.scrubbed(rows, "index").sum() == 0


@pytest.mark.parametrize("dtype", FLOATS + (torch.uint8, torch.int64), ids=str)
def test_blank_outputs_and_record_replay(dtype):
    b = sg.blank((17, 3), dtype, "cpu")
    assert sg.same_bits(b, sg.blank((17, 3), dtype, "cpu"))
    assert bool(torch.isnan(b).all()) if dtype.is_floating_point else bool((sg._bytes(b) == 0x5A).all())
    sg._state["record"] = specs = []
    try:
        sg.out((17, 3), dtype, "cpu")
    finally:
        sg._state["record"] = None
    assert specs == [((17, 3), dtype)]
    pre = sg.blank((17, 3), dtype, "cpu")
    sg._state["replay"] = [pre]
    try:
        assert sg.out((17, 3), dtype, "cpu") is pre
        sg._state["replay"] = [pre]
        with pytest.raises(AssertionError, match="other outputs"):
            sg.out((17, 4), dtype, "cpu")
    finally:
        sg._state["replay"] = None


def _bits(a, b, what):
    assert sg.same_bits(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ"


def test_compare_reports_b_and_c():
    want = {"z": torch.rand(5, 3), "flags": torch.ones(4, dtype=torch.uint8)}
    blanks = {k: sg.blank(v.shape, v.dtype, "cpu") for k, v in want.items()}
    ok = []
    sg._compare("warm", {k: v.clone() for k, v in want.items()}, want, blanks, {None: _bits}, ok)
    assert ok == []
    bad = []
    got = {"z": want["z"].clone(), "flags": blanks["flags"].clone()}
    got["z"][2, 1] = float("inf")
    sg._compare("gated", got, want, blanks, {None: _bits}, bad)
    assert {(r, c) for r, c, _ in bad} == {("gated", "b"), ("gated", "c")}
    assert any("1 of 15 elements differ" in m for _, _, m in bad) and any("not finite" in m for _, _, m in bad)
    assert any("still holds its placeholder" in m for _, _, m in bad)
    e = sg.GateFailure("case", bad)
    assert isinstance(e, AssertionError) and e.failed == {("gated", "b"), ("gated", "c")}
    loose = []
    sg._compare("gated", {"z": want["z"] + 1e-9, "flags": want["flags"]}, want, blanks,
                {None: _bits, "z": lambda a, b, what: torch.testing.assert_close(a, b)}, loose)
    assert loose == []


@pytest.mark.parametrize("longest,gate", [(0.59, 200.0), (20.0, 200.0), (35.0, 350.0), (250.0, 1000.0)])
def test_gate_length_rule(longest, gate, monkeypatch):
    """200 ms, or 10 x the longest enqueue time if that is more, never more than 1 s."""
    monkeypatch.setattr(sg, "LONGEST_ENQUEUE_MS", longest)
    assert sg.gate_ms() == gate
