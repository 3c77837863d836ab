"""Stream gates: a sequence of library calls issued on a side stream that is held back by a device sleep, and the checks that show whether
every launch of the sequence really ran on, and only on, that stream, and whether anything made the host wait.

include/baler_amd.h promises that all work of a call is enqueued asynchronously on the caller's stream and that nothing synchronises
the host.  On the default stream neither half can be seen: a helper launch that went to stream 0 is still ordered correctly there, and a
hidden hipStreamSynchronize costs nothing when the stream is empty.  `run_gated` makes both visible:

    S = free_side_stream()                # a non-blocking side stream: no implicit order against stream 0, and a hardware queue of its own
    on S:   gate                          # torch.cuda._sleep: a fixed-length device sleep, it always ends by itself
            gate_end.record()
            staged[k].copy_(ins[k])       # the true inputs arrive BEHIND the gate; until then `staged` holds placeholders
            outs = seq(staged)            # the library calls under test
            host_waited = gate_end.query()        # True: the gate is over, so something in seq made the host wait for the stream
            clones of every output and in/out tensor          # the consumer on the caller's stream

A launch that left S runs at once, while the gate still sleeps: it reads placeholders (or workspaces the preceding scrub run left wrong)
and what it writes differs from the reference, or it reads an output that the sequence has not written yet.  Three runs of `seq`, each
after reset() and the scrub runs, so that each starts from the same state -- in this order:

    gated   as above, FIRST: the library meets the true inputs behind the gate for the first time
    plain   on the default stream; its outputs are the reference bits
    warm    on S, ungated: bit for bit equal to plain; the host side of seq is timed and held to a tenth of the gate

Assertions, reported together in one GateFailure (an AssertionError; .failed holds (run, letter) pairs):
    (a) host_waited is False;
    (b) every clone equals plain bit for bit (`same`: another comparison for the named outputs -- bamd_column_moments sums with atomics);
    (c) no clone still equals its placeholder and every floating-point clone is finite, so that (b) is not vacuous.

The scrub runs: seq, ungated, over finite inputs that differ from the true ones (scrubbed()), after reset() has loaded another
parameter vector -- on the stream of the coming run (per-stream scratch, workspace growth and the output shapes are met here), then once
more on the default stream.  They leave the handle's parameter copy, weight fragments and workspaces and the per-stream scratch of the
handle-free kernels holding WRONG finite data, so that a launch that runs early computes on wrong data.

Why the gated run comes first, and why the second scrub.  With the order plain, warm, gated and one scrub on S, a library copy whose
converting launch of bamd_encode (float32 workspace -> 16-bit codes) went to stream 0 passed unseen in 9 of the 45 cases that reach
that launch, all of them single-chunk.  The cause: the stray launch defeats the scrub as well.  The warm run leaves the workspace
holding the true codes (decode widens the float16 codes into it).  In the scrub run on S the stray launch runs AHEAD of the encode
kernel of its own call, converts those stale true codes into the scrub's float16 output, and the scrub's decode widens them back into
the workspace: the true codes survive the scrub, the stray launch of the gated run converts them early, and the result is right.  A
stray launch can carry stale values across any number of runs on S.  So (1) the gated run comes before any run on the true inputs:
until the gate ends nothing on the device derives from them, whatever the library does with its streams; and (2) the last scrub runs
on the default stream, where a launch that strays to stream 0 is in order and the workspaces end up holding what the scrub inputs give.
With both, that library copy fails (b) in its gated run in 45 of 45 cases and in no other case.

Stream 0 must be free to run on while S sleeps.  The runtime maps streams to a few hardware queues (4 by default), and about one side
stream of torch's pool in four shares the default stream's: a launch that left S for stream 0 then queues behind the gate like
everything else, and the result is right.  free_side_stream() takes a stream behind whose short sleep a default-stream launch is seen
to finish; the gated run repeats that check with a launch on stream 0 right after the gate is enqueued -- if it queued behind the
gate, nothing true has been staged yet and another stream is taken -- and once more after the sequence, which must hold.

Outputs are taken from out(): in the gated run these tensors are allocated and filled (NaN; 0x5A bytes for integer types) BEFORE the
gate, so a reader that runs early meets the fill and not a recycled block that happens to hold the values of an earlier run.

Placeholders (placeholder()) are wrong but harmless -- a mis-ordered launch computes a wrong answer and cannot fault:
    "data"      NaN (rows, codes, gradients, parameters, Adam state, prior / projections, binary16 deltas)
    "index"     zeros: valid indices (rows / cols of bamd_apply_deltas)
    "features"  [0 ; 1] (min ; range of a (2, n_cols) float64 features / renorm tensor)
    "mask"      zeros, where the true int_mask has ones
    "edges"     edges * 0.5 - 7: strictly increasing, different from the true histogram edges

Gate length: 200 ms, or 10 x the longest host-side enqueue time of any sequence of tests/test_gpu_streams.py if that is more, and never
more than 1 s.  Measured on an MI355X with the library of the commit before this module (warm run, host time of seq): the longest is
0.59 ms, PJ_Conv_AE (pjconv-z10, routing lat32-64); every other sequence is under 0.5 ms.  10 x 0.59 ms is far below 200 ms, so the gate
stays at 200 ms (LONGEST_ENQUEUE_MS below; gate_ms() applies the rule, and run_gated asserts that the warm run's host time is at most a
tenth of the calibrated gate, so the figure cannot go stale unnoticed).
Cycles -> milliseconds are calibrated once per session with two events around one sleep, and the gate that results is measured."""
import time

import torch

GATE_TARGET_MS = 200.0
GATE_MAX_MS = 1000.0
LONGEST_ENQUEUE_MS = 0.59     # pjconv-z10 lat32-64; see the docstring
STREAM_TRIES = 8

_cal = {}
_state = {"record": None, "replay": None}


def gate_ms():
    return min(GATE_MAX_MS, max(GATE_TARGET_MS, 10.0 * LONGEST_ENQUEUE_MS))


class GateFailure(AssertionError):
    def __init__(self, what, failures):
        self.failed = {(run, letter) for run, letter, _ in failures}
        super().__init__(f"{what}: " + "; ".join(f"[{run} ({letter})] {msg}" for run, letter, msg in failures))


# ---- the gate --------------------------------------------------------------------------------------------------------------------
def _timed_sleep(stream, cycles):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        torch.cuda._sleep(int(cycles))
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def calibration():
    """{"cycles_per_ms", "gate_cycles", "gate_ms" (measured)}, made once per session."""
    if not _cal:
        s = torch.cuda.Stream()
        _timed_sleep(s, 1_000_000)
        per_ms, cycles = None, 4_000_000
        for _ in range(8):                         # a sleep long enough to time: at least 5 ms
            ms = _timed_sleep(s, cycles)
            if ms >= 5.0:
                per_ms = cycles / ms
                break
            cycles *= 4
        assert per_ms, "torch.cuda._sleep could not be calibrated"
        gate_cycles = int(per_ms * gate_ms())
        got = _timed_sleep(s, gate_cycles)
        assert 0.75 * gate_ms() <= got <= GATE_MAX_MS, f"the calibrated gate measures {got:.1f} ms (target {gate_ms():.0f} ms)"
        _cal.update(cycles_per_ms=per_ms, gate_cycles=gate_cycles, gate_ms=got)
        print(f"\n[stream gate] calibration: {per_ms:.0f} cycles per ms; gate of {gate_cycles} cycles measures {got:.1f} ms")
    return _cal


# ---- tensors ---------------------------------------------------------------------------------------------------------------------
def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bytes(a), _bytes(b))


def blank(shape, dtype, device="cuda"):
    """The fill of an output that nothing has written yet: NaN, or the byte 0x5A for integer types."""
    t = torch.empty(tuple(shape), dtype=dtype, device=device)
    if dtype.is_floating_point:
        t.fill_(float("nan"))
    else:
        t.reshape(-1).view(torch.uint8).fill_(0x5A)
    return t


def out(shape, dtype, device="cuda"):
    """An output tensor for a sequence.  Plain / warm / scrub runs: a fresh blank().  Gated run: the next of the blanks that run_gated
    made before the gate (same order, shape and dtype as in the plain run)."""
    shape = tuple(int(d) for d in shape)
    if _state["replay"] is not None:
        t = _state["replay"].pop(0)
        assert tuple(t.shape) == shape and t.dtype == dtype, "the sequence asks for other outputs than in its plain run"
        return t
    if _state["record"] is not None:
        _state["record"].append((shape, dtype))
    return blank(shape, dtype, device)


KINDS = ("data", "index", "features", "mask", "edges")


def _kind(t, kind):
    if kind is None:
        kind = "data" if t.dtype.is_floating_point else None
    assert kind in KINDS, f"an input of dtype {t.dtype} needs an explicit placeholder kind"
    return kind


def placeholder(t, kind=None):
    kind = _kind(t, kind)
    if kind == "data":
        assert t.dtype.is_floating_point
        return torch.full_like(t, float("nan"))
    if kind in ("index", "mask"):
        assert not t.dtype.is_floating_point
        if kind == "mask":
            assert bool(t.any()), "the true int_mask must have ones"
        return torch.zeros_like(t)
    if kind == "features":
        assert t.dim() == 2 and t.shape[0] == 2 and t.dtype == torch.float64
        p = torch.zeros_like(t)
        p[1] = 1.0
        return p
    assert t.dtype == torch.float64 and bool((t[..., 1:] > t[..., :-1]).all()), "edges must be strictly increasing"
    return t * 0.5 - 7.0


def scrubbed(t, kind=None):
    """The input of a scrub run: finite, and different from the true one (data: rolled by one row and rescaled; the rest: the placeholder)."""
    kind = _kind(t, kind)
    if kind == "data":
        return (torch.roll(t.to(torch.float64), 1, 0) * 0.75 + 0.125).to(t.dtype)
    return placeholder(t, kind)


# ---- the three runs --------------------------------------------------------------------------------------------------------------
def _compare(run, got, ref, blanks, same, failures):
    """Assertions (b) and (c) of one run.  same: name -> comparison(got, want, what); the entry None is the bit-for-bit comparison that
    every other output gets (tests/test_gpu_streams.py passes assert_same_bits of tests/test_gpu_guard_bands.py)."""
    for k, want in ref.items():
        try:
            (same.get(k) or same[None])(got[k], want, f"{k} against the plain run")
        except AssertionError as e:
            failures.append((run, "b", str(e).splitlines()[0]))
        if same_bits(got[k], blanks[k]):
            failures.append((run, "c", f"{k} still holds its placeholder"))
        elif got[k].dtype.is_floating_point and not bool(torch.isfinite(got[k]).all()):
            failures.append((run, "c", f"{k} is not finite"))


def free_side_stream():
    """A non-blocking side stream that does not share the default stream's hardware queue: a short sleep on it does not hold back a
    launch on stream 0.  (The streams of torch's pool keep their queues: in every session the same streams of the pool share one.)"""
    cal = calibration()
    probe = torch.zeros(1, device="cuda")
    default = torch.cuda.default_stream()
    for _ in range(STREAM_TRIES):
        S = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            torch.cuda._sleep(cal["gate_cycles"] // 10)
        probe.add_(1.0)
        default.synchronize()
        free = not S.query()
        torch.cuda.synchronize()
        if free:
            return S
    raise AssertionError(f"none of {STREAM_TRIES} side streams runs beside the default stream: each shares its hardware queue")


def run_gated(seq, ins, inout=(), kinds=None, reset=None, same=None, what="sequence"):
    """seq: dict of device tensors -> dict of output tensors (taken from out()), library calls in between.  ins: the true inputs; inout:
    the names among them that seq writes (params, m, v, ...); kinds: name -> placeholder kind of the inputs that are not "data";
    reset(): restores the handle's loaded parameters (another finite vector; the true one arrives through seq); same: name ->
    comparison(got, want, what); its entry None is the bit-for-bit comparison of every output it does not name.  Raises GateFailure;
    returns {"outs", "warm_ms", "gated_ms", "gate_ms"}."""
    kinds = kinds or {}
    cal = calibration()
    default = torch.cuda.default_stream()
    failures = []

    def begin(stream, specs=None):
        """reset() and the scrub run: on `stream`, then once more on the default stream, where even a launch that strays to stream 0 is in
        order, so that the handle's workspaces hold what the scrub inputs give whatever the library does with its streams."""
        for s in (stream, default):
            if reset is not None:
                reset()
            _state["record"] = specs if s is stream else None
            try:
                with torch.cuda.stream(s):
                    seq({k: scrubbed(v, kinds.get(k)) for k, v in ins.items()})
            finally:
                _state["record"] = None
            torch.cuda.synchronize()
        if reset is not None:
            reset()
            torch.cuda.synchronize()

    def results(t, outs):
        assert not set(outs) & set(inout), "an output is named like an in/out tensor"
        return {**outs, **{k: t[k] for k in inout}}

    # gated, FIRST: until the gate ends nothing on the device derives from the true inputs
    for _ in range(STREAM_TRIES):
        S = free_side_stream()
        specs = []
        begin(S, specs)
        pre = [blank(shape, dtype) for shape, dtype in specs]
        staged = {k: placeholder(v, kinds.get(k)) for k, v in ins.items()}
        gate_end, probe = torch.cuda.Event(), torch.zeros(1, device="cuda")
        torch.cuda.synchronize()
        try:
            with torch.cuda.stream(S):
                torch.cuda._sleep(cal["gate_cycles"])
                gate_end.record()
            probe.add_(1.0)                       # stream 0 runs on beside the gate before the sequence ...
            default.synchronize()
            if gate_end.query():                  # ... or it does not: nothing true has been staged yet, take another stream
                continue
            with torch.cuda.stream(S):
                for k, v in ins.items():
                    staged[k].copy_(v)
                _state["replay"] = list(pre)
                t0 = time.perf_counter()
                outs = seq(staged)
                gated_ms = (time.perf_counter() - t0) * 1e3
                host_waited = gate_end.query() or S.query()
                gated = {k: v.clone() for k, v in results(staged, outs).items()}
            probe.add_(1.0)                       # ... and after it
            default.synchronize()
            free_after = not gate_end.query()
            break
        finally:
            _state["replay"] = None
            torch.cuda.synchronize()
    else:
        raise AssertionError(f"{what}: in {STREAM_TRIES} runs stream 0 queued behind the gate: no run can vouch that no launch left its stream")
    if host_waited:
        failures.append(("gated", "a", f"the gate was over when the sequence returned ({gated_ms:.1f} ms after it began, behind a gate of "
                                       f"{cal['gate_ms']:.0f} ms): a call made the host wait for its stream"))
    else:
        assert free_after, f"{what}: stream 0 queued behind the gate after the sequence: this run cannot vouch that no launch left its stream"

    # plain: the reference bits
    begin(default)
    t = {k: v.clone() for k, v in ins.items()}
    ref = results(t, seq(t))
    torch.cuda.synchronize()
    blanks = {k: blank(v.shape, v.dtype) for k, v in ref.items() if k not in inout}
    blanks.update({k: placeholder(ins[k], kinds.get(k)) for k in inout})
    for k, v in ref.items():
        assert not same_bits(v, blanks[k]), f"{what}: the plain run left {k} unwritten"
        assert not v.dtype.is_floating_point or bool(torch.isfinite(v).all()), f"{what}: the plain run's {k} is not finite"

    # warm
    begin(S)
    with torch.cuda.stream(S):
        t = {k: v.clone() for k, v in ins.items()}
        t0 = time.perf_counter()
        outs = seq(t)
        warm_ms = (time.perf_counter() - t0) * 1e3
        got = results(t, outs)
    torch.cuda.synchronize()
    _compare("warm", got, ref, blanks, same, failures)
    _compare("gated", gated, ref, blanks, same, failures)
    print(f"[stream gate] {what}: host enqueue {warm_ms:.2f} ms warm, {gated_ms:.2f} ms gated; gate {cal['gate_ms']:.0f} ms")
    assert warm_ms * 10.0 <= cal["gate_ms"], (f"{what}: the host side of the sequence took {warm_ms:.1f} ms, more than a tenth of the gate of "
                                              f"{cal['gate_ms']:.0f} ms: raise LONGEST_ENQUEUE_MS (the gate is 10 x the longest enqueue time)")
    if failures:
        raise GateFailure(what, failures)
    return {"outs": gated, "warm_ms": warm_ms, "gated_ms": gated_ms, "gate_ms": cal["gate_ms"]}
