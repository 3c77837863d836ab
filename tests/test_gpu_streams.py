"""Side-stream tests: every call runs on, and only on, its caller's stream, and nothing makes the host wait (tests/stream_gate.py).

include/baler_amd.h: "all work is enqueued asynchronously on the hipStream_t passed as `stream`; nothing synchronises the host", and a
handle re-packs its weight fragments lazily "on the stream of the first call that needs them after an optimiser step".  The rest of the
suite calls the library on the default stream, where a launch that went to stream 0 is still in order and a blocking call costs nothing.
Here each case issues ONE sequence of calls on a side stream behind a gate (a 200 ms device sleep) and holds
  (a) the sequence returned while the gate was still pending;
  (b) every output and in/out tensor, cloned on the same stream, equals the same sequence on the default stream bit for bit
      (bamd_column_moments: the comparison of tests/test_gpu_guard_bands.py at the bar of tests/test_gpu_colstats.py);
  (c) no output is a placeholder and every floating-point output is finite.
The negative controls come first and prove on the machine that runs the suite that the detector detects: a call on the wrong stream, a
trailing launch on the wrong stream, and a host wait.

Handle sequence (129 rows: several row groups and a remainder), every (family, routing) of tests/test_gpu_guard_bands.py plus the wide
fp64 class and the two binary16 inference modes:
    load_params -> encode(raw rows, features) into float32 -> encode into float16 -> decode(float16 codes) -> decode(renorm + int_mask)
    into float64 -> forward_loss(raw rows, features) -> fwd_bwd -> train_step(t = 1, loss_accum) -> encode -> adam_step(t = 2) -> decode
so that the lazily re-made fragments (16-bit inference fragments, bf16 training fragments, the wide state of 64..127-column tables, the
wide fp64 class's copy) are re-made behind the gate once after a fused step and once after a plain Adam launch.  Every family serves
every call of it (F16 / F16X3 handles and the wide fp64 class train on other kernels than they infer on; the case line names the path).
No oracle call: parity of the plain calls is the job of the other modules."""
import numpy as np
import pytest
import torch

import stream_gate as sg
from baler_amd import native
from test_gpu_guard_bands import (FAMILIES, ROUTES, _sums_close, assert_same_bits, dev, family, feats_of, forward_loss_raw, raw2)

pytestmark = pytest.mark.gpu

F32, F64, F16 = torch.float32, torch.float64, torch.float16
N = 129
BITS = {None: assert_same_bits}
# families of this module (the FAMILIES layout of tests/test_gpu_guard_bands.py; the last field here: the h.path the case must report)
EXTRA = {
    "cfd625-fp64": ("dense", 625, 7, "fp64", {}, ("default", "lat32-64"), "fused-infer"),     # fused64w.hip: the lazily re-made wide fp64 fragments
    "ae24-fp16": ("dense", 24, 15, "fp16", {}, ("default",), "f16"),
    "ae24-fp16x3": ("dense", 24, 15, "fp16x3", {}, ("default",), "f16x3"),                   # infer16_stale
}
HANDLE_CASES = [pytest.param(f, r, id=f"{f}-{r}") for f, v in FAMILIES.items() for r in dict.fromkeys(v[5] + v[6])]
HANDLE_CASES += [pytest.param(f, r, id=f"{f}-{r}") for f, v in EXTRA.items() for r in v[5]]


def make_family(name, route, monkeypatch):
    if name in FAMILIES:
        return family(name, route, monkeypatch)
    spec = EXTRA[name]
    got = family(name, route, monkeypatch, spec=spec)
    assert got[0].path == spec[6], f"{name}: path {got[0].path}, expected {spec[6]}"
    return got


def other_params(flat):
    """Another finite parameter vector of the same scale: what reset() loads, ungated, before every run."""
    return (torch.roll(flat, 7) * 0.9).contiguous()


def handle_inputs(h, flat, seed):
    F = h.dims[0]
    xdt = F64 if h.param_dtype == F64 else F32
    x = dev(np.random.default_rng(seed).random((N, F)), xdt)
    fnp, mnp = feats_of(F)
    mnp[0] = 1
    ins = {"p": flat, "x": x, "xraw": dev(x.cpu().numpy().astype(np.float64) * fnp[1] + fnp[0], xdt), "features": dev(fnp), "renorm": dev(fnp),
           "int_mask": dev(mnp), "m": torch.zeros_like(flat), "v": torch.zeros_like(flat),
           "loss_accum": torch.full((1,), 0.25, dtype=F64, device="cuda")}
    kinds = {"features": "features", "renorm": "features", "int_mask": "mask"}
    return ins, kinds, ("p", "m", "v", "loss_accum")


def handle_sequence(h):
    F, Z, npar, pdt = h.dims[0], h.z_dim, h.nparams, h.param_dtype
    xdt = F64 if pdt == F64 else F32

    def seq(t):
        o = {}
        h.load_params(t["p"])
        o["z32"] = h.encode(t["xraw"], features=t["features"], out=sg.out((N, Z), F32))
        o["z16"] = h.encode(t["x"], out=sg.out((N, Z), F16))
        o["d16"] = h.decode(o["z16"], out=sg.out((N, F), F32))
        o["d64"] = h.decode(o["z32"], features=t["renorm"], int_mask=t["int_mask"], out=sg.out((N, F), F64))
        o["recon"], o["loss"] = sg.out((N, F), xdt), sg.out((1,), F64)
        forward_loss_raw(h, t["xraw"], t["features"], o["recon"], o["loss"])
        o["g"] = sg.out((npar + 1,), pdt)
        h.fwd_bwd(t["x"], o["g"])
        h.train_step(t["x"], t["p"], t["m"], t["v"], 1, 1e-3, loss_accum=t["loss_accum"])
        o["z_step"] = h.encode(t["x"], out=sg.out((N, Z), F32))          # the fragments follow a fused step ...
        h.adam_step(t["p"], o["g"], t["m"], t["v"], 2, 1e-3)
        o["d_adam"] = h.decode(o["z_step"], out=sg.out((N, F), xdt))     # ... and a plain Adam launch
        return o
    return seq


# ---- negative controls: AE(24, 15) fp32 ------------------------------------------------------------------------------------------
UNSEEN = ("the harness let it pass: the side stream shared a hardware queue with the default stream, or the gate was too short "
          "(tests/stream_gate.py: free_side_stream, gate_ms)")


def control(monkeypatch, faulty):
    """Run `load_params, then faulty(h, t)` through the harness; -> the (run, letter) pairs it reported."""
    h, _, flat, _, _ = make_family("ae24-fp32", "default", monkeypatch)
    ins, kinds, _ = handle_inputs(h, flat, 5)
    other = other_params(flat)

    def seq(t):
        h.load_params(t["p"])
        return faulty(h, t)
    try:
        sg.run_gated(seq, {"p": ins["p"], "x": ins["x"]}, reset=lambda: h.load_params(other), same=BITS, what=f"control {faulty.__name__}")
    except sg.GateFailure as e:
        print(f"    reported: {e}")
        return e.failed
    pytest.fail(f"control {faulty.__name__}: {UNSEEN}")


def test_control_wrong_stream(monkeypatch):
    def wrong_stream(h, t):
        with torch.cuda.stream(torch.cuda.default_stream()):
            return {"z": h.encode(t["x"], out=sg.out((N, 15), F32))}
    failed = control(monkeypatch, wrong_stream)
    assert ("gated", "b") in failed and ("gated", "a") not in failed, f"reported {sorted(failed)}; {UNSEEN}"


def test_control_trailing_launch(monkeypatch):
    def trailing_launch(h, t):
        z = h.encode(t["x"], out=sg.out((N, 15), F32))
        with torch.cuda.stream(torch.cuda.default_stream()):
            return {"z": z, "z16": z.to(F16)}
    failed = control(monkeypatch, trailing_launch)
    assert ("gated", "b") in failed and ("gated", "a") not in failed, f"reported {sorted(failed)}; {UNSEEN}"


def test_control_host_wait(monkeypatch):
    def host_wait(h, t):
        z = h.encode(t["x"], out=sg.out((N, 15), F32))
        torch.cuda.current_stream().synchronize()
        return {"z": z}
    failed = control(monkeypatch, host_wait)
    assert failed == {("gated", "a")}, f"reported {sorted(failed)}; {UNSEEN}"


# ---- handle sequences ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,route", HANDLE_CASES)
def test_handle_sequence(name, route, monkeypatch):
    h, _, flat, cmode, _ = make_family(name, route, monkeypatch)
    ins, kinds, inout = handle_inputs(h, flat, 11)
    other = other_params(flat)
    got = sg.run_gated(handle_sequence(h), ins, inout=inout, kinds=kinds, reset=lambda: h.load_params(other), same=BITS,
                       what=f"{name} {route}")
    print(f"[streams] family={name} path={h.path} compute={cmode} routing={route} {ROUTES[route]} rows={N}: every call of the sequence "
          f"served; host enqueue {got['warm_ms']:.2f} ms")


# ---- handle-free sequence --------------------------------------------------------------------------------------------------------
C, D, NP, NBIG = 24, 7, 3, 4097      # 4097 rows: the first size on bamd_swd's passes through global memory
E_RESP, E_RESID = np.linspace(-60.0, 60.0, 41), np.linspace(-1.0, 1.0, 33)


def free_inputs(dtype, seed):
    rng = np.random.default_rng(seed)
    xnp = rng.uniform(0.5, 2.0, size=(N, C))
    fnp = np.stack([xnp.min(0) - 0.5, xnp.max(0) - xnp.min(0) + 1.0])
    mnp = (rng.random(C) < 0.3).astype(np.uint8)
    mnp[0] = 1
    sel = rng.choice(N * C, size=N * C // 5, replace=False)
    proj = rng.normal(size=(NP, D))
    ins = {"x": dev(xnp, dtype), "r": dev(xnp * (1.0 + rng.normal(scale=0.08, size=xnp.shape)), dtype), "features": dev(fnp), "int_mask": dev(mnp),
           "table": dev(xnp, dtype), "rows": dev(sel // C, torch.int64), "cols": dev(sel % C, torch.int32), "vals": dev(rng.normal(size=sel.size), F16),
           "proj": dev(proj / np.linalg.norm(proj, axis=1, keepdims=True), dtype),
           "z": dev(rng.normal(size=(N, D)) * 0.7 + 0.2, dtype), "prior": dev(rng.normal(size=(N, D)), dtype),
           "zbig": dev(rng.normal(size=(NBIG, D)) * 0.7 + 0.2, dtype), "priorbig": dev(rng.normal(size=(NBIG, D)), dtype),
           "e_resp": dev(E_RESP), "e_resid": dev(E_RESID), "e_val": dev(np.tile(np.linspace(0.0, 3.0, 25), (C, 1)))}
    kinds = {"features": "features", "int_mask": "mask", "rows": "index", "cols": "index", "e_resp": "edges", "e_resid": "edges", "e_val": "edges"}
    return ins, kinds, ("table",)


def free_steps(dtype, with_minmax=True):
    """The handle-free sequence as a list of steps (t, o), one library call each (column_moments: two)."""
    P, S = native._ptr, native._stream
    code = native.F64 if dtype == F64 else native.F32

    def minmax(t, o):
        o["minmax"] = sg.out((2, C), F64)
        raw2("bamd_minmax", (P(t["x"]), code, N, C, P(o["minmax"]), S(t["x"])))

    def col_minmax(t, o):
        o["col_minmax"] = sg.out((2, C), F64)
        raw2("bamd_col_minmax", (P(t["x"]), code, N, C, P(o["col_minmax"]), S(t["x"])))

    def normalize(t, o):
        o["norm"] = sg.out((N, C), dtype)
        raw2("bamd_normalize", (P(t["x"]), code, N, C, P(t["features"]), P(o["norm"]), code, S(t["x"])))

    def renormalize(t, o):
        o["renorm"] = sg.out((N, C), F64)
        raw2("bamd_renormalize", (P(t["x"]), code, N, C, P(t["features"]), P(t["int_mask"]), P(o["renorm"]), S(t["x"])))

    def emd_rows(t, o):
        o["emd"] = sg.out((1,), F64)
        raw2("bamd_emd_rows", (P(t["x"]), P(t["r"]), code, N, C, P(o["emd"]), S(t["x"])))

    def error_deltas(t, o):
        o["flags"], o["deltas"] = sg.out((N, C), torch.uint8), sg.out((N, C), F16)
        raw2("bamd_error_deltas", (P(t["x"]), P(t["r"]), code, N * C, 10.0, P(o["flags"]), P(o["deltas"]), S(t["x"])))

    def apply_deltas(t, o):
        native.apply_deltas(t["table"], t["rows"], t["cols"], t["vals"])

    def swd(z, prior, n, tag):
        def step(t, o):
            o["swd_loss" + tag], o["swd_dz" + tag] = sg.out((1,), F64), sg.out((n, D), dtype)
            raw2("bamd_swd", (P(t[z]), P(t[prior]), P(t["proj"]), code, n, D, NP, 0.5, P(o["swd_loss" + tag]), P(o["swd_dz" + tag]), S(t[z])))
        return step

    def column_moments(t, o):
        o["mom0"], o["mom1"] = sg.out((13, C), F64), sg.out((13, C), F64)
        raw2("bamd_column_moments", (P(t["x"]), P(t["r"]), code, N, C, -1, 0.0, P(o["mom0"]), 0, S(t["x"])))
        o["mom1"].copy_(o["mom0"])
        raw2("bamd_column_moments", (P(t["x"]), P(t["r"]), code, N, C, -1, 0.0, P(o["mom1"]), 1, S(t["x"])))

    def column_hist(t, o):
        n_er, n_ed, n_ev = len(E_RESP), len(E_RESID), t["e_val"].shape[1]
        for k, e in (("h_resp", n_er), ("h_resid", n_ed), ("h_before", n_ev), ("h_after", n_ev)):
            o[k] = sg.out((C, e - 1), torch.int64)
        raw2("bamd_column_hist", (P(t["x"]), P(t["r"]), code, N, C, -1, 0.0, P(t["e_resp"]), n_er, P(o["h_resp"]), P(t["e_resid"]), n_ed,
                                  P(o["h_resid"]), P(t["e_val"]), n_ev, P(o["h_before"]), P(o["h_after"]), 0, S(t["x"])))

    steps = [col_minmax, normalize, renormalize, emd_rows, error_deltas, apply_deltas, swd("z", "prior", N, ""),
             swd("zbig", "priorbig", NBIG, "_big"), column_moments, column_hist]
    return ([minmax] if with_minmax else []) + steps


FREE_SAME = {None: assert_same_bits, "mom0": _sums_close, "mom1": _sums_close}       # colstats.hip sums with atomics


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_handle_free_sequence(dtype):
    ins, kinds, inout = free_inputs(dtype, 21)
    steps = free_steps(dtype)

    def seq(t):
        o = {}
        for step in steps:
            step(t, o)
        return o
    got = sg.run_gated(seq, ins, inout=inout, kinds=kinds, same=FREE_SAME, what=f"handle-free {dtype}")
    o = got["outs"]
    assert int(o["flags"].sum()) > 0 and all(int(o[k].sum()) > 0 for k in ("h_resp", "h_resid", "h_before", "h_after")), "nothing flagged / counted"
    print(f"[streams] handle-free {dtype} rows={N} (swd also {NBIG}): host enqueue {got['warm_ms']:.2f} ms")


# ---- two streams at once (ungated, as the two tests of tests/test_gpu_parity.py are) ----------------------------------------------
def _results(t, o, inout):
    return {**o, **{k: t[k] for k in inout}}


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_handle_free_two_streams(dtype):
    """The per-(device, stream) scratch of bamd_swd, bamd_emd_rows and the column statistics: the handle-free sequence (without bamd_minmax,
    which test_handle_free_kernels_on_two_streams has) from two streams on different tables, call by call in turn."""
    steps = free_steps(dtype, with_minmax=False)
    tables, refs = [], []
    for seed in (31, 32):
        ins, _, inout = free_inputs(dtype, seed)
        t, o = {k: v.clone() for k, v in ins.items()}, {}
        for step in steps:
            step(t, o)
        tables.append(ins)
        refs.append(_results(t, o, inout))
    torch.cuda.synchronize()
    streams = (torch.cuda.Stream(), torch.cuda.Stream())
    for rnd in range(5):
        ts = [{k: v.clone() for k, v in ins.items()} for ins in tables]
        os_ = [{}, {}]
        torch.cuda.synchronize()
        for step in steps:
            for i in (0, 1):
                with torch.cuda.stream(streams[i]):
                    step(ts[i], os_[i])
        torch.cuda.synchronize()
        for i in (0, 1):
            for k, want in refs[i].items():
                (FREE_SAME.get(k) or assert_same_bits)(_results(ts[i], os_[i], inout)[k], want, f"round {rnd} stream {i}: {k}")


@pytest.mark.parametrize("name", ["cfd625-fp32", "ae24-fp64", "ae24-bf16"])
def test_two_handles_two_streams(name, monkeypatch):
    """test_two_handles_two_streams of tests/test_gpu_parity.py (AE(24, 15) fp32) for a wide fp32, an fp64 and a bf16 family: two handles with
    different parameters, each driven from its own stream, against the same calls on the default stream bit for bit."""
    ha, _, pa, _, _ = make_family(name, "default", monkeypatch)
    hb, _, _, _, _ = make_family(name, "default", monkeypatch)
    pb = other_params(pa)
    hb.load_params(pb)
    F, Z = ha.dims[0], ha.z_dim
    xdt = F64 if ha.param_dtype == F64 else F32
    x = dev(np.random.default_rng(41).random((N, F)), xdt)

    def calls(h):
        g = torch.zeros(h.nparams + 1, dtype=h.param_dtype, device="cuda")
        z = h.encode(x, out_dtype=F32)
        h.fwd_bwd(x, g)
        return {"z": z, "z16": h.encode(x, out_dtype=F16), "d": h.decode(z), "g": g}
    want = [calls(ha), calls(hb)]
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    for rnd in range(3):
        with torch.cuda.stream(sa):
            ga = calls(ha)
        with torch.cuda.stream(sb):
            gb_ = calls(hb)
        torch.cuda.synchronize()
        for tag, got, ref in (("a", ga, want[0]), ("b", gb_, want[1])):
            for k in ref:
                assert_same_bits(got[k], ref[k], f"{name} round {rnd} handle {tag}: {k}")
    assert not torch.equal(want[0]["z"], want[1]["z"])
