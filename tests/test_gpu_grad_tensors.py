"""Every training path's gradient against the fp64 oracle TENSOR BY TENSOR (tests/grad_tensors.py).

The suite's gradient checks mostly hold the whole flat vector, which in these models is the decoder: a 1e-5 bar on the vector of
AE(24, 15) is a 2 .. 5 % bar on en1.weight.  Here every tensor meets the family's existing bar -- 1e-5 in fp32, 1e-11 in fp64, ten
times those for FPGA_prototype_model as in tests/test_gpu_fpga.py -- against its own norm and its own maximum.  No new tolerance:
tests/test_grad_tensors_host.py shows on the CPU that plain float32 NumPy arithmetic stays within HALF the bar on every tensor for
every (family, row count, input) used here, so a miss is the kernel's.

Cases: one per (family, training routing) of FAMILIES / ROUTES of tests/test_gpu_guard_bands.py, without the bf16 families (held per
tensor to their own emulation in tests/test_gpu_bf16_contract.py) and without pjconv-z10 (per tensor already), plus the routings of
MORE_ROUTES below for kernels those tables do not force at small sizes.  Every knob is one of the README's table and is set before
the handle is created.
Rows: 513 (crosses the 512-row switch of the wide 16-row launches, one past the reference's batch size, a one-row last tile), then
129, 17 and 1 on ONE handle, so that the smaller calls run over workspaces the larger one left dirty; the pair routings of ae24-fp32
first run 256 * 64 + 65 rows (the second iteration of two workgroups).  All rows, the big batch included, come from the off-the-kink
generator of the family's reference class: a LeakyReLU sign that differs between float32 and float64 is an error of the comparison.
Calls per row count: fwd_bwd on float64 rows and on float32 rows (reference: the oracle on the widened rows), at 129 rows fwd_bwd with
features (raw rows, normalise-on-load), and fwd_bwd_latent with the guard-band suite's latent term.  Every output starts from a
non-zero fill.  Separately the latent term's own share, fwd_bwd_latent - fwd_bwd, is held on the encoder tensors (latent_share)."""
import functools

import numpy as np
import pytest
import torch

import fpga_ref
import grad_tensors as gt
from oracle import c_oracle as orc
from test_gpu_guard_bands import BIG, FAMILIES, ROUTES, TOL, DenseRef, FpgaRef, dev, family, feats_of, host

pytestmark = pytest.mark.gpu

ROWS = (513, 129, 17, 1)
FEATURE_ROWS = 129
SEED = 4000
PAIR_ROUTES = ("pair-roles0", "pair-roles1", "pair-tail-split")

# Routings of this module alone (README knobs).  On the layer-wise path a batch of up to 768 rows takes every weight gradient in one
# launch (dw_small_all_k) whatever BALER_AMD_SHORT_DW says, so the short-side kernels (from 128 rows; the LDS-tiled GEMM below) need
# BALER_AMD_DW_SMALL_ROWS=0 and the LDS-tiled GEMM at every size needs both.
MORE_ROUTES = {
    "dw64-macro4": {"BALER_AMD_DW64_MACRO_BLKS": "4"},       # the tile-block fp64 weight-gradient kernel from 64 rows on (default 1,024)
    "gemm-small0": {"BALER_AMD_GEMM_SMALL_ROWS": "0"},       # forward / input-gradient products on the tiled GEMM
    "dw-small0": {"BALER_AMD_DW_SMALL_ROWS": "0"},           # the per-layer weight-gradient launches instead of the one launch
    "dw-small0-short-dw0": {"BALER_AMD_DW_SMALL_ROWS": "0", "BALER_AMD_SHORT_DW": "0"},
}
ALL_ROUTES = {**ROUTES, **MORE_ROUTES}


def more_routes(name):
    kind, F, _, mode, env, _, _ = FAMILIES[name]
    if mode == "fp64":
        return ("dw64-macro4",)
    if env or kind == "dims":                                # the two layer-wise families
        return ("gemm-small0", "dw-small0", "dw-small0-short-dw0")
    if kind == "dense" and F > 127:                          # the wide families
        return ("dw-small0",)
    return {"class40-fp32": ("lat4-0",), "ae24-fp32": ("pair-tail-split",)}.get(name, ())


NAMES = [f for f, v in FAMILIES.items() if v[3] != "bf16" and v[0] != "pj"]
CASES = [(f, r) for f in NAMES for r in FAMILIES[f][6] + more_routes(f)]


def bar_of(name):
    kind, mode = FAMILIES[name][0], FAMILIES[name][3]
    return TOL[mode] * (10 if kind == "fpga" else 1)


def rows_of(name, route):
    return ((BIG,) if name == "ae24-fp32" and route in PAIR_ROUTES else ()) + ROWS


# ---- what the calls get and what they are held to: NumPy alone, shared with tests/test_grad_tensors_host.py -----------------------
@functools.lru_cache(maxsize=None)
def reference_of(name):
    """The family's reference object on the parameters as the handle holds them, built without a handle (test_gradient_tensors
    checks that it equals the one `family` returns)."""
    kind, F, Z, mode, _, _, _ = FAMILIES[name]
    if kind == "fpga":
        d, rng = fpga_ref.dims(F, Z), np.random.default_rng(17)
        flat = np.concatenate([np.concatenate([rng.uniform(-1, 1, d[l + 1] * d[l]) / np.sqrt(d[l]), rng.uniform(-1, 1, d[l + 1]) / np.sqrt(d[l])])
                               for l in range(6)])
        ref = FpgaRef(d, flat)
    else:
        dims = F if kind == "dims" else orc.ae_dims(F, Z)
        ref = DenseRef(dims, orc.formula_params(dims, 100 + dims[0] + Z))
    if mode != "fp64":
        ref.flat = ref.flat.astype(np.float32).astype(np.float64)
    return ref


def latent_dim(ref):
    return ref.dims[(len(ref.dims) - 1) // 2]


@functools.lru_cache(maxsize=None)
def inputs_of(name, n):
    """[(tag, rows as the call gets them, features or None, the rows the kernel computes on in float64)] and the latent call's
    (rows, latent_grad in the parameter type, rows in float64)."""
    ref, mode = reference_of(name), FAMILIES[name][3]
    x64 = ref.rows(n, SEED + n)
    out = [("x=float64", x64, None, x64), ("x=float32", x64.astype(np.float32), None, x64.astype(np.float32).astype(np.float64))]
    if n == FEATURE_ROWS:
        fnp, _ = feats_of(ref.dims[0])
        for dt in (np.float64, np.float32):
            raw = (x64.astype(dt).astype(np.float64) * fnp[1] + fnp[0]).astype(dt)
            out.append((f"x={np.dtype(dt).name} features", raw, fnp, (raw.astype(np.float64) - fnp[0]) / fnp[1]))
    pdt = np.float64 if mode == "fp64" else np.float32
    lg = np.random.default_rng(n).normal(size=(n, latent_dim(ref))) * (0.01 * 24 / ref.dims[0])
    xl = x64.astype(pdt)
    return out, (xl, lg.astype(pdt), xl.astype(np.float64))


@functools.lru_cache(maxsize=None)
def references_of(name, n):
    """({tag: (loss, gradient)}, (loss, gradient) with the latent term) of the fp64 reference, computed once per (family, rows) and
    shared by every routing."""
    ref = reference_of(name)
    ins, (_, lg, seen) = inputs_of(name, n)
    return {tag: ref.fwd_bwd(s) for tag, _, _, s in ins}, ref.fwd_bwd(seen, lg.astype(np.float64))


def latent_share(g_lat, g_plain, want_lat, want_plain, dims, bar, what):
    """The latent term's own share of the encoder gradient: (fwd_bwd_latent - fwd_bwd) on the same handle and rows against the same
    difference of the reference, per encoder tensor, rel-L2 against the difference's own norm at 100 x the family's bar (the
    difference of two float32 results that agree to 1e-5 each, where the latent share is about 1 % of the tensor).  The reference
    share must be at least 1e-3 of the tensor's norm, or the bound would say nothing."""
    L = len(dims) - 1
    d_got, d_want = np.asarray(g_lat, dtype=np.float64) - g_plain, want_lat - want_plain
    worst = ("", 0.0)
    for name, s in gt.tensor_slices(dims)[:2 * (L // 2)]:
        if s.stop == s.start:
            continue
        share = np.linalg.norm(d_want[s]) / np.linalg.norm(want_plain[s])
        assert share >= 1e-3, f"{what}: the latent term is {share:.2e} of {name}: the check has no power"
        err = np.linalg.norm(d_got[s] - d_want[s]) / np.linalg.norm(d_want[s])
        worst = max(worst, (name, err), key=lambda t: np.inf if np.isnan(t[1]) else t[1])
        assert err <= 100 * bar, f"{what}: latent share of {name} off by {err:.3e} of its own norm (bar {100 * bar:g}, share {share:.2e})"
    print(f"    latent share {what}: worst {worst[0]} {worst[1]:.3e} (bar {100 * bar:g})")


@pytest.mark.parametrize("name,route", [pytest.param(f, r, id=f"{f}-{r}") for f, r in CASES])
def test_gradient_tensors(name, route, monkeypatch):
    for k, v in MORE_ROUTES.get(route, {}).items():
        monkeypatch.setenv(k, v)
    h, ref, _, cmode, _ = family(name, route if route in ROUTES else "default", monkeypatch)
    print(f"[grad tensors] family={name} routing={route} {ALL_ROUTES[route]}")
    mine = reference_of(name)
    assert list(mine.dims) == list(ref.dims) and np.array_equal(mine.flat, ref.flat), "reference_of() and family() disagree on the parameters"
    assert cmode == FAMILIES[name][3]
    dims, bar, pdt, np_ = list(ref.dims), bar_of(name), h.param_dtype, h.nparams
    case_worst = ("", 0.0)

    def held(g, lo, go, what):
        nonlocal case_worst
        g = host(g)
        if lo != 0.0:
            lerr = abs(g[-1] - lo) / lo
            print(f"    loss {what}: {lerr:.3e} (bar {bar:g})")
            assert lerr <= bar, f"{what}: loss"
        w = gt.assert_per_tensor(g[:-1], go, dims, bar, what)
        case_worst = max(case_worst, w, key=lambda t: t[1])
        return g[:-1]

    for n in rows_of(name, route):
        print(f"  rows={n}")
        ins, (xl, lg, _) = inputs_of(name, n)
        want, (lo_lat, go_lat) = references_of(name, n)
        plain = {}
        for tag, x, fnp, _ in ins:
            g = torch.full((np_ + 1,), 3.0, dtype=pdt, device="cuda")
            h.fwd_bwd(dev(x), g, features=None if fnp is None else dev(fnp))
            plain[tag] = held(g, *want[tag], f"{name} {route} n={n} fwd_bwd {tag}")
        g = torch.full((np_ + 1,), -7.0, dtype=pdt, device="cuda")
        h.fwd_bwd_latent(dev(xl), dev(lg), g)
        what = f"{name} {route} n={n} fwd_bwd_latent"
        g_lat = held(g, lo_lat, go_lat, what)
        tag = f"x={xl.dtype.name}"
        latent_share(g_lat, plain[tag], go_lat, want[tag][1], dims, bar, what)
    print(f"[grad tensors] family={name} routing={route}: worst tensor {case_worst[0]} {case_worst[1]:.3e} (bar {bar:g})")
