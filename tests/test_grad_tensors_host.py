"""tests/grad_tensors.py proved on the CPU before the GPU tests trust it:
  (a) the per-tensor checker sees three mutations of the oracle's gradient that the whole-vector bar lets through;
  (b) for every (family, row count, input) of tests/test_gpu_grad_tensors.py plain float32 NumPy arithmetic stays within HALF the
      family's bar on every tensor against the fp64 reference (float64 arithmetic for the fp64 families): the bars asked of the
      kernels are reachable tensor by tensor, with and without the latent term -- a condition on the cases, not a measurement;
  (c) the float64 fwd_bwd_np agrees with oracle/c_oracle and tests/fpga_ref.py to 1e-12 per tensor."""
import os

import numpy as np
import pytest

import fpga_ref
import grad_tensors as gt
import test_gpu_grad_tensors as cases
from oracle import c_oracle as orc
from test_gpu_guard_bands import BIG, FAMILIES, DenseRef
from test_gpu_parity import TOL32, rel


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
def _ae24():
    dims = orc.ae_dims(24, 15)
    ref = DenseRef(dims, orc.formula_params(dims, 139))
    x = ref.rows(513, 513)
    return dims, ref, x


def _drop_last_row(tensor):
    def mutate(dims, ref, x, go):
        _, g_last = orc.fwd_bwd(dims, ref.flat, x[-1:])          # the gradient is a sum over rows
        s = dict(gt.tensor_slices(dims))[tensor]
        out = go.copy()
        out[s] -= g_last[s]
        return out
    return mutate


def _scale(tensor, factor):
    def mutate(dims, ref, x, go):
        out = go.copy()
        out[dict(gt.tensor_slices(dims))[tensor]] *= factor
        return out
    return mutate


@pytest.mark.parametrize("tensor,mutate", [("en1.weight", _drop_last_row("en1.weight")), ("en1.bias", _drop_last_row("en1.bias")),
                                           ("en2.weight", _scale("en2.weight", 1.0 + 5e-4))],
                         ids=["en1.weight-without-the-last-row", "en1.bias-without-the-last-row", "en2.weight-times-1.0005"])
def test_checker_sees_what_the_whole_vector_bar_does_not(tensor, mutate):
    dims, ref, x = _ae24()
    _, go = orc.fwd_bwd(dims, ref.flat, x)
    bad = mutate(dims, ref, x, go)
    whole = rel(bad, go)
    errs = {n: max(l2, mx) for n, l2, mx in gt.per_tensor(bad, go, dims)}
    print(f"\n{tensor}: whole vector {whole:.3e}, own scale {errs[tensor]:.3e}")
    assert 0.0 < whole < TOL32, "the blind spot: the whole-vector bar passes this mutation"
    assert [n for n, e in errs.items() if e > 1e-4] == [tensor]
    assert all(e == 0.0 for n, e in errs.items() if n != tensor)
    with pytest.raises(AssertionError, match=tensor.replace(".", r"\.") + ": rel-L2"):
        gt.assert_per_tensor(bad, go, dims, TOL32, "mutated")
    gt.assert_per_tensor(go, go, dims, 0.0, "unmutated")


def test_per_tensor_edges():
    dims = orc.ae_dims(24, 15)
    names = [n for n, _ in gt.tensor_slices(dims)]
    assert names[:2] == ["en1.weight", "en1.bias"] and names[-2:] == ["de4.weight", "de4.bias"] and len(names) == 16
    assert [n for n, _ in gt.tensor_slices([3, 2, 3])] == ["L0.weight", "L0.bias", "L1.weight", "L1.bias"]
    assert gt.tensor_slices([3, 2, 3], names=False) == [slice(0, 6), slice(6, 8), slice(8, 14), slice(14, 17)]
    d = [3, 0, 3]                                                # zero-size tensors are skipped
    assert [n for n, _, _ in gt.per_tensor(np.ones(3), np.ones(3), d)] == ["L1.bias"]
    want = np.array([0.0] * 6 + [1.0, 2.0] + [0.0] * 9)          # a reference tensor of norm 0 asks for exact zeros
    got = want.copy()
    assert all(l2 == 0.0 and mx == 0.0 for _, l2, mx in gt.per_tensor(got, want, [3, 2, 3]))
    got[0] = 1e-300
    assert gt.per_tensor(got, want, [3, 2, 3])[0] == ("L0.weight", np.inf, np.inf)
    with pytest.raises(AssertionError, match="L0.weight"):
        gt.assert_per_tensor(got, want, [3, 2, 3], 1.0, "zero reference")
    got = want.copy()
    got[7] = np.nan                                              # a NaN is above every bar
    with pytest.raises(AssertionError, match="L0.bias"):
        gt.assert_per_tensor(got, want, [3, 2, 3], 1e300, "nan")


# ---- (b), (c) ----------------------------------------------------------------------------------------------------------------------
def _rows(name):
    return ((BIG,) if name == "ae24-fp32" else ()) + cases.ROWS


def _act(name):
    return "relu" if FAMILIES[name][0] == "fpga" else "leaky"


def test_cases_cover_the_families_and_their_routings():
    assert set(cases.NAMES) == {f for f, v in FAMILIES.items() if v[3] != "bf16" and f != "pjconv-z10"}
    for f in cases.NAMES:
        have = {r for n, r in cases.CASES if n == f}
        assert set(FAMILIES[f][6]) <= have
        assert ("dw64-macro4" in have) == (FAMILIES[f][3] == "fp64")
    assert {r for n, r in cases.CASES if n == "ae24-fp32"} >= set(cases.PAIR_ROUTES)
    assert all(cases.rows_of("ae24-fp32", r)[0] == BIG for r in cases.PAIR_ROUTES) and cases.rows_of("ae24-fp32", "default") == cases.ROWS
    assert "lat4-0" in {r for n, r in cases.CASES if n == "class40-fp32"}
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "README.md")) as f:
        readme = f.read()
    mine = {k for f in cases.NAMES for r in cases.more_routes(f) for k in cases.ALL_ROUTES[r]}      # the knobs of the routings this module adds
    assert mine and not [k for k in mine if f"`{k}" not in readme], "a routing knob the README's table does not name"


@pytest.mark.parametrize("name", cases.NAMES)
def test_plain_arithmetic_alone_stays_within_half_the_bar(name):
    ref, mode, bar = cases.reference_of(name), FAMILIES[name][3], cases.bar_of(name)
    dt = np.float64 if mode == "fp64" else np.float32
    dims = list(ref.dims)
    for n in _rows(name):
        ins, (_, lg, seen_l) = cases.inputs_of(name, n)
        want, (_, go_lat) = cases.references_of(name, n)
        for tag, _, _, seen in ins:
            _, g = gt.fwd_bwd_np(dims, ref.flat, seen, dt, _act(name))
            gt.assert_per_tensor(g, want[tag][1], dims, bar / 2, f"{name} n={n} {tag} {np.dtype(dt).name} NumPy")
        _, g = gt.fwd_bwd_np(dims, ref.flat, seen_l, dt, _act(name), latent_grad=lg)
        gt.assert_per_tensor(g, go_lat, dims, bar / 2, f"{name} n={n} latent {np.dtype(dt).name} NumPy")


@pytest.mark.parametrize("name", cases.NAMES)
def test_float64_restatement_agrees_with_the_references(name):
    ref = cases.reference_of(name)
    dims = list(ref.dims)
    for n in (129, 17, 1):
        ins, (_, lg, seen_l) = cases.inputs_of(name, n)
        want, (lo_lat, go_lat) = cases.references_of(name, n)
        tag, _, _, seen = ins[0]
        lo, g = gt.fwd_bwd_np(dims, ref.flat, seen, np.float64, _act(name))
        gt.assert_per_tensor(g, want[tag][1], dims, 1e-12, f"{name} n={n} float64 NumPy")
        assert abs(lo - want[tag][0]) <= 1e-12 * want[tag][0]
        lo, g = gt.fwd_bwd_np(dims, ref.flat, seen_l, np.float64, _act(name), latent_grad=lg)
        gt.assert_per_tensor(g, go_lat, dims, 1e-12, f"{name} n={n} latent float64 NumPy")
        assert abs(lo - lo_lat) <= 1e-12 * lo_lat
    if FAMILIES[name][0] == "fpga":                               # the FPGA restatement directly, its latent term included
        x = ref.rows(17, 5)
        lg = np.random.default_rng(1).normal(size=(17, dims[3])) * 0.01
        _, g = gt.fwd_bwd_np(dims, ref.flat, x, np.float64, "relu", latent_grad=lg)
        gt.assert_per_tensor(g, fpga_ref.fwd_bwd(dims, ref.flat, x, lg)[1], dims, 1e-12, f"{name} fpga_ref with a latent term")
