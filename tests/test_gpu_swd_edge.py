"""bamd_swd at its edges (swd.hip), element by element against the stable-sort reference tests/swd_ref.py: every row count at which
the kernel changes branch, exact ties, NaN and infinities in z, prior and proj, guard bands and the order of calls; and the
one-thread-per-row kernel of bamd_emd_rows (elementwise.hip, up to 64 columns) at the standard of tests/test_gpu_emd_wide.py.

Inputs are swd_ref.dyadic throughout: float32, float64 and the reference sort the same keys and form the same w (derivation in
tests/swd_ref.py), so the order inside every tie group is checked by the comparison itself -- the ranks of a group meet different
prior values.  d in {1, 3, 8} and ns in {1, 2, 5}, all nine pairs at every size; every projection is drawn on its own.

Bars (the two of tests/test_gpu_swae.py for this call): |got - want| <= tol * max|want| over the elements that are finite in the
reference, tol = 1e-5 in float32 and 1e-12 in float64; the loss relative to itself at the same tol.  What is left to round is one
product by (T)(2 scale) and a sum of ns <= 5 terms per element, a few units of 2^-24 / 2^-53.  Non-finite elements must have the
reference's class (NaN, +inf, -inf) exactly.

Every call under test runs behind a call of the same (n, d, ns) on the same stream with finite inputs and reg_weight = 1e30
(`poison`): an element of the scratch G that the call under test does not write then shows in dz at about 1e24, not as a plausible
number left by an earlier call."""
import itertools
import math

import numpy as np
import pytest
import torch

import guard_bands as gb
import test_gpu_emd_wide as wide
from baler_amd import native
from oracle import c_oracle as orc
from swd_ref import SIZES, dyadic, swd_ref
from test_gpu_guard_bands import assert_same_bits, both, dev, host, raw2

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DTYPES = pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
TOL = {F32: 1e-5, F64: 1e-12}
D_NS = list(itertools.product((1, 3, 8), (1, 2, 5)))
NAN_SIZES = [3, 5, 37, 65, 257, 1000, 4095, 4097, 8191, 8193]      # every one has padding
TIE_SIZES = [37, 257, 4096, 4097, 8193]
NAN, INF = float("nan"), float("inf")


def rw(n):
    return 100.0 / (n * (n - 1))                 # training's reg_weight (modules/utils.py)


def draw(n, d, ns, seed=0):
    rng = np.random.default_rng(100003 * seed + 31 * n + 7 * d + ns)
    proj = np.stack([dyadic(rng, d, 1.0) for _ in range(ns)])
    return dyadic(rng, (n, d), 4.0), dyadic(rng, (n, d), 4.0), proj


def finite(a):
    return np.nan_to_num(a, nan=1.0, posinf=2.0, neginf=-2.0)


def poison(z, prior, proj, dtype):
    native.swd(dev(finite(z), dtype), dev(finite(prior), dtype), dev(finite(proj), dtype), 1e30)


def swd(z, prior, proj, dtype, reg_weight=None):
    """bamd_swd behind a poisoning call: -> (loss tensor, dz tensor)."""
    poison(z, prior, proj, dtype)
    return native.swd(dev(z, dtype), dev(prior, dtype), dev(proj, dtype), rw(z.shape[0]) if reg_weight is None else reg_weight)


def classes(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    return np.where(np.isnan(a), 1, np.where(a == np.inf, 2, np.where(a == -np.inf, 3, 0)))


def held(got, want, dtype, what):
    """The kernel's (loss, dz) against swd_ref's: classes exactly, finite elements and the loss at the bars of the module docstring."""
    (gl, gdz), (wl, wdz), tol = got, want, TOL[dtype]
    gl, gdz = gl.item(), host(gdz)
    assert np.array_equal(classes(gdz), classes(wdz)), f"{what}: dz differs from the reference in {int((classes(gdz) != classes(wdz)).sum())} NaN / inf classes"
    fin = classes(wdz) == 0
    if fin.any():
        top = np.abs(wdz[fin]).max()
        err = np.abs(gdz[fin] - wdz[fin]).max() / top if top > 0 else np.abs(gdz[fin]).max()
        print(f"    {what}: dz {err:.3e} of max|want| = {top:.3e} (bar {tol:g})")
        assert err <= tol, what + " dz"
    if math.isfinite(wl):
        print(f"    {what}: loss {gl:.17g} reference {wl:.17g} (bar {tol:g})")
        assert abs(gl - wl) <= tol * abs(wl), what + " loss"
    else:
        assert classes(np.float64(gl)) == classes(np.float64(wl)), f"{what}: loss {gl}, reference {wl}"


def check(z, prior, proj, dtype, what):
    want = swd_ref(z, prior, proj, rw(z.shape[0]))
    held(swd(z, prior, proj, dtype), want, dtype, what)
    return want


# ---- a. finite, every size ---------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("n", SIZES)
def test_finite_every_size(n, dtype):
    for d, ns in D_NS:
        z, prior, proj = draw(n, d, ns)
        what = f"n={n} d={d} ns={ns} {dtype}"
        check(z, prior, proj, dtype, what)
        first, again = swd(z, prior, proj, dtype), swd(z, prior, proj, dtype)
        assert_same_bits(again[0], first[0], what + ": loss of a second call")
        assert_same_bits(again[1], first[1], what + ": dz of a second call")
    z, prior, _ = draw(n, 1, 1, seed=1)
    one, both_ways = np.array([[1.0]]), np.array([[1.0], [-1.0]])
    zs = np.sort(z, axis=0)
    for name, zz, proj in (("as drawn", z, one), ("sorted", zs, one), ("sorted in reverse", zs[::-1].copy(), one),
                           ("ascending and descending in one call", zs, both_ways), ("as drawn, both ways", z, both_ways)):
        check(zz, prior, proj, dtype, f"n={n} d=1 {name} {dtype}")


# ---- b. ties -----------------------------------------------------------------------------------------------------------------------
def tie_cases(n, d, ns):
    z, prior, proj = draw(n, d, ns, seed=2)
    dup = z.copy()
    dup[10:20] = dup[10]
    dup[30:34] = dup[5]
    rng = np.random.default_rng(n)
    return prior, proj, {"rows 10..19 identical, rows 30..33 equal to row 5": dup, "all rows identical": np.tile(z[:1], (n, 1)),
                         "all zeros": np.zeros_like(z), "keys from {0, 1, 2, 3} / 64": rng.integers(0, 4, size=z.shape) / 64.0}


@DTYPES
@pytest.mark.parametrize("n", TIE_SIZES)
def test_ties(n, dtype):
    for d, ns in D_NS:
        prior, proj, cases = tie_cases(n, d, ns)
        for name, z in cases.items():
            check(z, prior, proj, dtype, f"n={n} d={d} ns={ns} {dtype} {name}")


# ---- c. NaN in z -------------------------------------------------------------------------------------------------------------------
def nan_cases(n, d):
    """name -> (rows that hold a NaN, column)."""
    c = d // 2
    return {"NaN at row 0": ([0], c), "NaN at row n // 2": ([n // 2], c), "NaN at row n - 1": ([n - 1], d - 1),
            "NaNs in two rows": ([1, n - 1], 0), "NaN in every row": (list(range(n)), c)}


@DTYPES
@pytest.mark.parametrize("n", NAN_SIZES)
def test_nan_in_z(n, dtype):
    for d, ns in D_NS:
        z0, prior, proj = draw(n, d, ns, seed=3)
        for name, (rows, col) in nan_cases(n, d).items():
            what = f"n={n} d={d} ns={ns} {dtype} {name}"
            z = z0.copy()
            z[rows, col] = NAN
            wl, wdz = check(z, prior, proj, dtype, what)
            # what the reference gives, said once more: the loss is NaN, the rows that hold a NaN are NaN, nothing else is NaN or inf
            mask = np.zeros((n, d), dtype=bool)
            mask[rows] = True
            assert math.isnan(wl) and np.array_equal(np.isnan(wdz), mask) and np.isfinite(wdz[~mask]).all(), what
            keep = np.setdiff1d(np.arange(n), rows)
            if len(keep) >= 2:
                zr, pr = np.ascontiguousarray(z[keep]), np.ascontiguousarray(prior[keep])
                want = check(zr, pr, proj, dtype, what + ", those rows removed")
                assert math.isfinite(want[0])


# ---- d. infinities in z ------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("n", NAN_SIZES)
def test_inf_in_z(n, dtype):
    for d, ns in D_NS:
        z0, prior, proj = draw(n, d, ns, seed=4)
        proj = np.where(proj == 0, 1.0 / 64, proj)              # (inf * 0 is a NaN: keep the projections of an inf row infinite)
        for name, puts in (("one +inf", [(n // 2, INF)]), ("one -inf", [(n - 1, -INF)]), ("+inf and -inf in different rows", [(0, INF), (n - 1, -INF)])):
            what = f"n={n} d={d} ns={ns} {dtype} {name}"
            z = z0.copy()
            for row, v in puts:
                z[row, d // 2] = v
            wl, wdz = check(z, prior, proj, dtype, what)
            rows = [r for r, _ in puts]
            assert wl == INF and not np.isfinite(wdz[rows]).any() and np.isfinite(np.delete(wdz, rows, axis=0)).all(), what
    z, prior, _ = draw(n, 1, 1, seed=5)
    z[n // 2, 0] = prior[0, 0] = INF
    wl, _ = check(z, prior, np.array([[0.5]]), dtype, f"n={n} {dtype} +inf at the top rank of both sides")
    assert math.isnan(wl)


# ---- e. NaN in prior and in proj ---------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("n", NAN_SIZES)
def test_nan_in_prior_and_in_proj(n, dtype):
    for d, ns in D_NS:
        z, prior0, proj0 = draw(n, d, ns, seed=6)
        prior = prior0.copy()
        prior[n // 2, d - 1] = NAN
        wl, wdz = check(z, prior, proj0, dtype, f"n={n} d={d} ns={ns} {dtype} NaN in one row of prior")
        # the NaN is the last of every projection's sorted prior values: it meets the top rank of z there and no other
        assert math.isnan(wl) and 1 <= np.isnan(wdz).all(axis=1).sum() <= ns and (np.isnan(wdz).all(axis=1) == np.isnan(wdz).any(axis=1)).all()
        proj = proj0.copy()
        proj[ns - 1, 0] = NAN
        wl, wdz = check(z, prior0, proj, dtype, f"n={n} d={d} ns={ns} {dtype} NaN in one projection")
        assert math.isnan(wl) and np.isnan(wdz).all()


# ---- f. guard bands ----------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("n", [37, 4097])
def test_guard_bands(n, dtype):
    d, ns = 3, 5
    z0, prior, proj = draw(n, d, ns, seed=7)
    zn = z0.copy()
    zn[n // 2, 1] = NAN
    P, S = native._ptr, native._stream
    for name, z in (("NaN at row n // 2", zn), ("ties", tie_cases(n, d, ns)[2]["rows 10..19 identical, rows 30..33 equal to row 5"])):
        what = f"swd n={n} {dtype} {name}"

        def call(i, o):
            poison(z, prior, proj, dtype)
            raw2("bamd_swd", (P(i["z"]), P(i["prior"]), P(i["proj"]), native._dt(i["z"]), n, d, ns, rw(n), P(o["loss"]), P(o["dz"]), S(i["z"])))
        got = both(what, call, {"z": dev(z, dtype), "prior": dev(prior, dtype), "proj": dev(proj, dtype)},
                   {"loss": gb.poisoned((1,), F64, "cuda"), "dz": gb.poisoned((n, d), dtype, "cuda")})
        held((got["loss"], got["dz"]), swd_ref(z, prior, proj, rw(n)), dtype, what + " framed")


# ---- g. order of calls -------------------------------------------------------------------------------------------------------------
@DTYPES
def test_a_nan_call_leaves_nothing_behind(dtype):
    small, big = draw(65, 3, 5, seed=8), list(draw(8193, 3, 5, seed=8))
    big[0][4000, 1] = NAN
    first = swd(*small, dtype)
    check(*big, dtype, f"n=8193 {dtype} NaN at row 4000")
    third = swd(*small, dtype)
    assert_same_bits(third[0], first[0], f"{dtype}: loss at n=65 after a NaN call at n=8193")
    assert_same_bits(third[1], first[1], f"{dtype}: dz at n=65 after a NaN call at n=8193")
    held(third, swd_ref(*small, rw(65)), dtype, f"n=65 {dtype} after a NaN call at n=8193")


# ---- h. bamd_emd_rows up to 64 columns: one thread sorts a row (emd_partial, elementwise.hip) --------------------------------------
NARROW = pytest.mark.parametrize("c", [1, 2, 3, 24, 63, 64])


@DTYPES
@NARROW
def test_narrow_emd_parity_with_the_oracle(c, dtype):
    x, r = wide.tables(300, c, dtype)
    xs, rs = host(x), host(r)
    for n in (1, 2, 300):
        wide.close(native.emd_rows(x[:n], r[:n]).item(), orc.emd_rows(xs[:n], rs[:n]), wide.TOL, f"{n} x {c} {dtype}")


@DTYPES
@NARROW
def test_narrow_emd_rows_of_few_distinct_values(c, dtype):
    rng = np.random.default_rng(c)
    x, r = dev(rng.integers(0, 4, size=(37, c)), dtype), dev(rng.integers(0, 4, size=(37, c)), dtype)
    if torch.equal(x, r):                                     # (c = 1 or 2 could draw the same table twice; it does not with this seed)
        r = (r + 1).contiguous()
    base = native.emd_rows(x, r)
    wide.close(base.item(), orc.emd_rows(host(x), host(r)), wide.TOL, f"ties 37 x {c} {dtype}")
    assert torch.equal(native.emd_rows(wide.permuted(x, 3), wide.permuted(r, 4)), base), "columns permuted independently in x and recon"


@DTYPES
@NARROW
def test_narrow_emd_identical_tables_give_zero(c, dtype):
    x, _ = wide.tables(37, c, dtype)
    out = native.emd_rows(x, x.clone())
    assert torch.equal(out, torch.zeros(1, dtype=F64, device="cuda"))
    assert torch.equal(native.emd_rows(x, wide.permuted(x, 5)), out), "recon = x with its columns permuted"


@DTYPES
@pytest.mark.parametrize("c", [1, 24, 64])
def test_narrow_emd_nan_and_inf(c, dtype):
    """The assertions of tests/test_gpu_emd_wide.py::test_nan_and_inf, on the one-thread-per-row kernel."""
    wide.test_nan_and_inf(c, dtype)


@DTYPES
def test_narrow_emd_rows_go_round_the_grid_twice(dtype):
    """512 * 256 + 1 rows of 4 columns: the grid is capped at 512 workgroups of 256 one-row threads, so the last row is the first
    that a thread takes on its second trip round the grid-stride loop.  Entries are multiples of 2^-6 below 4, the last row's below
    1024: every |a - b|, every row mean (a division by 4) and every partial sum is exact in float64 (below 2^30 at a resolution of
    2^-8), so the result is THE sum, whatever the order, and a row counted twice or not at all changes it."""
    n, c = 512 * 256 + 1, 4
    rng = np.random.default_rng(4)
    x, r = rng.integers(0, 256, size=(n, c)) / 64.0, rng.integers(0, 256, size=(n, c)) / 64.0
    x[-1], r[-1] = [1000.0, 3.0, 2.0, 1.0], [0.0, 1.0, 2.0, 3.0]
    want = float((np.abs(np.sort(x, axis=1) - np.sort(r, axis=1)).sum(axis=1) / c).sum())
    assert want == orc.emd_rows(x, r)
    got = native.emd_rows(dev(x, dtype), dev(r, dtype)).item()
    print(f"    {n} x {c} {dtype}: kernel {got!r} exact {want!r}")
    assert got == want
    head = native.emd_rows(dev(x[:-1], dtype), dev(r[:-1], dtype)).item()
    assert want - head == 1000.0 / c, "the last row's own term"
