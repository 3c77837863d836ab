"""bamd_swd, the parts a machine without a GPU can check (tests/swd_ref.py):
  * swd_ref, the stable-sort reference of tests/test_gpu_swd_edge.py, against the torch restatement of tests/test_gpu_swae.py: equal
    where no two rows tie (NaN and +inf included), equal in the loss and in every tie group's gradient SUM where rows tie, and
    different in single elements there -- which is why the GPU edge tests compare with swd_ref;
  * the bitonic network of csrc/bitonic.hpp under the total order of bitonic_cmpx_total: a stable sort with NaN last, whatever the
    keys hold, with every real row among the first n ranks;
  * the same network under the plain compare that swd.hip used before: with one NaN among the keys it puts padding among the first
    n ranks (the kernel then scattered through a row index >= n, out of the projection's row of G) and loses the NaN into the
    padding (the loss then came out finite).  That is the evidence that the GPU tests would fail on that kernel; it is not run
    there, because the failure is an out-of-bounds store.
Errors are measured as max|got - want| / max|want| over a tensor (maxerr of tests/test_gpu_parity.py)."""
import math

import numpy as np

from swd_ref import SIZES, dyadic, network, padded, parent_rule, swd_ref, total_rule
from test_gpu_swae import _swd_ref

TOL = 1e-13
HOST_SIZES = [n for n in SIZES if n <= 600]           # (larger networks cost too much in plain Python)


def gaussian(seed, n=64, d=5, ns=7):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, d)) * 0.3 + 0.1, rng.normal(size=(n, d)), rng.normal(size=(ns, d))


def classes(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    return np.where(np.isnan(a), 1, np.where(a == np.inf, 2, np.where(a == -np.inf, 3, 0)))


def same(got, want, what):
    """Same non-finite classes everywhere, finite elements within TOL of the largest finite magnitude."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(classes(got), classes(want)), what + ": NaN / inf classes"
    fin = classes(want) == 0
    if fin.any():
        err = np.abs(got[fin] - want[fin]).max() / max(np.abs(want[fin]).max(), 1e-300)
        print(f"    {what}: {err:.3e} (bar {TOL:g})")
        assert err <= TOL, what


def test_swd_ref_equals_the_torch_restatement_without_ties():
    z, prior, proj = gaussian(1)
    for name, edit in (("finite", lambda z: None), ("NaN", lambda z: z.__setitem__((9, 2), np.nan)),
                       ("+inf", lambda z: z.__setitem__((40, 0), np.inf)),
                       ("NaN and +inf", lambda z: (z.__setitem__((9, 2), np.nan), z.__setitem__((40, 0), np.inf)))):
        zz = z.copy()
        edit(zz)
        loss, dz = swd_ref(zz, prior, proj, 0.7)
        tl, tdz = _swd_ref(zz, prior, proj, 0.7)
        same(loss, tl, name + " loss")
        same(dz, tdz, name + " dz")
        if name == "finite":
            assert math.isfinite(loss) and np.isfinite(dz).all()
        if name == "NaN":
            assert math.isnan(loss) and np.isnan(dz[9]).all() and not np.isnan(np.delete(dz, 9, axis=0)).any()
        if name == "+inf":
            assert loss == np.inf and not np.isfinite(dz[40]).any() and np.isfinite(np.delete(dz, 40, axis=0)).all()


def test_with_ties_only_group_sums_agree():
    z, prior, proj = gaussian(2)
    z[10:20] = z[10]
    z[30:34] = z[5]
    groups = (list(range(10, 20)), [5, 30, 31, 32, 33])
    loss, dz = swd_ref(z, prior, proj, 0.7)
    tl, tdz = _swd_ref(z, prior, proj, 0.7)
    same(loss, tl, "ties loss")
    rest = [r for r in range(64) if not any(r in g for g in groups)]
    same(dz[rest], tdz[rest], "ties: rows outside the groups")
    scale, apart = np.abs(dz).max(), []
    for g in groups:
        err = np.abs(dz[g].sum(0) - tdz[g].sum(0)).max() / scale
        apart.append(np.abs(dz[g] - tdz[g]).max() / scale)
        print(f"    group of {len(g)} rows: sum {err:.3e} (bar {TOL:g}), single elements {apart[-1]:.3e}")
        assert err <= TOL
    # torch.sort hands a tie group's ranks to its rows in another order than a stable sort does
    assert max(apart) > 1e-6, "the two references agree element by element on ties: nothing to tell them apart"


def key_sets(n):
    """name -> n keys: the inputs of the GPU edge tests, as one projection sees them."""
    rng = np.random.default_rng(n)
    real = rng.normal(size=n)

    def with_(at, v):
        k = real.copy()
        k[list(at)] = v
        return k
    return {"NaN at row 0": with_([0], np.nan), "NaN in the middle": with_([n // 2], np.nan), "NaN at row n-1": with_([n - 1], np.nan),
            "two NaNs": with_([0, n - 1], np.nan), "all NaN": np.full(n, np.nan), "+inf": with_([n // 2], np.inf),
            "-inf": with_([n // 2], -np.inf), "+inf and NaN": np.where(np.arange(n) % 2 == 0, np.inf, np.nan),
            "all equal": np.full(n, 0.25), "dyadic, many ties": dyadic(rng, n, 3 / 64)}


def test_network_with_the_total_order_is_a_stable_sort():
    for n in HOST_SIZES:
        for name, keys in key_sets(n).items():
            key, row = network(*padded(keys, total_rule), total_rule)
            what = f"n={n} {name}"
            assert sorted(row[:n]) == list(range(n)), what + ": the first n ranks are not the n real rows"
            assert row[:n] == list(np.argsort(keys, kind="stable")), what + ": not the stable order"
            assert np.array_equal(np.asarray(key[:n]), keys[row[:n]], equal_nan=True), what + ": keys parted from their rows"
            assert all(math.isnan(k) for k in key[n:]) and row[n:] == list(range(n, len(row))), what + ": padding"


def test_network_with_the_plain_compare_misplaces_padding_and_loses_the_nan():
    cases = pad_in = nan_lost = unsorted = 0
    for n in HOST_SIZES:
        for name, keys in key_sets(n).items():
            if np.isnan(keys).sum() != 1:
                continue
            key, row = network(*padded(keys, parent_rule), parent_rule)
            cases += 1
            pad_in += any(r >= n for r in row[:n])
            nan_lost += not any(math.isnan(k) for k in key[:n])
            unsorted += row[:n] != list(np.argsort(keys, kind="stable"))
    print(f"    plain compare, one NaN, n in {HOST_SIZES}: {cases} cases, padding among the first n ranks in {pad_in}, "
          f"NaN at a rank >= n in {nan_lost}, not the stable order in {unsorted}")
    assert pad_in >= 1, "no case puts a row index >= n among the first n ranks"
    assert nan_lost >= 1, "no case puts the NaN at a rank >= n"
    # how often: one NaN at a random row among n Gaussian keys, 20 draws per n (with the total order: never, checked beside it)
    ns_, draws, pad_in, nan_lost = (3, 5, 37, 40, 100, 129, 600), 20, 0, 0
    rng = np.random.default_rng(0)
    for n in ns_:
        for _ in range(draws):
            keys = rng.normal(size=n)
            keys[rng.integers(n)] = np.nan
            key, row = network(*padded(keys, parent_rule), parent_rule)
            pad_in += any(r >= n for r in row[:n])
            nan_lost += not any(math.isnan(k) for k in key[:n])
            assert network(*padded(keys, total_rule), total_rule)[1][:n] == list(np.argsort(keys, kind="stable"))
    print(f"    plain compare, one NaN at a random row, n in {ns_}, {draws} draws each: padding among the first n ranks in {pad_in} of "
          f"{len(ns_) * draws}, NaN at a rank >= n in {nan_lost} of {len(ns_) * draws}")
    assert pad_in >= 1 and nan_lost >= 1
    # the same inputs without the NaN: the plain compare sorts them
    for n in HOST_SIZES:
        keys = np.random.default_rng(n).normal(size=n)
        assert network(*padded(keys, parent_rule), parent_rule)[1][:n] == list(np.argsort(keys, kind="stable"))
