"""baler_amd/colbox.py without a GPU: np.histogram stands in for bamd_column_hist.  quartiles against np.percentile bit for bit,
select against np.sort, box_stats against matplotlib.cbook.boxplot_stats on every column of every case, the round bound, a two-rank
split, and the fixture g22 (what the unmodified reference drew)."""
import os

import numpy as np
import pytest

import colbox_cases as cc
from baler_amd import colbox, native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])


@DTYPES
def test_key_maps(dtype):
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.standard_normal(500), [0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-40, 1e-310, -1e-310]]).astype(dtype)
    k = colbox.okey(x)
    order = np.argsort(x, kind="stable")
    assert (np.diff(k[order].astype(object)) >= 0).all()
    assert ((np.diff(k[order].astype(object)) == 0) == (np.diff(x[order]) == 0)).all()
    np.testing.assert_array_equal(colbox.unkey(k, dtype), x)
    assert colbox.okey(np.array([-0.0], dtype))[0] == colbox.okey(np.array([0.0], dtype))[0]
    assert not np.signbit(colbox.unkey(colbox.okey(np.array([-0.0], dtype)), dtype))[0]
    below = int(colbox.okey(np.array([0.0], dtype))[0]) - 1
    assert np.signbit(colbox.unkey(below, dtype)) and colbox.unkey(below, dtype) == 0


@DTYPES
def test_bracket_edges(dtype):
    key = lambda v: int(colbox.okey(np.array([v], dtype))[0])      # noqa: E731
    keys, edges = colbox.bracket_edges(key(-1e-3), key(1e-3), dtype)
    assert len(keys) == len(edges) <= 1025 and keys[0] == key(-1e-3) and keys[-1] == key(1e-3) + 1
    assert (np.diff(edges) > 0).all() and edges.dtype == np.float64            # -0 / +0 merged
    assert abs(edges[len(edges) // 2]) < np.finfo(dtype).tiny                  # through the subnormals
    keys, edges = colbox.bracket_edges(key(1.0), key(np.inf), dtype)
    assert edges[-1] == np.inf and (np.diff(edges) > 0).all()
    keys, edges = colbox.bracket_edges(key(1.0), key(1.0) + 2, dtype)
    assert keys == [key(1.0) + i for i in range(4)]


@DTYPES
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 100, 101, 1000, 4099])
def test_quartiles_equal_np_percentile(n, dtype):
    rng = np.random.default_rng(n)
    for kind in ("gauss", "ties", "zeros"):
        x = rng.standard_normal(n) * 1e-3
        if kind == "ties":
            x = np.round(rng.standard_normal(n) * 8) / 64           # multiples of 2^-6
        if kind == "zeros":
            x[rng.integers(0, n, max(1, n // 10))] = 0.0
            x[::3] *= -1                                            # zeros of both signs
        x = x.astype(dtype)
        want = np.percentile(x, [25, 50, 75])
        s = np.sort(x)
        stats = s[colbox.quartile_ranks([n])[0]][None, :]
        got = colbox.quartiles(stats, [n], dtype)[0]
        assert got.dtype == want.dtype
        np.testing.assert_array_equal(got, want, err_msg=f"{kind} n={n}")      # (the keys carry one zero: its sign is not compared)


def _all_cases():
    for dtype in (np.float64, np.float32):
        for name, (b, a) in cc.seeded_cases(dtype).items():
            yield f"{name}-{np.dtype(dtype).name}", dtype, b, a


def _g22(golden, tag):
    g = golden("g22_boxplot.npz")
    return g, g[f"before_{tag}"], g[f"after_{tag}"]


@DTYPES
def test_select_equals_np_sort(dtype):
    worst = 0
    for name, (b, a) in cc.seeded_cases(dtype).items():
        resid = cc.residual(b, a, cc.cut_of(b.shape[1]))
        count, mn, mx = cc.moments(resid)
        ok = [len(resid) > 0 and not np.isnan(resid[:, k]).any() for k in range(resid.shape[1])]
        n = len(resid)
        ranks = np.array([sorted({0, n // 4, n // 2, (3 * n) // 4, max(n - 1, 0)}) if o else [] for o in ok], dtype=object)
        width = max([len(r) for r in ranks] + [1])
        rk = np.full((len(ok), width), -1, np.int64)
        for k, r in enumerate(ranks):
            rk[k, :len(r)] = r
        with np.errstate(all="ignore"):
            lo, hi = mn.astype(dtype), mx.astype(dtype)
        kmin = [int(v) if o else 1 for v, o in zip(colbox.okey(lo), ok)]
        kmax = [int(v) if o else 0 for v, o in zip(colbox.okey(hi), ok)]
        vals, info = colbox.select(rk, count, kmin, kmax, cc.np_hist(resid), dtype)
        for k, o in enumerate(ok):
            if not o:
                continue
            s = np.sort(resid[:, k])
            for j in range(width):
                if rk[k, j] >= 0:
                    assert vals[k, j] == s[rk[k, j]], f"{name} column {k} rank {rk[k, j]}: {vals[k, j]} != {s[rk[k, j]]}"
            assert info["non_nan"][k] == n
        assert info["rounds"] <= colbox.round_bound(dtype, width), name
        worst = max(worst, info["rounds"])
    print(f"{np.dtype(dtype).name}: at most {worst} rounds")


@DTYPES
def test_round_bound_of_one_target(dtype):
    """One target per column has all 1024 bins of every round: 7 rounds for float64 keys, 4 for float32."""
    assert colbox.round_bound(np.float64) == 7 and colbox.round_bound(np.float32) == 4
    assert colbox.round_bound(np.float64, 6) == 9 and colbox.round_bound(np.float32, 6) == 4
    assert colbox.round_bound(np.float64, 2, shared_first=False) == 8 and colbox.round_bound(np.float32, 2, shared_first=False) == 4
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal((4099, 3)) * 1e-3, np.full((1, 3), 1e30), np.full((1, 3), -1e30)]).astype(dtype)
    count, mn, mx = cc.moments(x)
    kmin, kmax = [int(v) for v in colbox.okey(mn.astype(dtype))], [int(v) for v in colbox.okey(mx.astype(dtype))]
    for r in (0, 1, 2050, 4099, 4100):
        vals, info = colbox.select(np.full((3, 1), r), count, kmin, kmax, cc.np_hist(x), dtype)
        np.testing.assert_array_equal(vals[:, 0], np.sort(x, axis=0)[r])
        assert info["rounds"] <= colbox.round_bound(dtype) and info["extra"] == 0


def test_box_stats_equal_boxplot_stats():
    for what, dtype, b, a in _all_cases():
        resid = cc.residual(b, a, cc.cut_of(b.shape[1]))
        count, mn, mx = cc.moments(resid)
        got, info = colbox.box_stats(count, mn, mx, cc.np_hist(resid), dtype)
        cc.check_box(got, resid, what)
        assert info["quartile_rounds"] <= colbox.round_bound(dtype, 6) and info["whisker_rounds"] <= colbox.round_bound(dtype, 2, shared_first=False), what
        assert info["extra_calls"] <= 3, what


@pytest.mark.parametrize("tag, dtype", [("f64", np.float64), ("f32", np.float32)])
def test_g22_holds_what_the_reference_drew(golden, tag, dtype):
    g, b, a = _g22(golden, tag)
    assert str(g["source"]) == "reference plot_box_and_whisker, unmodified" and b.dtype == dtype
    resid = cc.residual(b, a, (3, 1e-6))
    np.testing.assert_array_equal(g[f"stats_{tag}"], cc.want_box(resid))          # matplotlib here computes what it computed there
    count, mn, mx = cc.moments(resid)
    got, _ = colbox.box_stats(count, mn, mx, cc.np_hist(resid), dtype)
    np.testing.assert_array_equal(np.stack([got[k] for k in colbox.BOX_KEYS[:5]], axis=1), g[f"stats_{tag}"])
    edge = got["box_edge"]
    np.testing.assert_array_equal(np.array([-edge - edge * 0.1, edge + edge * 0.1]), g[f"xlim_{tag}"])


@DTYPES
def test_two_rank_split_sums_to_the_same_result(dtype):
    b, a = cc.seeded_cases(dtype)["gauss4099"]
    resid = cc.residual(b, a, None)
    count, mn, mx = cc.moments(resid)
    one, info1 = colbox.box_stats(count, mn, mx, cc.np_hist(resid), dtype)
    h0, h1 = cc.np_hist(resid[:1500]), cc.np_hist(resid[1500:])
    two, info2 = colbox.box_stats(count, mn, mx, lambda e: h0(e) + h1(e), dtype)
    for k in colbox.BOX_KEYS:
        np.testing.assert_array_equal(one[k], two[k])
    assert info1 == info2
    cc.check_box(two, resid, "two ranks")


def test_header_and_symbols():
    with open(os.path.join(REPO, "include", "baler_amd.h")) as f:
        flat = " ".join(f.read().replace("*", " ").split())
    assert "n_ed < 0: per-column residual bins" in flat
    assert len(native.SYMBOLS) == 38
