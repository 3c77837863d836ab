"""What tests/test_colbox_host.py and tests/test_gpu_colbox.py share: the seeded (before, after) table pairs, the references
(np.sort, matplotlib.cbook.boxplot_stats) and the comparisons."""
import matplotlib.cbook as cbook
import numpy as np

from baler_amd import colbox

STATS = ("q1", "med", "q3", "whislo", "whishi")


def cut_of(c):
    return (3, 1e-6) if c > 3 else None


def residual(before, after, cut):
    """The kept rows' residual in the tables' dtype, as plot_1D forms it (plotting.py:118-123)."""
    keep = np.ones(len(before), bool) if cut is None else ~(before[:, cut[0]] < cut[1])
    with np.errstate(all="ignore"):
        return np.subtract(after[keep], before[keep])


def moments(resid):
    """count, min and max of the residual as bamd_column_moments gives them (the extrema skip NaN)."""
    c = resid.shape[1]
    r64 = resid.astype(np.float64)
    return (np.full(c, len(resid), np.int64), np.fmin.reduce(r64, axis=0, initial=np.inf), np.fmax.reduce(r64, axis=0, initial=-np.inf))


def np_hist(resid):
    """np.histogram per column as the `hist` of colbox."""
    def hist(edges):
        assert 2 <= edges.shape[1] <= 1025 and (np.diff(edges, axis=1) > 0).all()          # what bamd_column_hist accepts
        return np.stack([np.histogram(resid[:, k].astype(np.float64), bins=edges[k])[0] for k in range(resid.shape[1])]).astype(np.int64)
    return hist


def want_box(resid):
    """(c, 5) float64: boxplot_stats of every column; an empty column gives five NaN."""
    out = np.full((resid.shape[1], 5), np.nan)
    if len(resid):
        with np.errstate(all="ignore"):
            for k in range(resid.shape[1]):
                s = cbook.boxplot_stats(resid[:, k])[0]
                out[k] = [s[x] for x in STATS]
    return out


def want_edge(box):
    """The reference's expression over the whisker lines' x data in matplotlib's order (q1, whislo, q3, whishi per column)."""
    w = np.stack([box[:, 0], box[:, 3], box[:, 2], box[:, 4]], axis=1).ravel()
    return max([abs(min(w)), max(w)])


def check_box(got, resid, what):
    want = want_box(resid)
    have = np.stack([got[k] for k in colbox.BOX_KEYS[:5]], axis=1)
    assert have.dtype == np.float64 and have.shape == want.shape, what
    np.testing.assert_array_equal(have, want, err_msg=what)          # as values: NaN equals NaN, -0 equals +0
    np.testing.assert_array_equal(np.float64(got["box_edge"]), np.float64(want_edge(want)), err_msg=what + " box_edge")


def seeded_cases(dtype):
    """name -> (before, after).  Three columns each unless named otherwise."""
    rng = np.random.default_rng(2210)
    tiny = np.finfo(dtype).smallest_subnormal
    cases = {}
    for n in (1, 2, 3, 5, 17, 257, 4099):
        b = rng.standard_normal((n, 3))
        cases[f"gauss{n}"] = (b, b + rng.standard_normal((n, 3)) * 0.05)
        b = np.round(b * 64) / 64
        cases[f"ties{n}"] = (b, b + np.round(rng.standard_normal((n, 3)) * 4) / 64)
    n = 257
    b = rng.standard_normal((n, 4))
    a = b + rng.standard_normal((n, 4)) * 0.05
    a[:, 0] = b[:, 0] + 0.25                                  # a constant column (0.25 and the summands are exact in either dtype)
    b[:, 0] = np.round(b[:, 0] * 64) / 64
    a[:, 0] = b[:, 0] + 0.25
    a[5, 1] = np.nan                                          # a column with one NaN
    b[:, 3] = np.abs(b[:, 3]) + 1.0                           # (every row passes the cut)
    cases["constant-nan"] = (b, a)
    b = rng.standard_normal((n, 3))
    a = b + rng.standard_normal((n, 3)) * 0.05
    a[0, 0], a[1, 1], a[2:200, 2], a[200:, 1] = np.inf, -np.inf, np.inf, np.inf
    a[3, 0] = -np.inf
    cases["inf"] = (b, a)
    b = rng.standard_normal((n, 4))
    b[:, 3] = -np.abs(b[:, 3])                                # all rows cut
    cases["all-cut"] = (b, b + 0.5)
    b = np.zeros((n, 3))
    cases["ulp-across-zero"] = (b, rng.integers(-3, 4, (n, 3)) * tiny * np.where(rng.random((n, 3)) < 0.5, -1.0, 1.0))
    cases["subnormal"] = (b, rng.integers(-2000, 2000, (n, 3)) * tiny)
    return {k: (np.ascontiguousarray(b.astype(dtype)), np.ascontiguousarray(a.astype(dtype))) for k, (b, a) in cases.items()}
