"""bamd_column_moments / bamd_column_hist on the GPU against the reference's own plot_1D run (fixture g21) and against numpy:
counts and extrema bit for bit, sums within the library's fp64 bar of 1e-11."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from baler_amd import native
from baler_amd.modules import helper

pytestmark = pytest.mark.gpu

TOL = 1e-11         # the project's fp64 bar: a strided per-thread sum + fixed trees over <= 1e7 values errs by ~1e-14 relative
E_RESP, E_RESID = np.arange(-20, 20, 0.1), np.arange(-1, 1, 0.01)
_POOL = ThreadPoolExecutor(16)


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def np_moments(before, after, cut):
    """numpy's statistics of plot_1D in the tables' dtype (plotting.py:118-123, 143-147), sums taken in float64.
    -> dict of MOMENT_ROWS plus abs_* sums that scale the tolerances."""
    keep = np.ones(len(before), bool) if cut is None else ~(before[:, cut[0]] < cut[1])
    b, a = before[keep], after[keep]
    with np.errstate(all="ignore"):
        resid = np.subtract(a, b)
        resp = np.divide(resid, b) * 100
        f64 = dict(axis=0, dtype=np.float64)
        r = {"count": np.full(before.shape[1], keep.sum(), np.float64),
             "resid_sum": resid.sum(**f64), "resid_sumsq": np.square(resid).sum(**f64),
             "resp_sum": resp.sum(**f64), "resp_sumsq": np.square(resp).sum(**f64),
             "abs_resid": np.abs(resid).sum(**f64), "abs_resp": np.abs(resp).sum(**f64)}
        for name, v in (("resid", resid), ("before", b), ("after", a), ("sum", b + a)):
            r[name + "_min"] = np.fmin.reduce(v.astype(np.float64), axis=0, initial=np.inf)      # NaN skipped
            r[name + "_max"] = np.fmax.reduce(v.astype(np.float64), axis=0, initial=-np.inf)
    return r, resid, resp, b, a


def check_sums(got, ref, what):
    """|sum - numpy's| <= 1e-11 * sum |v| (i.e. the mean within 1e-11 of mean |v|), sums of squares within 1e-11 relative;
    a non-finite reference value must be reproduced as it is."""
    worst = 0.0
    for key, scale in (("resid_sum", "abs_resid"), ("resid_sumsq", "resid_sumsq"), ("resp_sum", "abs_resp"), ("resp_sumsq", "resp_sumsq")):
        g, w, s = got[key], ref[key], ref[scale]
        fin = np.isfinite(w) & np.isfinite(s)
        np.testing.assert_array_equal(g[~fin], w[~fin], err_msg=f"{what} {key} (non-finite)")
        err = np.abs(g[fin] - w[fin]) / np.maximum(s[fin], 1e-300)
        err = err[s[fin] > 0]
        if err.size:
            worst = max(worst, float(err.max()))
        assert (np.abs(g[fin] - w[fin]) <= TOL * s[fin]).all(), f"{what} {key}: {err.max() if err.size else 0:.3e}"
    return worst


def check_exact(got, ref, what):
    for key in ("count", "resid_min", "resid_max", "before_min", "before_max", "after_min", "after_max", "sum_min", "sum_max"):
        np.testing.assert_array_equal(got[key], ref[key], err_msg=f"{what} {key}")


def raw_dict(raw):
    return dict(zip(native.MOMENT_ROWS, raw.cpu().numpy()))


def value_edges(ref, dtype):
    with np.errstate(all="ignore"):
        return np.stack([np.asarray(helper.report_value_edges(dtype(lo), dtype(hi)), np.float64)
                         for lo, hi in zip(ref["sum_min"], ref["sum_max"])])


def np_hists(resid, resp, b, a, e_val):
    """np.histogram with explicit bins, column by column (threads: numpy's sort releases the GIL)."""
    c = b.shape[1]

    def col(k):
        usable = np.all(np.diff(e_val[k]) >= 0)          # np.histogram refuses non-monotonic (NaN) bins: nothing to count there
        zero = np.zeros(e_val.shape[1] - 1, np.int64)
        return (np.histogram(resp[:, k], bins=E_RESP)[0], np.histogram(resid[:, k], bins=E_RESID)[0],
                np.histogram(b[:, k], bins=e_val[k])[0] if usable else zero,
                np.histogram(a[:, k], bins=e_val[k])[0] if usable else zero)
    out = list(_POOL.map(col, range(c)))
    return {name: np.stack([o[i] for o in out]).astype(np.int64) for i, name in enumerate(("resp", "resid", "before", "after"))}


def gpu_hists(bd, ad, e_val, cut, **kw):
    return native.column_hist(bd, ad, dev(E_RESP), dev(E_RESID), dev(e_val), cut, **kw)


def check_counts(got, want, what):
    for name in ("resp", "resid", "before", "after"):
        np.testing.assert_array_equal(got[name].cpu().numpy(), want[name], err_msg=f"{what} counts {name}")


# ---- the reference's own run -----------------------------------------------------------------------------------------------------
def test_fixture_parity(golden):
    g = golden("g21_colstats.npz")
    before, after, cut = g["before"], g["after"], (3, 1e-6)
    bd, ad = dev(before), dev(after)
    raw = native.column_moments_raw(bd, ad, cut)
    s = native.moments_summary(raw)
    ref, resid, resp, b, a = np_moments(before, after, cut)

    # every histogram the reference drew, every bin
    for k in range(6):
        np.testing.assert_array_equal(helper.report_value_edges(s["sum_min"][k], s["sum_max"][k]), g["edges_before"][k])
    counts = native.column_hist(bd, ad, dev(g["edges_response"][0]), dev(g["edges_residual"][0]), dev(g["edges_before"]), cut)
    np.testing.assert_array_equal(counts["resp"].cpu().numpy(), g["counts_response"])
    np.testing.assert_array_equal(counts["resid"].cpu().numpy(), g["counts_residual"])
    np.testing.assert_array_equal(counts["before"].cpu().numpy(), g["counts_before"])
    np.testing.assert_array_equal(counts["after"].cpu().numpy(), g["counts_after"])

    # extrema: bit for bit numpy's, and the reference's label text
    check_exact(raw_dict(raw), ref, "g21")
    np.testing.assert_array_equal(np.round(s["resid_max"], 6), g["resid_max_rounded"])
    np.testing.assert_array_equal(np.round(s["resid_min"], 6), g["resid_min_rounded"])

    # means and RMS: the recorded values and numpy's float64 ones
    worst = check_sums(raw_dict(raw), ref, "g21")
    with np.errstate(all="ignore"):
        for key, rec, v in (("resid_mean", g["resid_mean"], resid), ("resp_mean", g["resp_mean"], resp)):
            scale = np.abs(v).mean(axis=0)
            fin = np.isfinite(rec) & np.isfinite(scale)
            np.testing.assert_array_equal(s[key][~fin], rec[~fin])
            err = np.abs(s[key][fin] - rec[fin]) / scale[fin]
            print(f"g21 {key}: worst error relative to mean|v| {err.max():.3e}")
            assert (err <= TOL).all()
        for key, rec, digits, v in (("resid_rms", g["resid_rms_rounded"], 6, resid), ("resp_rms", g["resp_rms_rounded"], 4, resp)):
            want = np.sqrt(np.mean(np.square(v), axis=0))
            fin = np.isfinite(want)
            np.testing.assert_array_equal(s[key][~fin], want[~fin])
            np.testing.assert_array_equal(rec[~fin], want[~fin])
            err = np.abs(s[key][fin] - want[fin]) / want[fin]
            print(f"g21 {key}: worst relative error {err.max():.3e}")
            assert (err <= TOL).all()
            assert (np.abs(s[key][fin] - rec[fin]) <= 0.5000001 * 10.0 ** -digits + TOL * want[fin]).all()   # the label is round(rms, digits)
    print(f"g21 sums: worst error relative to sum|v| {worst:.3e}")


# ---- numpy on seeded tables ------------------------------------------------------------------------------------------------------
def seeded(n, c, dtype, seed):
    rng = np.random.default_rng(seed)
    before = rng.normal(1.0, 2.0, (n, c))
    before[:, c // 2] = rng.exponential(1e-3, n)                       # small values: large responses
    after = before + rng.normal(0.0, 0.05, (n, c)) * rng.uniform(0.1, 3.0, c)
    return before.astype(dtype), after.astype(dtype)


@pytest.mark.parametrize("with_cut", [False, True], ids=["nocut", "cut"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("c", [1, 3, 24, 61, 128])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 1_000_003])
def test_against_numpy(n, c, dtype, with_cut):
    before, after = seeded(n, c, dtype, 1000 * c + n % 977)
    cut = (min(3, c - 1), -1.5) if with_cut else None                  # drops ~10 % of the rows
    what = f"n={n} c={c} {np.dtype(dtype).name} cut={cut}"
    ref, resid, resp, b, a = np_moments(before, after, cut)
    bd, ad = dev(before), dev(after)
    raw = raw_dict(native.column_moments_raw(bd, ad, cut))
    check_exact(raw, ref, what)
    worst = check_sums(raw, ref, what)
    e_val = value_edges(ref, dtype)
    check_counts(gpu_hists(bd, ad, e_val, cut), np_hists(resid, resp, b, a, e_val), what)
    print(f"{what}: worst sum error {worst:.3e}")


# ---- edge semantics --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_edge_semantics(dtype):
    rng = np.random.default_rng(7)
    n, c = 600, 5
    before = rng.normal(2.0, 1.0, (n, c))
    after = before + rng.normal(0.0, 0.2, (n, c))
    before[3, 0], after[4, 0] = np.nan, np.nan
    before[5, 1], after[6, 1] = np.inf, -np.inf
    before[7, 2], after[7, 2] = np.inf, np.inf                          # inf - inf
    before[10:14, 4] = 0.0                                              # response +-inf ...
    after[10:12, 4] = 0.0                                               # ... and 0 / 0
    before[20, 3] = np.nan                                              # a NaN in the cut column keeps its row
    before[21:30, 3] = -5.0                                             # rows the cut drops
    before, after = before.astype(dtype), after.astype(dtype)
    # residuals exactly on edges[0], an inner edge and edges[-1] of the residual bins, and their neighbours
    for i, e in enumerate((E_RESID[0], E_RESID[77], E_RESID[-1])):
        for j, v in enumerate((np.nextafter(e, -np.inf), e, np.nextafter(e, np.inf))):
            r = 100 + 3 * i + j
            before[r, 1], before[r, 3] = 0.0, 2.0                       # (and the row passes the cut)
            after[r, 1] = dtype(v)                                      # before = 0: the residual IS after (exact in either dtype)
    cut = (3, -1.0)
    ref, resid, resp, b, a = np_moments(before, after, cut)
    bd, ad = dev(before), dev(after)
    raw = raw_dict(native.column_moments_raw(bd, ad, cut))
    check_exact(raw, ref, "edge")
    for key in ("resid_sum", "resid_sumsq", "resp_sum", "resp_sumsq"):
        fin = np.isfinite(ref[key])
        np.testing.assert_array_equal(raw[key][~fin], ref[key][~fin])   # equal_nan: NaN == NaN, inf == inf
        np.testing.assert_allclose(raw[key][fin], ref[key][fin], rtol=TOL, atol=0)
    assert not np.isfinite(ref["resp_sum"]).all() and not np.isfinite(ref["resid_sum"]).all()
    e_val = value_edges(ref, dtype)
    # values exactly on the value bins' first and last edge exist by construction (the extrema of before + after need not be
    # table values, so put before / after values ON the edges of one column)
    before2, after2 = before.copy(), after.copy()
    before2[200, 0], after2[201, 0], before2[202, 0] = dtype(e_val[0, 0]), dtype(e_val[0, -1]), dtype(e_val[0, 50])
    ref2, resid2, resp2, b2, a2 = np_moments(before2, after2, cut)
    want = np_hists(resid2, resp2, b2, a2, e_val)
    check_counts(gpu_hists(dev(before2), dev(after2), e_val, cut), want, "edge")
    if dtype == np.float64:                                             # e[0] and its upper neighbour; e[-1] and its lower one
        assert want["resid"][1, 0] >= 2 and want["resid"][1, -1] >= 2


# ---- chunked = whole -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c, dtype", [(24, np.float64), (3, np.float32)], ids=["24xf64", "3xf32-unaligned-chunks"])
def test_chunked_equals_whole(c, dtype):
    n = 100_003
    before, after = seeded(n, c, dtype, 99)
    cut = (min(3, c - 1), -1.5)
    bd, ad = dev(before), dev(after)
    whole = native.column_moments_raw(bd, ad, cut)
    ref = np_moments(before, after, cut)[0]
    e_val = value_edges(ref, dtype)
    whole_counts = gpu_hists(bd, ad, e_val, cut)

    def run(chunk):
        raw, counts = None, None
        for lo in range(0, n, chunk):
            raw = native.column_moments_raw(bd[lo:lo + chunk], ad[lo:lo + chunk], cut, out=raw)
            counts = gpu_hists(bd[lo:lo + chunk], ad[lo:lo + chunk], e_val, cut, out=counts)
        return raw, counts

    for chunk in (1001, 33_334, 65_536):                                # each with a ragged last chunk
        raw, counts = run(chunk)
        raw2, counts2 = run(chunk)
        assert torch.equal(raw, raw2), "a chunking must be bitwise repeatable"
        for k in counts:
            assert torch.equal(counts[k], counts2[k]) and torch.equal(counts[k], whole_counts[k])
        check_exact(raw_dict(raw), raw_dict(whole), f"chunk {chunk}")
        w = raw_dict(whole)
        one_call = dict(abs_resid=ref["abs_resid"], abs_resp=ref["abs_resp"], resid_sum=w["resid_sum"], resid_sumsq=w["resid_sumsq"],
                        resp_sum=w["resp_sum"], resp_sumsq=w["resp_sumsq"])
        worst = check_sums(raw_dict(raw), one_call, f"chunk {chunk}")
        print(f"chunk {chunk}: worst sum error vs one call {worst:.3e}")
    assert torch.equal(whole, native.column_moments_raw(bd, ad, cut))


# ---- ABI error paths -------------------------------------------------------------------------------------------------------------
def test_abi_error_paths():
    L = native.lib()
    INVALID, UNSUPPORTED = -1, -5
    x = torch.ones((8, 4), dtype=torch.float64, device="cuda")
    out = torch.full((13, 4), 7.0, dtype=torch.float64, device="cuda")
    e = dev(np.array([0.0, 1.0, 2.0]))
    cnt = torch.full((4, 2), 5, dtype=torch.int64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    null = ctypes.c_void_p(0)

    def mom(before=p(x), after=p(x), dtype=1, n=8, c=4, cut_col=-1, o=p(out), acc=0):
        return L.bamd_column_moments(before, after, dtype, n, c, cut_col, 0.0, o, acc, null)

    def hist(before=p(x), n=8, c=4, cut_col=-1, er=p(e), n_er=3, cr=p(cnt), acc=0):
        return L.bamd_column_hist(before, p(x), 1, n, c, cut_col, 0.0, er, n_er, cr, null, 0, null, null, 0, null, null, acc, null)

    for rc in (mom(before=null), mom(after=null), mom(c=0), mom(cut_col=4), mom(dtype=2), mom(o=null),
               hist(before=null), hist(c=0), hist(cut_col=4), hist(n_er=1), hist(n_er=1026), hist(cr=null), hist(er=null)):
        assert rc == INVALID
        assert L.bamd_last_error()
    assert b"bamd_column_hist" in L.bamd_last_error()
    assert mom(c=129) == UNSUPPORTED and hist(c=129) == UNSUPPORTED
    # n_rows = 0: fine; outputs neutral, or untouched under accumulate
    assert mom(n=0, acc=1) == 0 and hist(n=0, acc=1) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (cnt == 5).all()
    assert mom(n=0, before=null, after=null) == 0 and hist(n=0) == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[list(native.MOMENT_SUM_ROWS)] == 0).all() and (o[list(native.MOMENT_MIN_ROWS)] == np.inf).all() \
        and (o[list(native.MOMENT_MAX_ROWS)] == -np.inf).all() and (cnt == 0).all()
    assert mom() == 0 and hist() == 0
    torch.cuda.synchronize()
    assert (out[0] == 8).all() and cnt[:, 0].eq(8).all() and cnt[:, 1].eq(0).all()      # response 0 sits in bin [0, 1)
    with pytest.raises(native.NativeError):
        native.column_moments(x, x.float())
    with pytest.raises(native.NativeError):
        native.column_hist(x, x, edges_resp=e.float())
