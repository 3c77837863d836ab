"""bamd_column_hist with per-column residual bins (n_ed < 0; native.column_hist with 2-D edges_resid) against np.histogram column by
column: exact counts.  Edge arrays that are not evenly spaced (through the subnormals), that begin with -inf and end with +inf, 2 and
1025 edges; values on, just below and just above edges, NaN residuals, the row cut; accumulate, the scalar-load route, the other
histograms of the same call, the refusals, guard bands and a gated side stream."""
import ctypes

import numpy as np
import pytest
import torch

import guard_bands as gb
import stream_gate as sg
from baler_amd import native

pytestmark = pytest.mark.gpu

E_RESP = np.arange(-20, 20, 0.1)


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def same_bits(got, want, what):
    assert torch.equal(got, want), what


def key_spaced(c):
    """(c, 601) edges from about -1e-3 through the float64 subnormals and 0 to about +1e-3, another scale in every column."""
    mag = np.logspace(-3, -320, 300)
    base = np.concatenate([-mag, [0.0], mag[::-1]])
    e = np.stack([base * (1.0 + k / 1000.0) for k in range(c)])
    assert (np.diff(e, axis=1) > 0).all() and e.shape == (c, 601)
    return e


def edge_sets(c):
    col = np.arange(c, dtype=np.float64)[:, None]
    padded = []
    for k in range(c):                                     # 3 + k % 5 edges of the caller's, padded past the last one to 8
        real = list(np.linspace(-0.1, 0.1 + 0.01 * k, 3 + k % 5))
        while len(real) < 8:
            real.append(np.nextafter(real[-1], np.inf))
        padded.append(real)
    return {
        "two": np.concatenate([-0.05 - 0.001 * col, 0.05 + 0.001 * col], axis=1),
        "even1025": np.linspace(-0.2, 0.2, 1025)[None, :] * (1.0 + col / 100.0),
        "keyspaced": key_spaced(c),
        "inf": np.concatenate([np.full((c, 1), -np.inf), -0.01 * (col + 1), 0 * col, 0.02 + 0 * col, np.full((c, 1), np.inf)], axis=1),
        "padded": np.array(padded),
    }


def tables(n, c, dtype, edges, seed):
    """Gaussian residuals of width 0.05; where there are rows enough: rows with before = 0, so that the residual IS `after`, put on,
    just below and just above some edges of every column (in the table's dtype), NaN and +-inf residuals, rows that a cut drops."""
    rng = np.random.default_rng(seed)
    before = rng.normal(1.0, 2.0, (n, c))
    after = before + rng.normal(0.0, 0.05, (n, c))
    before, after = before.astype(dtype), after.astype(dtype)
    k = edges.shape[1]
    r = 0
    for j in sorted({0, 1, k // 2, k - 2, k - 1}):
        for step in (-1, 0, 1):
            if r >= n - 3:
                break
            with np.errstate(over="ignore"):
                v = edges[:, j].astype(dtype)
            if step:
                v = np.nextafter(v, dtype(step * np.inf))
            before[r], after[r] = 0, v
            r += 1
    if n > 8:
        after[n - 1, 0] = np.nan
        after[n - 2, c - 1] = np.inf
        after[n - 3, c // 2] = -np.inf
        before[n - 4, 0] = np.nan                           # NaN - x
    return before, after


def np_counts(before, after, edges, cut):
    keep = np.ones(len(before), bool) if cut is None else ~(before[:, cut[0]] < cut[1])
    with np.errstate(all="ignore"):
        resid = np.subtract(after[keep], before[keep])
    return np.stack([np.histogram(resid[:, k].astype(np.float64), bins=edges[k])[0] for k in range(before.shape[1])]).astype(np.int64)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("c", [1, 3, 6, 24, 86, 128])
@pytest.mark.parametrize("n", [1, 17, 257, 4099])
def test_against_numpy(n, c, dtype):
    for name, edges in edge_sets(c).items():
        before, after = tables(n, c, dtype, edges, 100 * c + n)
        bd, ad, ed = dev(before), dev(after), dev(edges)
        caught = 0
        for cut in (None, (min(3, c - 1), -1.5)):
            want = np_counts(before, after, edges, cut)
            got = native.column_hist(bd, ad, edges_resid=ed, cut=cut)
            assert set(got) == {"resid"} and tuple(got["resid"].shape) == (c, edges.shape[1] - 1)
            np.testing.assert_array_equal(got["resid"].cpu().numpy(), want, err_msg=f"{name} n={n} c={c} cut={cut}")
            caught += int(want.sum())
        if n >= 17:
            assert caught > 0, f"{name}: the bins caught nothing"


@pytest.mark.parametrize("c, dtype", [(24, np.float64), (3, np.float32)], ids=["24xf64", "3xf32-odd-rows"])
def test_accumulate_over_chunks_equals_one_call(c, dtype):
    """Chunks of 1001 rows: in the 3-column float32 table every second chunk begins at an odd row, 12 bytes off a 16-byte boundary:
    the scalar-load route."""
    n = 4099
    edges = key_spaced(c)
    before, after = tables(n, c, dtype, edges, 5)
    bd, ad, ed = dev(before), dev(after), dev(edges)
    cut = (min(3, c - 1), -1.5)
    whole = native.column_hist(bd, ad, edges_resid=ed, cut=cut)
    np.testing.assert_array_equal(whole["resid"].cpu().numpy(), np_counts(before, after, edges, cut))
    acc = None
    for lo in range(0, n, 1001):
        if dtype == np.float32 and (lo // 1001) % 2:
            assert bd[lo:].data_ptr() % 16
        acc = native.column_hist(bd[lo:lo + 1001], ad[lo:lo + 1001], edges_resid=ed, cut=cut, out=acc)
    assert torch.equal(acc["resid"], whole["resid"])
    # the scalar route on its own: a chunk from an odd row on
    one = native.column_hist(bd[1:], ad[1:], edges_resid=ed, cut=cut)
    np.testing.assert_array_equal(one["resid"].cpu().numpy(), np_counts(before[1:], after[1:], edges, cut))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_beside_the_other_histograms(dtype):
    n, c = 4099, 24
    edges = edge_sets(c)["even1025"]
    before, after = tables(n, c, dtype, edges, 9)
    bd, ad = dev(before), dev(after)
    e_val = dev(np.stack([np.linspace(-8.0 - k, 9.0, 200) for k in range(c)]))
    cut = (3, -1.5)
    both = native.column_hist(bd, ad, dev(E_RESP), dev(edges), e_val, cut)
    alone = native.column_hist(bd, ad, edges_resid=dev(edges), cut=cut)
    others = native.column_hist(bd, ad, edges_resp=dev(E_RESP), edges_val=e_val, cut=cut)
    assert set(both) == {"resp", "resid", "before", "after"}
    assert torch.equal(both["resid"], alone["resid"])
    for k in ("resp", "before", "after"):
        assert torch.equal(both[k], others[k]) and int(both[k].sum()) > 0
    again = native.column_hist(bd, ad, dev(E_RESP), dev(edges), e_val, cut, out=both)
    assert torch.equal(again["resid"], 2 * alone["resid"]) and torch.equal(again["resp"], 2 * others["resp"])


def test_abi_refusals_and_no_rows():
    L = native.lib()
    INVALID = -1
    x = torch.ones((8, 4), dtype=torch.float64, device="cuda")
    e = dev(np.tile(np.array([-1.0, 0.0, 1.0]), (4, 1)))
    cnt = torch.full((4, 2), 5, dtype=torch.int64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    null = ctypes.c_void_p(0)

    def hist(n=8, n_ed=-3, acc=0):
        return L.bamd_column_hist(p(x), p(x), 1, n, 4, -1, 0.0, null, 0, null, p(e), n_ed, p(cnt), null, 0, null, null, acc, null)

    for bad in (-1, -1026, 0, 1, 1026):
        assert hist(n_ed=bad) == INVALID
        assert b"bamd_column_hist" in L.bamd_last_error() and b"n_ed" in L.bamd_last_error()
    torch.cuda.synchronize()
    assert (cnt == 5).all()                          # a refusal writes nothing
    assert hist(n=0, acc=1) == 0
    torch.cuda.synchronize()
    assert (cnt == 5).all()
    assert hist(n=0) == 0
    torch.cuda.synchronize()
    assert (cnt == 0).all()
    assert hist() == 0 and hist(acc=1) == 0
    torch.cuda.synchronize()
    assert cnt[:, 1].eq(16).all() and cnt[:, 0].eq(0).all()      # residual 0 sits in [0, 1]
    with pytest.raises(native.NativeError):
        native.column_hist(x, x, edges_resid=e[:3])              # one edge array per column
    with pytest.raises(native.NativeError):
        native.column_hist(x, x, edges_resid=e, out={"resid": cnt[:, :1].contiguous()})


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_inside_guard_bands(dtype):
    n, c = 257, 24
    edges = key_spaced(c)
    before, after = tables(n, c, dtype, edges, 3)
    bd, ad, ed = dev(before), dev(after), dev(edges)
    plain = native.column_hist(bd, ad, edges_resid=ed)["resid"]
    np.testing.assert_array_equal(plain.cpu().numpy(), np_counts(before, after, edges, None))
    for lead in (0, 1, 3):
        (bv, ba), (av, aa), (ev, ea) = gb.framed(bd, lead), gb.framed(ad, lead), gb.framed(ed, lead)
        snaps = [t.clone() for t in (ba, aa, ea)]
        ov, oa = gb.framed(torch.zeros_like(plain), lead)
        native.column_hist(bv, av, edges_resid=ev, out={"resid": ov})
        torch.cuda.synchronize()
        gb.assert_guards_intact(oa, lead, c, f"counts lead={lead}")
        for arena, snap, what in zip((ba, aa, ea), snaps, ("before", "after", "edges")):
            gb.assert_inputs_untouched(arena, snap, what)
        assert torch.equal(ov, plain)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_on_a_gated_side_stream(dtype):
    n, c = 4099, 24
    edges = edge_sets(c)["even1025"]
    before, after = tables(n, c, dtype, edges, 4)
    plain = native.column_hist(dev(before), dev(after), edges_resid=dev(edges))["resid"]

    def seq(t):
        o = {"resid": sg.out((c, edges.shape[1] - 1), torch.int64), "resid2": sg.out((c, edges.shape[1] - 1), torch.int64)}
        L = native.lib()
        P = lambda x: ctypes.c_void_p(x.data_ptr())      # noqa: E731
        S = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        code = 1 if dtype == np.float64 else 0
        for name, acc in (("resid", 0), ("resid2", 0), ("resid2", 1)):
            rc = L.bamd_column_hist(P(t["x"]), P(t["r"]), code, n, c, -1, 0.0, None, 0, None, P(t["edges"]), -edges.shape[1], P(o[name]),
                                    None, 0, None, None, acc, S)
            assert rc == 0, L.bamd_last_error()
        return o

    res = sg.run_gated(seq, {"x": dev(before), "r": dev(after), "edges": dev(edges)}, kinds={"edges": "edges"}, same={None: same_bits},
                       what="per-column hist")
    assert torch.equal(res["outs"]["resid"], plain) and torch.equal(res["outs"]["resid2"], 2 * plain)
