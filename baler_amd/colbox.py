"""Box-and-whisker statistics of the report mode by exact selection: the host side (numpy only).

plotting.plot_box_and_whisker (plotting.py:76-98) draws, per column, matplotlib's boxplot_stats of the residual: the quartiles
(np.percentile, linear interpolation between two order statistics) and the whiskers (the extreme residuals inside the fences
q1 - 1.5 iqr, q3 + 1.5 iqr).  An order statistic of a table that is spread over row chunks and ranks is found here from integer
counts alone, which add across chunks and ranks in any order: the residual's dtype is mapped onto ordered integer keys, the key
interval that still holds the wanted rank (its bracket) is cut into bins, ``hist`` counts the residuals per bin
(bamd_column_hist with per-column edges on the GPU, np.histogram in CPU tests), and the bin that holds the rank becomes the next
bracket, until the bracket is one key.  Every decision is a pure function of the counts, so every rank takes the same path.

hist: callable, edges (c, k) float64, strictly increasing per column -> counts (c, k - 1) int64 with np.histogram's rule
(NaN and outside values not counted, last bin closed), summed over all chunks and ranks.
"""
import math

import numpy as np

BINS = 1024                     # bins of one call per column (bamd_column_hist: at most 1025 edges)
BOX_KEYS = ("box_q1", "box_med", "box_q3", "box_whislo", "box_whishi", "box_edge")


# ---- the order-preserving key maps ------------------------------------------------------------------------------------------------
def _uint(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return np.uint32, 32
    if dtype == np.float64:
        return np.uint64, 64
    raise TypeError(f"colbox: float32 or float64 expected, not {dtype}")


def okey(x):
    """float32 -> uint32, float64 -> uint64, order preserving: x < y <=> okey(x) < okey(y) for non-NaN values; -0 maps to +0's key.
    (Negative values: all bits flipped; others: the sign bit set.)"""
    x = np.asarray(x)
    ut, w = _uint(x.dtype)
    x = np.where(x == 0, np.zeros_like(x), x)
    u = x.view(ut)
    top = ut(1 << (w - 1))
    return np.where(u & top, ~u, u | top)


def unkey(k, dtype):
    """The inverse of okey: keys (array or Python int) -> values of ``dtype``.  The key just below okey(0) gives -0."""
    ut, w = _uint(dtype)
    k = np.asarray(k, dtype=ut)
    top = ut(1 << (w - 1))
    return np.where(k & top, k & ~top, ~k).astype(ut).view(np.dtype(dtype))


def _key1(v, dtype):
    return int(okey(np.asarray([v], dtype=dtype))[0])


def _val1(k, dtype):
    return unkey(np.asarray([k], dtype=_uint(dtype)[0]), dtype)[0]


def bracket_edges(klo, khi, dtype, bins=BINS):
    """The key bracket [klo, khi] cut into at most ``bins`` bins of (nearly) equal key counts.  -> (keys, edges): the m + 1 key
    boundaries (Python ints, the last one past khi) and their float64 values, exact because every boundary is a value of the
    table's dtype.  Equal edge values -- -0 and +0 -- are merged (data never carries -0's key).  A bracket that ends at
    key(+inf) closes with the edge +inf: np.histogram's closed last bin then holds +inf."""
    k_inf, k_m0 = _key1(np.inf, dtype), _key1(0.0, dtype) - 1
    n = khi - klo + 1
    m = min(bins, n)
    keys = [klo + (i * n) // m for i in range(m)] + [khi + 1]
    vals = unkey(np.array([min(k, k_inf) for k in keys], dtype=_uint(dtype)[0]), dtype).astype(np.float64).tolist()
    out_k, out_v = [], []
    for k, v in zip(keys, vals):
        if out_v and v == out_v[-1]:
            if k == k_m0 + 1 and out_k[-1] == k_m0:
                continue                      # [-0, +0): no key of the data
            if k > k_inf:
                out_k[-1] = k                 # [+inf, past +inf): the closed last edge is +inf itself
                continue
        out_k.append(k)
        out_v.append(v)
    return out_k, np.array(out_v, dtype=np.float64)


def round_bound(dtype, brackets=1, bins=BINS, shared_first=True):
    """Rounds that settle every target of a column with at most ``brackets`` distinct brackets at a time: a round cuts a bracket
    of n keys to at most ceil(n / B) keys, B = (bins + 1) // brackets - 1 (the brackets share the call's bins + 1 edges), so it
    settles log2(B) of the key's bits.  shared_first: all
    targets begin with one bracket (the column's extrema), so the first round has all ``bins``; the whiskers' two targets begin
    with brackets of their own."""
    w = _uint(dtype)[1]
    per = math.log2((bins + 1) // brackets - 1)
    if not shared_first:
        return math.ceil(w / per)
    first = math.log2(bins)
    return 1 if w <= first else 1 + math.ceil((w - first) / per)


# ---- selection --------------------------------------------------------------------------------------------------------------------
def _pad(values, k):
    """k strictly increasing float64 edges that contain ``values``: the extra ones split bins whose counts are added up again."""
    vals = list(values)
    fin = [v for v in vals if np.isfinite(v)]
    up, down = (fin[-1], fin[0]) if fin else (0.0, 0.0)
    extra = []
    while len(vals) + len(extra) < k:
        if not fin and not extra:
            extra.append(0.0)
            continue
        up = np.nextafter(up, np.inf)
        if np.isfinite(up):
            extra.append(float(up))
        else:
            down = np.nextafter(down, -np.inf)
            extra.append(float(down))
    return np.sort(np.array(vals + extra, dtype=np.float64))


def _call(hist, per_col):
    """One ``hist`` call.  per_col: for every column a sorted float64 array of >= 2 distinct edge values, or None (no request).
    -> for every column (edges, csum) with csum[i] = the count below edges[i] from edges[0] on, or None."""
    k = max([2] + [len(e) for e in per_col if e is not None])
    edges = np.stack([_pad(e if e is not None else [0.0, 1.0], k) for e in per_col])
    counts = np.asarray(hist(edges))
    if counts.shape != (len(per_col), k - 1):
        raise ValueError(f"colbox: hist returned {counts.shape} for edges {edges.shape}")
    out = []
    for c, e in enumerate(per_col):
        out.append(None if e is None else (edges[c], np.concatenate([[0], np.cumsum(counts[c].astype(np.int64))])))
    return out


def _descend(targets, hist, dtype, bins=BINS):
    """targets: per column a list of [rank, klo, khi, below] (below = the count of values under key klo; the value of that rank
    lies in the bracket).  Narrows every bracket to one key.  -> (rounds, totals): the calls made and, per column, the sum of
    the first call's counts (None for a column without targets)."""
    rounds, totals = 0, [None] * len(targets)
    first = True
    while first or any(t[1] < t[2] for col in targets for t in col):
        per_col, plans = [], []
        for col in targets:
            live = [t for t in col if first or t[1] < t[2]]
            spans = sorted({(t[1], t[2]) for t in live})
            if not spans:
                per_col.append(None)
                plans.append(None)
                continue
            share = max(1, (bins + 1) // len(spans) - 1)            # the column's edges, all brackets together, stay within bins + 1
            cut = {s: bracket_edges(s[0], s[1], dtype, share) for s in spans}
            per_col.append(np.unique(np.concatenate([cut[s][1] for s in spans])))
            plans.append((live, cut))
        res = _call(hist, per_col)
        rounds += 1
        for c, plan in enumerate(plans):
            if plan is None:
                continue
            edges, csum = res[c]
            if first:
                totals[c] = int(csum[-1])
            live, cut = plan
            for t in live:
                keys, vals = cut[(t[1], t[2])]
                at = csum[np.searchsorted(edges, vals)]             # counts below every boundary of this bracket
                inside = at - at[0] + t[3]
                b = int(np.searchsorted(inside[1:], t[0], side="right"))
                b = min(b, len(keys) - 2)                          # (a rank outside the bracket cannot happen; stay in bounds)
                t[1], t[2], t[3] = _clip_zero(keys[b], dtype, True), _clip_zero(keys[b + 1] - 1, dtype, False), int(inside[b])
        first = False
    return rounds, totals


def _clip_zero(k, dtype, up):
    """-0's key holds no data: a bracket never begins or ends on it."""
    k_m0 = _key1(0.0, dtype) - 1
    return (k + 1 if up else k - 1) if k == k_m0 else k


def _select(ranks, kmin, kmax, hist, dtype, bins, klo=None, khi=None, below=None, n_fin=None):
    """The engine behind select / box_stats.  ranks: (c, t) int64, negative = no target.  klo / khi / below: optional (c, t)
    narrower first brackets.  -> values (c, t) of ``dtype`` (NaN: no target), totals, rounds (first call included), and the
    extra call's flag."""
    ranks = np.asarray(ranks, dtype=np.int64)
    c, nt = ranks.shape
    k_inf, k_max = _key1(np.inf, dtype), _key1(np.finfo(dtype).max, dtype)
    out = np.full((c, nt), np.nan, dtype=dtype)
    # +inf among the data: np.histogram cannot tell the largest finite value from +inf in a closed last bin, so one call counts
    # the values <= the largest finite one; a rank at or past that count is +inf, the others are selected below key(+inf).
    extra = 0
    if n_fin is None:
        n_fin = [None] * c
        need = [col for col in range(c) if kmin[col] <= kmax[col] == k_inf and (ranks[col] >= 0).any()]
        if need:
            big = float(np.finfo(dtype).max)
            res = _call(hist, [np.array([-np.inf, big]) if col in need else None for col in range(c)])
            extra = 1
            for col in need:
                n_fin[col] = int(res[col][1][-1])
    targets, where = [], []
    for col in range(c):
        col_t, col_w = [], []
        if kmin[col] <= kmax[col]:
            top = min(kmax[col], k_max) if n_fin[col] is not None else kmax[col]
            for j in range(nt):
                r = int(ranks[col, j])
                if r < 0:
                    continue
                if n_fin[col] is not None and r >= n_fin[col]:
                    out[col, j] = np.inf
                    continue
                lo = kmin[col] if klo is None else max(kmin[col], int(klo[col][j]))
                hi = top if khi is None else min(top, int(khi[col][j]))
                lo, hi = _clip_zero(lo, dtype, True), _clip_zero(hi, dtype, False)
                col_t.append([r, lo, hi, 0 if below is None else int(below[col][j])])
                col_w.append(j)
        targets.append(col_t)
        where.append(col_w)
    rounds, totals = 0, [None] * c
    if any(targets):
        rounds, totals = _descend(targets, hist, dtype, bins)
    for col in range(c):
        for t, j in zip(targets[col], where[col]):
            out[col, j] = _val1(t[1], dtype)
    # a column whose targets are all +inf had no selection call: its total comes from a call of its own
    alone = [col for col in range(c) if n_fin[col] is not None and not targets[col] and (ranks[col] >= 0).any()]
    if alone:
        res = _call(hist, [np.array([-np.inf, np.inf]) if col in alone else None for col in range(c)])
        extra += 1
        for col in alone:
            totals[col] = int(res[col][1][-1])
    return out, totals, rounds, extra, n_fin


def select(ranks, count, kmin, kmax, hist, dtype, bins=BINS):
    """Exact order statistics.  ranks: (c, t) 0-based ranks among the column's non-NaN values in ascending order (negative: no
    target); count: (c,) kept values per column (a column with count 0 has no targets); kmin / kmax: per column okey of the
    smallest and largest non-NaN value (Python ints; kmin > kmax: none).  -> (values (c, t) of ``dtype``, NaN where there is no
    target; info: "rounds" (selection calls; at most round_bound(dtype, brackets) of them), "extra" (0 or 1: the +inf count),
    "non_nan" (c,) the first call's total per column, -1 where no call was made)."""
    ranks = np.array(ranks, dtype=np.int64, copy=True)
    count = np.asarray(count, dtype=np.int64)
    ranks[count <= 0] = -1
    vals, totals, rounds, extra, _ = _select(ranks, list(kmin), list(kmax), hist, np.dtype(dtype).type, bins)
    return vals, {"rounds": rounds, "extra": extra, "non_nan": np.array([-1 if t is None else t for t in totals], dtype=np.int64)}


# ---- quartiles and the box ----------------------------------------------------------------------------------------------------------
_Q = np.true_divide(np.array([25, 50, 75]), 100)          # what np.percentile makes of its argument


def quartile_ranks(n):
    """n: (c,) value counts -> (c, 6) int64: the two order statistics (lower, upper) that np.percentile's linear method reads for
    25, 50 and 75 %; -1 where n = 0."""
    n = np.asarray(n, dtype=np.int64).reshape(-1, 1)
    vi = n * _Q + (1 - _Q) - 1                             # numpy's virtual index with alpha = beta = 1
    lo = np.clip(np.floor(vi).astype(np.int64), 0, np.maximum(n - 1, 0))
    hi = np.minimum(lo + 1, np.maximum(n - 1, 0))
    out = np.stack([lo, hi], axis=2).reshape(len(n), 6)
    out[n[:, 0] <= 0] = -1
    return out


def quartiles(order_stats, n, dtype):
    """np.percentile(x, [25, 50, 75]) from its order statistics.  order_stats: (c, 6) of ``dtype`` as quartile_ranks orders them;
    n: (c,).  -> (c, 3) float64.  numpy's own interpolation: the difference of the two order statistics is taken IN THE TABLE'S
    DTYPE, the rest in float64; lower + d g, and upper - d (1 - g) where g >= 0.5."""
    s = np.asarray(order_stats, dtype=dtype).reshape(-1, 3, 2)
    n = np.asarray(n, dtype=np.int64).reshape(-1, 1)
    vi = n * _Q + (1 - _Q) - 1
    g = vi - np.floor(vi)
    a, b = s[:, :, 0], s[:, :, 1]
    with np.errstate(all="ignore"):
        d = np.subtract(b, a)
        r = np.add(a, d * g)
        r = np.where(g >= 0.5, np.subtract(b, d * (1 - g)), r)
    r = np.asarray(r, dtype=np.float64)
    r[n[:, 0] <= 0] = np.nan
    return r


def _ceil_in(v, dtype):
    """The smallest value of ``dtype`` that is >= v (float64, not NaN)."""
    f = np.asarray(v, dtype=np.float64).astype(dtype)
    return np.where(f.astype(np.float64) < v, np.nextafter(f, dtype(np.inf)), f).astype(dtype)


def _floor_in(v, dtype):
    f = np.asarray(v, dtype=np.float64).astype(dtype)
    return np.where(f.astype(np.float64) > v, np.nextafter(f, dtype(-np.inf)), f).astype(dtype)


def box_stats(count, resid_min, resid_max, hist, dtype, bins=BINS):
    """matplotlib.cbook.boxplot_stats (q1, med, q3, whislo, whishi; whis = 1.5) of every column's residual.  count, resid_min,
    resid_max: (c,) from bamd_column_moments (the extrema skip NaN).  -> (dict of BOX_KEYS: five float64 (c,) arrays and the
    scalar box_edge; info: "rounds" (all hist calls), "quartile_rounds", "whisker_rounds", "extra_calls").
    A column with a NaN residual or without kept rows gets five NaN, as boxplot_stats gives."""
    dtype = np.dtype(dtype).type
    count = np.asarray(count, dtype=np.int64)
    c = len(count)
    with np.errstate(all="ignore"):
        lo_v, hi_v = np.asarray(resid_min, dtype=np.float64).astype(dtype), np.asarray(resid_max, dtype=np.float64).astype(dtype)
    some = (count > 0) & (lo_v <= hi_v)
    kmin = [int(k) if s else 1 for k, s in zip(okey(lo_v), some)]
    kmax = [int(k) if s else 0 for k, s in zip(okey(hi_v), some)]
    ranks = quartile_ranks(count)
    ranks[~some] = -1
    stats, totals, r1, x1, n_fin = _select(ranks, kmin, kmax, hist, dtype, bins)
    # the first call counted every non-NaN residual of the column: fewer than `count` means a NaN among them
    ok = some & np.array([t is not None and t == n for t, n in zip(totals, count)])
    q = quartiles(stats, count, dtype)
    q[~ok] = np.nan
    q1, med, q3 = q[:, 0], q[:, 1], q[:, 2]
    with np.errstate(all="ignore"):
        iqr = q3 - q1
        fence_lo, fence_hi = q1 - 1.5 * iqr, q3 + 1.5 * iqr
    # whislo = the smallest residual >= fence_lo = the order statistic whose rank is the count of residuals below the fence;
    # whishi = the largest residual <= fence_hi.  One call counts both; comparisons are float64's, as numpy compares.
    want_lo, want_hi = ok & ~np.isnan(fence_lo), ok & ~np.isnan(fence_hi)
    with np.errstate(all="ignore"):
        L = _ceil_in(np.where(want_lo, fence_lo, 0.0), dtype)
        U = _floor_in(np.where(want_hi, fence_hi, 0.0), dtype)
        U_next = np.nextafter(U, dtype(np.inf)).astype(np.float64)        # count(x <= U) = count(x < the next value)
    x2 = 0
    wr = np.full((c, 2), -1, dtype=np.int64)
    klo = [[kmin[k], kmin[k]] for k in range(c)]
    khi = [[kmax[k], kmax[k]] for k in range(c)]
    below = [[0, 0] for _ in range(c)]
    if (want_lo | want_hi).any():
        per_col = []
        for k in range(c):
            th = ([float(L[k])] if want_lo[k] else []) + ([float(U_next[k])] if want_hi[k] and U[k] != np.inf else [])
            per_col.append(np.unique(np.array([-np.inf] + th + [np.inf])) if want_lo[k] or want_hi[k] else None)
        res = _call(hist, per_col)
        x2 = 1
        for k in range(c):
            if res[k] is None:
                continue
            edges, csum = res[k]
            n = int(count[k])
            if want_lo[k]:
                r = int(csum[np.searchsorted(edges, float(L[k]))])
                if r < n:
                    wr[k, 0], klo[k][0], below[k][0] = r, _key1(L[k], dtype), r
            if want_hi[k]:
                r = n if U[k] == np.inf else int(csum[np.searchsorted(edges, float(U_next[k]))])
                if r > 0:
                    wr[k, 1], khi[k][1] = r - 1, _key1(U[k], dtype)
    wv, _, r2, x3, _ = _select(wr, kmin, kmax, hist, dtype, bins, klo=klo, khi=khi, below=below, n_fin=n_fin)
    wv = wv.astype(np.float64)
    with np.errstate(invalid="ignore"):
        whislo = np.where((wr[:, 0] < 0) | (wv[:, 0] > q1), q1, wv[:, 0])
        whishi = np.where((wr[:, 1] < 0) | (wv[:, 1] < q3), q3, wv[:, 1])
    # the half-width of the reference's x axis before its 10 % margin: Python's min / max over the whisker lines' x data in
    # matplotlib's order (q1, whislo, q3, whishi per column), which is what decides the outcome when a NaN is among them
    xs = np.stack([q1, whislo, q3, whishi], axis=1).ravel()
    edge = np.float64(max(abs(min(xs)), max(xs))) if c else np.float64(np.nan)
    result = dict(zip(BOX_KEYS, (q1, med, q3, whislo, whishi, np.asarray(edge, dtype=np.float64))))
    info = {"rounds": r1 + r2 + x1 + x2 + x3, "quartile_rounds": r1, "whisker_rounds": r2, "extra_calls": x1 + x2 + x3}
    return result, info
