"""A reference for bamd_swd that can be compared element by element, the bitonic network of csrc/bitonic.hpp in plain Python, and
inputs on which float32 and float64 sort the same keys.

swd_ref: float64 NumPy with a STABLE argsort, which is the order the kernel promises (include/baler_amd.h): NaN keys last, equal keys
in row order.  The torch restatement of tests/test_gpu_swae.py (torch.sort, not stable) has the same loss and the same gradient summed
over every group of identical rows, but hands the ranks of a tie group to its rows in another order, so single gradient elements
differ (tests/test_swd_host.py asserts both).

network: the loops, the pair indexing and the direction rule of bitonic_network / bitonic_lo / bitonic_up, written out again here
(nothing is imported from the kernel), over (key, row) pairs, with one of two exchange rules:
    parent_rule   x > y or (x == y and xi > yi): the plain compare, under which a NaN key is unordered and the network is no sort;
    total_rule    bitonic_cmpx_total: NaN is the greatest key, equal keys (all NaNs are equal) are ordered by row.
padded() pads the way swd.hip did with each rule: +inf under parent_rule, NaN under total_rule, rows n, n + 1, ...

dyadic: integer multiples of 2^-6.  With |z|, |prior| <= 4 (at most 2^8 steps of 2^-6), |proj| <= 1 (2^6 steps) and d <= 8, every
product z[i, k] * proj[s, k] is an integer multiple of 2^-12 of magnitude <= 4, and a projection (the sum of d <= 8 of them) is a
multiple of 2^-12 of magnitude <= 32: 5 + 12 = 17 bits, which float32 (24) and float64 (53) both hold exactly, as they hold every
partial sum, whatever the order of the additions.  w = sort(a) - sort(b) is a multiple of 2^-12 below 64: 18 bits, exact too.  So
  * both precisions, and the float64 reference, sort the SAME keys and form the same w;
  * distinct rows project to exactly equal keys often (2^18 possible values at most, far fewer for small scale or d = 1);
  * the only roundings left in the kernel are (T)(2 scale) and its product with w, and the ns-term sum of swd_dz_k.
proj need not have unit rows: the kernel does not care."""
import numpy as np


def swd_ref(z, prior, proj, reg_weight):
    """-> (loss, dz (n, d)) in float64; NaN / inf propagate as IEEE arithmetic has them."""
    z, prior, proj = (np.asarray(t, dtype=np.float64) for t in (z, prior, proj))
    n, ns = z.shape[0], proj.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        a = (z @ proj.T).T
        b = np.sort((prior @ proj.T).T, axis=1)
        order = np.argsort(a, axis=1, kind="stable")
        w = np.take_along_axis(a, order, axis=1) - b
        loss = reg_weight * np.mean(w * w)
        G = np.empty_like(w)
        np.put_along_axis(G, order, (2.0 * reg_weight / (ns * n)) * w, axis=1)
        dz = G.T @ proj
    return float(loss), dz


def dyadic(rng, shape, scale):
    """Integer multiples of 2^-6 in [-scale, scale], float64."""
    k = int(round(scale * 64))
    return rng.integers(-k, k + 1, size=shape).astype(np.float64) / 64.0


# ---- the network of csrc/bitonic.hpp -----------------------------------------------------------------------------------------------
def parent_rule(x, y, xi, yi):
    return x > y or (x == y and xi > yi)


def _after(x, y):
    return (not x <= y) and y == y


def total_rule(x, y, xi, yi):
    return _after(x, y) or (not _after(y, x) and xi > yi)


def padded(keys, rule):
    """(keys, rows) of length m = 2^p >= max(n, 2), padded as swd.hip pads for that rule."""
    n = len(keys)
    m = 2
    while m < n:
        m <<= 1
    pad = float("inf") if rule is parent_rule else float("nan")
    return [float(k) for k in keys] + [pad] * (m - n), list(range(m))


def network(keys, rows, rule):
    """bitonic_network(m, 0, 2, m, ...) over (key, row) pairs: -> (sorted keys, their rows).  len(keys) is a power of two."""
    key, row = list(keys), list(rows)
    m = len(key)
    assert m >= 2 and m & (m - 1) == 0 and len(row) == m
    k = 2
    while k <= m:
        j = k >> 1
        while j > 0:
            for t in range(m // 2):
                lo = 2 * t - (t & (j - 1))               # bitonic_lo
                hi = lo + j
                up = (lo & k) == 0                       # bitonic_up
                if rule(key[lo], key[hi], row[lo], row[hi]) == up:
                    key[lo], key[hi] = key[hi], key[lo]
                    row[lo], row[hi] = row[hi], row[lo]
            j >>= 1
        k <<= 1
    return key, row


# The row counts of tests/test_gpu_swd_edge.py, the smallest that reach each branch of swd.hip: the smallest networks; either side of
# a padded size; the 256-thread loops; the last sizes of the one-workgroup kernel (4095, 4096) and the first of the passes through
# global memory (4097: m = 8192, one global step); 8192 has no padding; 8193 (m = 16384) has two global steps in its last phase;
# 16385 (m = 32768).  tests/test_swd_host.py runs `network` on those up to 600.
SIZES = (2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000, 4095, 4096, 4097, 8191, 8192, 8193, 16385)
