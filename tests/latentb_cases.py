"""Shared by tests/test_latentb_host.py and tests/test_gpu_latentb.py: packed b-bit latent codes (bamd_codeb, b = 1 .. 7).  The value
set of the store rule, an independent statement of the bit layout (np.packbits), the dense cases with their seeds, and parameter
vectors folded for levels = 2**b - 1 whose codes span 0 .. 2**b - 1 and clamp at both ends."""
import numpy as np

import latent8_cases as lc
from baler_amd import latent8
from oracle import c_oracle as orc

BITS = (1, 2, 3, 4, 5, 6, 7)
BAND, BAND_SHARE = lc.BAND, lc.BAND_SHARE      # the 8-bit comparison's band; code units are no larger at fewer levels

# (name, dims, seed of formula_params, seed of the rows): latent8_cases' dense cases plus the run-time-width class AE(30, 7)
DENSE = dict(lc.DENSE)
DENSE["ae30-7"] = (orc.ae_dims(30, 7), 89, 15)
ROWS_MAX = 257
ORACLE_CASES = ("ae24-15", "ae30-7", "cfd625-7")      # the fp32 chain, a class shape and a wide shape; compared at ORACLE_BITS
ORACLE_BITS = 5


def value_set(bits):
    """float32 values for every branch of the b-bit store rule: NaN, +-inf, +-0, every tie k + 0.5 around [0, 2**b - 1] with its
    two neighbours, the integers, large magnitudes, subnormals and a random spread."""
    top = latent8.levels(bits)
    f = lambda u: np.array(u, dtype=np.uint32).view(np.float32)      # noqa: E731
    special = f([0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x7F7FFFFF, 0xFF7FFFFF])
    ties = np.arange(-3, top + 4, dtype=np.float32) + np.float32(0.5)
    off = np.concatenate([np.nextafter(ties, np.float32(np.inf)), np.nextafter(ties, np.float32(-np.inf))])
    ints = np.arange(-3, top + 4, dtype=np.float32)
    big = np.array([1e3, -1e3, 1e9, -1e9, 3e38, -3e38, 255, 256, 1e-30, -1e-30], dtype=np.float32)
    spread = np.random.default_rng(bits).uniform(-3, top + 3, size=4000).astype(np.float32)
    return np.concatenate([special, ties, off, ints, big, spread])


def qb_scalar(v, bits):
    """The store rule element by element in Python arithmetic (round() is half-to-even), independent of latent8.qb."""
    top = 2 ** bits - 1
    out = np.empty(len(v), dtype=np.uint8)
    for i, x in enumerate(np.asarray(v, dtype=np.float32)):
        x = float(x)
        out[i] = 0 if (x != x or x <= 0) else top if x >= top else round(x)
    return out


def packbits_rows(q, bits):
    """The layout rule stated through np.packbits: the row's bit matrix (code k's bit i at column k * bits + i), packed
    least-significant bit first.  Independent of latent8.pack_rows."""
    q = np.asarray(q, dtype=np.uint8)
    bitmat = ((q[:, :, None] >> np.arange(bits, dtype=np.uint8)) & 1).reshape(q.shape[0], -1).astype(np.uint8)
    return np.packbits(bitmat, axis=1, bitorder="little")


def rows(name, n=ROWS_MAX):
    """The first n of the case's rows (float64 in [0, 1)); for latent8_cases' names these are that module's rows."""
    if name in lc.DENSE:
        return lc.rows(name, n)
    dims, _, seed = DENSE[name]
    return np.random.default_rng(seed).random((ROWS_MAX, dims[0]))[:n]


_oracle = {}


def oracle_case(name):
    """-> (dims, flat, lo, rng, z): formula parameters, the clamping scale (3rd / 97th percentile) of the oracle's float64 latent z
    of the case's 257 rows."""
    if name not in _oracle:
        dims, pseed, _ = DENSE[name]
        flat = orc.formula_params(dims, pseed)
        z = orc.encode(dims, flat, rows(name))
        lo, rng = lc.clamping_scale(z)
        _oracle[name] = (dims, flat, lo, rng, z)
    return _oracle[name]


def folded_case(name, bits):
    """-> (dims, folded flat (float64, unrounded), lo, rng) for levels = 2**bits - 1."""
    dims, flat, lo, rng, _ = oracle_case(name)
    return dims, latent8.fold_flat(flat, lc.layout(dims), lo, rng, latent8.levels(bits)), lo, rng


def band_share(c, bits):
    """Share of the values within BAND of a half-integer where that decides a code (a value below -0.5 - BAND or above
    2**bits - 0.5 + BAND clamps whatever its fraction), and the mask of the values the comparison leaves out."""
    c = np.asarray(c, dtype=np.float64)
    top = latent8.levels(bits)
    near = np.abs(c - np.floor(c) - 0.5) <= BAND
    return float((near & (c > -0.5 - BAND) & (c < top + 0.5 + BAND)).mean()), near | ~np.isfinite(c)
