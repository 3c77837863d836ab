"""Shared by tests/test_latent8_host.py and tests/test_gpu_latent8.py: the value set of the store rule, the dense cases with their
seeds, and folded parameter vectors whose codes span 0..255 and clamp at both ends."""
import numpy as np

from baler_amd import latent8
from baler_amd.modules import models
from oracle import c_oracle as orc

BAND = 5e-3             # codes are compared with q8(oracle) outside this distance from a half-integer: 2 x the fp32 bar (1e-5) x 255
BAND_SHARE = 0.03       # at most this share of the elements may fall inside the band (about 1 % for spread-out fractional parts)


def value_set():
    """float32 values for every branch of the store rule: NaN, +-inf, +-0, ties at k + 0.5 of both parities, values just off ties,
    the clamp edges (-0.5, 254.5, 255.5), large magnitudes, float32 subnormals and random bit patterns."""
    f = lambda bits: np.array(bits, dtype=np.uint32).view(np.float32)      # noqa: E731
    special = f([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001,
                 0x7F7FFFFF, 0xFF7FFFFF, 0x4F000000, 0xCF000000])
    ties = np.arange(-3, 260, dtype=np.float32) + np.float32(0.5)           # -2.5 ... 259.5: both parities, -0.5, 254.5, 255.5
    off = np.concatenate([np.nextafter(ties, np.float32(np.inf)), np.nextafter(ties, np.float32(-np.inf))])
    ints = np.arange(-3, 260, dtype=np.float32)
    big = np.array([1e3, -1e3, 65504, 1e10, -1e10, 3e38, -3e38, 255.49, 255.51, 256, 1e-30, -1e-30], dtype=np.float32)
    rng = np.random.default_rng(8)
    rand = rng.integers(0, 2**32, size=20000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    spread = rng.uniform(-20, 280, size=20000).astype(np.float32)
    return np.concatenate([special, ties, off, ints, big, rand, spread])


def q8_scalar(v):
    """The store rule element by element in Python arithmetic (round() is half-to-even), independent of latent8.q8."""
    out = np.empty(len(v), dtype=np.uint8)
    for i, x in enumerate(np.asarray(v, dtype=np.float32)):
        x = float(x)
        if x != x or x <= 0:
            out[i] = 0
        elif x >= 255:
            out[i] = 255
        else:
            out[i] = round(x)
    return out


# (name, dims, seed of formula_params, seed of the rows)
DENSE = {
    "ae24-15": (orc.ae_dims(24, 15), 99, 5),
    "ae24-2": (orc.ae_dims(24, 2), 98, 6),
    "ae40-10": (orc.ae_dims(40, 10), 97, 7),
    "ae100-10": (orc.ae_dims(100, 10), 96, 8),
    "ae100-40": (orc.ae_dims(100, 40), 95, 9),
    "ae130-9": (orc.ae_dims(130, 9), 94, 10),
    "cfd625-7": (orc.ae_dims(625, 7), 93, 11),
    "cfd2500-25": (orc.ae_dims(2500, 25), 92, 12),
    "layerwise-400-9": ([400, 120, 60, 30, 9, 30, 60, 120, 400], 91, 13),
    "fpga24-15": (models.fpga_dims(24, 15), 90, 14),
}
ROWS_MAX = 4100
N_CAL = {"cfd2500-25": 33}      # rows the scale is calibrated on (default 257); the widest model runs 33 rows


def rows(name, n=ROWS_MAX):
    """The first n of the case's 4100 rows (float64 in [0, 1)): every row count of a case shares them."""
    dims, _, seed = DENSE[name]
    return np.random.default_rng(seed).random((ROWS_MAX, dims[0]))[:n]


def layout(dims):
    return models.tensor_layout(dims)[0]


def clamping_scale(z):
    """[lo ; rng] from the 3rd and 97th percentile of every latent column: the codes span 0..255 and about 3 % of the rows clamp at
    either end."""
    lo, hi = np.percentile(z, 3, axis=0), np.percentile(z, 97, axis=0)
    return lo, hi - lo


_cache = {}


def folded_case(name):
    """-> (dims, flat, folded flat (float64, unrounded), lo, rng): formula parameters, the scale calibrated on the oracle's latent of
    the case's first N_CAL rows."""
    if name not in _cache:
        dims, pseed, _ = DENSE[name]
        flat = orc.formula_params(dims, pseed)
        lo, rng = clamping_scale(orc.encode(dims, flat, rows(name, N_CAL.get(name, 257))))
        _cache[name] = (dims, flat, latent8.fold_flat(flat, layout(dims), lo, rng), lo, rng)
    return _cache[name]


def band_share(c):
    """Share of the values whose distance from a half-integer is at most BAND (clamped values are far from the comparison: a value
    below -0.5 - BAND or above 255.5 + BAND gives 0 or 255 whatever its fraction)."""
    c = np.asarray(c, dtype=np.float64)
    near = np.abs(c - np.floor(c) - 0.5) <= BAND
    return float((near & (c > -0.5 - BAND) & (c < 255.5 + BAND)).mean()), near | ~np.isfinite(c)
