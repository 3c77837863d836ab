"""The fp16x3 inference mode (BAMD_MODE_F16X3) on the host: the ABI constants, the mode names, and what the NumPy emulation of the
contract (tests/f16x3_ref.py) says about its accuracy: fp32's, from binary16 products."""
import os
import re

import numpy as np
import pytest

import f16x3_ref as ref
from baler_amd import native, synth
from baler_amd.modules import models
from oracle import c_oracle as orc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL32 = 1e-5      # the project's fp32 parity bar


def test_header_declares_the_mode_and_the_path():
    header = open(os.path.join(REPO, "include", "baler_amd.h")).read()
    assert re.search(r"\bBAMD_MODE_F16X3\s*=\s*5\b", header)
    assert re.search(r"\bBAMD_PATH_F16X3\s*=\s*5\b", header)
    assert re.search(r"\bBAMD_MODE_F16\s*=\s*3\b", header) and re.search(r"\bBAMD_PATH_F16\s*=\s*4\b", header)
    assert not re.search(r"\bBAMD_MODE_\w+\s*=\s*4\b", header)      # 4 stays the "unknown mode" probe of tests/test_gpu_f16.py
    assert "BAMD_ABI_VERSION 1" in header


def test_mode_names_and_binding_constants():
    assert native.MODE_F16X3 == 5 and native.MODE_NAMES["fp16x3"] == 5 and native.MODE_NAMES["f16x3"] == 5
    assert native.MODE_NAMES["fp16"] == 3 and native.MODE_NAMES["bf16"] == 2 and native.MODE_NAMES["fp32"] == 0 and native.MODE_NAMES["fp64"] == 1
    assert 4 not in native.MODE_NAMES.values()
    assert native.PATH_NAMES[5] == "f16x3" and native.PATH_NAMES[4] == "f16"
    assert len(native.SYMBOLS) == 38                                 # a mode, not an entry point


def test_set_default_mode_accepts_fp16x3():
    before = models._DEFAULT_MODE
    try:
        models.set_default_mode("fp16x3")
        assert models._DEFAULT_MODE == "fp16x3"
        m = models.AE(24, 15)
        assert m.mode == "fp16x3" and m.flat.element_size() == 4      # float32 master parameters
        with pytest.raises(ValueError):
            models.set_default_mode("fp16x2")
    finally:
        models.set_default_mode(before)


def test_split():
    a = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -12, np.pi, -1e-3, 3e-6, 65504.0, 0.0], dtype=np.float32)
    hi, lo = ref.split(a)
    assert np.array_equal(hi, a.astype(np.float16).astype(np.float32))
    # hi + lo / 2^11 gives a back to 22 bits (exactly where a has no more)
    back = hi.astype(np.float64) + lo.astype(np.float64) / 2048
    normal = np.abs(a) >= 2.0 ** -14
    assert np.all(np.abs(back - a)[normal] <= 2.0 ** -22 * np.abs(a)[normal])
    assert np.all(np.abs(back - a)[~normal] <= 2.0 ** -36)      # below binary16's normal range: lo is a subnormal, 2^-24 / 2^11 apart
    assert back[1] == a[1] and back[2] == a[2] and lo[0] == 0 and lo[6] == 0
    # the scale keeps lo a NORMAL binary16 wherever hi is one: unscaled, the low part of 1e-3 is a binary16 subnormal
    assert abs(lo[4]) >= 2.0 ** -14 and abs(ref.split(a, 1.0)[1][4]) < 2.0 ** -14
    # beyond the range: hi is +-inf, lo is not finite, and so is everything computed from them
    hi, lo = ref.split(np.array([1e5, -7e4], dtype=np.float32))
    assert np.isposinf(hi[0]) and np.isneginf(hi[1]) and not np.isfinite(lo).any()


def c1_model():
    """The trained C1 fixture: AE(24, 15), float32 final parameters."""
    flat = np.load(os.path.join(REPO, "tests", "golden", "g7_c1_model_f32.npz"))["final_params_f32"].astype(np.float64)
    return orc.ae_dims(24, 15), flat


def model_and_rows(z, seed):
    if z == "c1":
        dims, flat = c1_model()
        return dims, flat, orc.normalize(synth.cms_rows(4096))
    dims = orc.ae_dims(24, z)
    return dims, orc.formula_params(dims, seed), np.random.default_rng(7).random((4096, 24))


def three(chain, dims, flat, x, zo, measure):
    """(encode, decode of the oracle's codes, forward) errors of an emulation against the fp64 oracle."""
    ro = orc.decode(dims, flat, zo)
    return (measure(chain(dims, flat, x, 0, 4), zo), measure(chain(dims, flat, zo, 4, 8), ro), measure(chain(dims, flat, x, 0, 8), ro))


CASES = [pytest.param("c1", 0, id="trained-c1")] + [pytest.param(z, s, id=f"formula-z{z}-seed{s}") for z in (15, 2) for s in (1, 23)]


@pytest.mark.parametrize("z,seed", CASES)
def test_emulated_error_is_fp32s(z, seed):
    """Against the fp64 oracle on 4,096 rows: the split chain meets the fp32 bar by the project's measure, its rel-L2 error is at
    most 1.5 x the float32 NumPy chain's (measured: 1.02 - 1.11 x; 1.5 is the project's allowance for accumulation-order variation),
    and the same chain WITHOUT the two correction products does not come near."""
    dims, flat, x = model_and_rows(z, seed)
    zo = orc.encode(dims, flat, x)
    e3 = three(ref.chain, dims, flat, x, zo, ref.rel_l2)
    e3m = three(ref.chain, dims, flat, x, zo, ref.rel)
    e32 = three(ref.fp32_chain, dims, flat, x, zo, ref.rel_l2)
    e1 = three(lambda *a: ref.chain(*a, products=1), dims, flat, x, zo, ref.rel_l2)
    e4 = three(lambda *a: ref.chain(*a, products=4), dims, flat, x, zo, ref.rel_l2)
    eu = three(lambda *a: ref.chain(*a, scale=1.0), dims, flat, x, zo, ref.rel_l2)
    e64 = three(lambda *a: ref.chain(*a, acc=np.float64), dims, flat, x, zo, ref.rel_l2)
    for i, what in enumerate(("encode", "decode", "forward")):
        print(f"{what}: split {e3[i]:.3e} (rel() {e3m[i]:.3e})  fp32 {e32[i]:.3e}  ratio {e3[i] / e32[i]:.2f};  one product {e1[i]:.3e}  "
              f"four {e4[i]:.3e}  unscaled {eu[i]:.3e}  float64 sums {e64[i]:.3e}")
        assert e3m[i] < TOL32, what
        assert e3[i] <= 1.5 * e32[i], what
        assert e1[i] > 1.5 * e32[i] and e1[i] > 100 * e3[i], what      # binary16 operands alone: the shipped fp16 mode's error


def test_binary16_codes_have_no_low_part():
    """Codes that are exactly binary16 (what bamd_decode reads with z_dtype = BAMD_F16) split into (code, 0): decoding them is the same
    computation with and without the low part of the input, bit for bit."""
    dims, flat, x = model_and_rows(15, 1)
    z16 = orc.encode(dims, flat, x[:512]).astype(np.float16)
    hi, lo = ref.split(z16.astype(np.float32))
    assert np.array_equal(hi, z16.astype(np.float32)) and not lo.any()
    with_lo = ref.chain(dims, flat, z16.astype(np.float64), 4, 8)
    offs = ref.layer_offsets(dims)
    assert with_lo.dtype == np.float32 and len(offs) == 8
    # the same decode with the input's low part dropped by hand: layer de1 on hi alone, then the contract's chain
    N, K = dims[5], dims[4]
    flat32 = flat.astype(np.float32)
    w = flat32[offs[4]:offs[4] + N * K].reshape(N, K)
    b = flat32[offs[4] + N * K:offs[4] + N * K + N]
    wh, wl = ref.split(w)
    a = (hi @ wh.T + b).astype(np.float32) + (hi @ wl.T).astype(np.float32) * np.float32(1 / 2048)
    a = np.maximum(a, a * np.float32(0.01))
    assert np.array_equal(ref.chain(dims, flat, a, 5, 8), with_lo)
