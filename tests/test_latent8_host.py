"""8-bit latent codes, host side (no GPU): the store / load rule in NumPy, the fold of the per-column scale into the model against
the fp64 oracle, config.latent_dtype = "uint8" parsing, the compressed.npz format with its refusals, and the header."""
import os
import re
import types

import numpy as np
import pytest
import torch

import latent8_cases as lc
import pjconv_ref
from baler_amd import hostio, latent8, native
from baler_amd.modules import helper, models
from oracle import c_oracle as orc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rel = pjconv_ref.rel        # max(rel-L2, max-norm): the suite's parity measure
FP64_BAR = 1e-11


def test_q8_is_the_store_rule():
    v = lc.value_set()
    q = latent8.q8(v)
    assert q.dtype == np.uint8 and q.shape == v.shape
    np.testing.assert_array_equal(q, lc.q8_scalar(v))
    one = lambda x: int(latent8.q8(np.array([x], dtype=np.float32))[0])      # noqa: E731
    assert [one(x) for x in (np.nan, -np.inf, np.inf, -0.0, 0.0, -0.5, 0.5, 1.5, 2.5, 253.5, 254.5, 255.5, 1e30, -1e30)] == \
        [0, 0, 255, 0, 0, 0, 0, 2, 2, 254, 254, 255, 255, 0]
    assert one(np.nextafter(np.float32(0.5), np.float32(1))) == 1 and one(np.nextafter(np.float32(254.5), np.float32(255))) == 255
    # a float64 value is rounded to float32 FIRST (an fp64 handle's rule): 0.5 + 2^-40 is 0.5 in float32 and ties to 0
    assert int(latent8.q8(np.array([0.5 + 2.0 ** -40]))[0]) == 0
    # the load rule: exact, and q8 is its left inverse
    w = latent8.widen8(np.arange(256, dtype=np.uint8))
    assert w.dtype == np.float32
    np.testing.assert_array_equal(w, np.arange(256, dtype=np.float32))
    np.testing.assert_array_equal(latent8.q8(w), np.arange(256, dtype=np.uint8))
    with pytest.raises(ValueError):
        latent8.widen8(np.zeros(3, dtype=np.int8))


@pytest.mark.parametrize("name", ["ae24-15", "ae40-10", "cfd625-7", "fpga24-15"])
def test_fold_against_the_oracle(name):
    dims, flat, folded, lo, rng = lc.folded_case(name)
    x = lc.rows(name, 513)
    s = latent8.scale_of(rng)
    assert (rng > 0).all() and np.allclose(s * rng, 255.0)
    z = orc.encode(dims, flat, x)
    got = orc.encode(dims, folded, x)
    want = (z - lo) * s
    print(f"{name}: encode_folded vs (encode - lo) * s: {rel(got, want):.2e}; codes in [{want.min():.1f}, {want.max():.1f}]")
    assert rel(got, want) < FP64_BAR
    c = np.random.default_rng(3).uniform(0, 255, size=(513, len(lo)))
    assert rel(orc.decode(dims, folded, c), orc.decode(dims, flat, c / s + lo)) < FP64_BAR
    # everything but the four tensors is untouched, and the input vector is not modified
    (we, be), (wd, bd) = latent8.latent_tensors(lc.layout(dims))
    same = np.ones(len(flat), dtype=bool)
    for key, off, shape in (we, be, wd, bd):
        same[off:off + int(np.prod(shape))] = False
    np.testing.assert_array_equal(folded[same], flat[same])
    np.testing.assert_array_equal(flat, orc.formula_params(dims, lc.DENSE[name][1]))
    mid = (len(dims) - 1) // 2
    assert we[2] == (dims[mid], dims[mid - 1]) and wd[2] == (dims[mid + 1], dims[mid])


def test_fold_with_a_constant_column():
    """rng = 0 in one column: s = 1 there, the code is z - lo = 0 and decodes to lo."""
    dims, flat, _, lo, rng = lc.folded_case("ae24-15")
    rng = rng.copy()
    rng[4] = 0.0
    s = latent8.scale_of(rng)
    assert s[4] == 1.0
    folded = latent8.fold_flat(flat, lc.layout(dims), lo, rng)
    x = lc.rows("ae24-15", 200)
    assert rel(orc.encode(dims, folded, x), (orc.encode(dims, flat, x) - lo) * s) < FP64_BAR
    c = np.random.default_rng(4).uniform(0, 255, size=(200, 15))
    c[:, 4] = 0.0
    assert rel(orc.decode(dims, folded, c), orc.decode(dims, flat, c / s + lo)) < FP64_BAR
    with pytest.raises(ValueError):
        latent8.fold_flat(flat, lc.layout(dims), lo[:-1], rng[:-1])


def test_fold_pj_conv_ae():
    z = 10
    torch.manual_seed(4)
    flat = models.pj_conv_init(z).numpy().astype(np.float64)
    x = np.random.default_rng(1).random((64, 784))
    zz = pjconv_ref.encode(z, flat, x)
    lo, rng = lc.clamping_scale(zz)
    s = latent8.scale_of(rng)
    folded = latent8.fold_flat(flat, models.pj_conv_layout(z)[0], lo, rng)
    assert rel(pjconv_ref.encode(z, folded, x), (zz - lo) * s) < FP64_BAR
    c = np.random.default_rng(2).uniform(0, 255, size=(64, z))
    assert rel(pjconv_ref.decode(z, folded, c), pjconv_ref.decode(z, flat, c / s + lo)) < FP64_BAR
    (we, be), (wd, bd) = latent8.latent_tensors(models.pj_conv_layout(z)[0])
    assert (we[0], be[0], wd[0], bd[0]) == ("encoder.5.weight", "encoder.5.bias", "decoder.0.weight", "decoder.0.bias")


@pytest.mark.parametrize("mode,dtype", [("fp32", np.float32), ("fp64", np.float64)])
def test_fold_of_a_model_returns_a_rounded_copy(mode, dtype):
    """fold(model, ...) evaluates in float64, rounds once to the model's parameter type and leaves the model as it was."""
    m = models.AE(24, 15, mode=mode)
    dims, flat, _, lo, rng = lc.folded_case("ae24-15")
    m.load_flat(flat)
    before = m.flat.clone()
    got = latent8.fold(m, lo, rng)
    assert got.dtype == dtype and got.shape == (m.nparams,)
    assert torch.equal(m.flat, before)
    want = latent8.fold_flat(m.flat[:m.nparams].numpy(), m.layout, lo, rng).astype(dtype)
    np.testing.assert_array_equal(got, want)
    pj = models.PJ_Conv_AE(784, 10, mode="fp32")
    assert latent8.fold(pj, np.zeros(10), np.ones(10)).shape == (pj.nparams,)


@pytest.mark.parametrize("name", sorted(lc.DENSE))
def test_band_share_of_the_committed_seeds(name):
    """tests/test_gpu_latent8.py compares codes with q8(oracle) outside a band of 5e-3 around the half-integers; for the seeds
    committed in latent8_cases.py at most 3 % of the oracle's folded latents lie inside it (the oracle alone, on the CPU)."""
    n = 33 if name == "cfd2500-25" else 4100       # the rows the GPU test runs
    dims, flat, folded, lo, rng = lc.folded_case(name)
    share, _ = lc.band_share(orc.encode(dims, folded, lc.rows(name, n)))
    print(f"{name}: {100 * share:.2f} % of the folded oracle latents within {lc.BAND} of a half-integer")
    assert share <= lc.BAND_SHARE


def test_latent_dtype_parsing_and_refusals_without_a_device(monkeypatch):
    def no_gpu():
        raise AssertionError("latent_dtype must be checked before any GPU work")
    monkeypatch.setattr(native, "require_gpu", no_gpu)
    assert helper.latent_dtype_of(types.SimpleNamespace(latent_dtype="uint8")) == "uint8"
    assert hostio.parse_latent_dtype("uint8") == "uint8" and hostio.LATENT_DTYPES["uint8"] == torch.uint8
    for bad in ("int8", "float32", "fp16", "half", "Float16", "", "u8", "UINT8", 8, torch.uint8, np.uint8):
        with pytest.raises(ValueError, match="latent_dtype"):
            helper.latent_dtype_of(types.SimpleNamespace(latent_dtype=bad))
    # the binding: 8 is a latent code only
    assert native.U8 == 8 and native._dt_latent(torch.empty(1, dtype=torch.uint8)) == native.U8
    with pytest.raises(native.NativeError):
        native._dt(torch.empty(1, dtype=torch.uint8))
    for dt in (torch.int8, torch.int16, torch.int32):
        with pytest.raises(native.NativeError):
            native._dt_latent(torch.empty(1, dtype=dt))


def _archive(tmp_path, **members):
    path = tmp_path / "compressed.npz"
    np.savez(path, names=np.array(["a", "b"]), normalization_features=np.zeros((2, 2)), **members)
    loaded = np.load(path)
    return hostio.open_npz_array(path, "data"), loaded.files, lambda k: loaded[k]


def test_uint8_archive_round_trip(tmp_path):
    n, z = 1000, 15
    codes = np.random.default_rng(5).integers(0, 256, size=(n, z), dtype=np.uint8)
    scale = np.stack([np.linspace(-3, 2, z), np.linspace(0.0, 7, z)])      # (a zero range is legal: a constant column)
    fields = hostio.latent_to_archive(codes, "uint8", scale=scale)
    assert sorted(fields) == ["data", "latent_dtype", "latent_scale"] and fields["data"] is codes
    data, keys, read = _archive(tmp_path, **fields)
    assert sorted(keys) == ["data", "latent_dtype", "latent_scale", "names", "normalization_features"]
    assert data.dtype == np.uint8 and data.shape == (n, z) and data.nbytes == n * z
    assert str(read("latent_dtype")) == "uint8"
    assert read("latent_scale").dtype == np.float64 and read("latent_scale").shape == (2, z)
    carrier, code_dtype = hostio.latent_from_archive(data, keys, read)
    assert code_dtype == torch.uint8 and carrier.dtype == np.uint8 and carrier.shape == (n, z)
    np.testing.assert_array_equal(hostio.latent_scale_from_archive(data, keys, read), scale)
    # upload / download move the bytes verbatim (CPU tensors take the same gather)
    t = hostio.upload_rows(carrier, device="cpu", keep_half=True)
    assert t.dtype == torch.uint8
    np.testing.assert_array_equal(t.numpy(), codes)
    np.testing.assert_array_equal(hostio.download_rows(t), codes)
    part = hostio.upload_rows(carrier, hostio.RowPlan.contiguous(n, 1, 3), device="cpu", keep_half=True)
    np.testing.assert_array_equal(part.numpy(), codes[334:667])
    # a uint8 TABLE (not codes) still takes the float64 route of every non-float32 table
    assert hostio.upload_rows(codes, device="cpu").dtype == torch.float64
    # every other archive has no scale, and the present calls keep their shapes
    assert hostio.latent_scale_from_archive(codes.astype(np.float32), ["data"], read) is None
    assert list(hostio.latent_to_archive(codes.astype(np.float32), None)) == ["data"]


def test_malformed_uint8_archives_are_refused(tmp_path, monkeypatch):
    def no_gpu():
        raise AssertionError("the archive must be refused before any GPU work")
    monkeypatch.setattr(native, "require_gpu", no_gpu)
    monkeypatch.setattr(hostio, "upload_rows", lambda *a, **k: no_gpu())
    n, z = 50, 15
    codes = np.random.default_rng(6).integers(0, 256, size=(n, z), dtype=np.uint8)
    good = np.stack([np.zeros(z), np.ones(z)])
    key = np.array("uint8")
    nan, inf, neg = good.copy(), good.copy(), good.copy()
    nan[0, 3], inf[1, 2], neg[1, 5] = np.nan, np.inf, -1e-9
    bad_archives = {
        "no scale": dict(data=codes, latent_dtype=key),
        "scale of the wrong shape": dict(data=codes, latent_dtype=key, latent_scale=good[:, :-1]),
        "transposed scale": dict(data=codes, latent_dtype=key, latent_scale=good.T),
        "flat scale": dict(data=codes, latent_dtype=key, latent_scale=good.reshape(-1)),
        "integer scale": dict(data=codes, latent_dtype=key, latent_scale=good.astype(np.int64)),
        "NaN entry": dict(data=codes, latent_dtype=key, latent_scale=nan),
        "inf entry": dict(data=codes, latent_dtype=key, latent_scale=inf),
        "negative range": dict(data=codes, latent_dtype=key, latent_scale=neg),
        "data not uint8": dict(data=codes.astype(np.int8), latent_dtype=key, latent_scale=good),
        "float16 data": dict(data=codes.astype(np.float16), latent_dtype=key, latent_scale=good),
        "uint16 data": dict(data=codes.astype(np.uint16), latent_dtype=key, latent_scale=good),
    }
    for what, members in bad_archives.items():
        sub = tmp_path / what.replace(" ", "_")
        sub.mkdir()
        data, keys, read = _archive(sub, **members)
        with pytest.raises(ValueError):
            hostio.latent_from_archive(data, keys, read)
        with pytest.raises(ValueError):
            hostio.latent_scale_from_archive(data, keys, read)
        # helper.decompress refuses it on the archive alone: no model is loaded, no device is asked for
        with pytest.raises(ValueError):
            helper.decompress("/nonexistent/model.pt", str(sub / "compressed.npz"), None, None, "AE", types.SimpleNamespace(), None, None)
    # the writer refuses the same things
    for scale in (None, good[:, :-1], nan, inf, neg):
        with pytest.raises(ValueError):
            hostio.latent_to_archive(codes, "uint8", scale=scale)
    with pytest.raises(ValueError):
        hostio.latent_to_archive(codes.astype(np.float32), "uint8", scale=good)
    with pytest.raises(ValueError):
        hostio.latent_to_archive(codes.astype(np.float16), "float16", scale=good)      # a scale belongs to uint8 codes only


def test_header_and_binding():
    header = open(os.path.join(REPO, "include", "baler_amd.h")).read()
    assert re.search(r"typedef enum bamd_code8 \{\s*BAMD_U8 = 8\s*\} bamd_code8;", header)
    m = re.search(r"typedef enum bamd_dtype \{([^}]*)\} bamd_dtype;", header)
    assert [e.strip() for e in m.group(1).split(",")] == ["BAMD_F32 = 0", "BAMD_F64 = 1", "BAMD_F16 = 2", "BAMD_BF16 = 3"]
    assert len(native.SYMBOLS) == 38 and len(set(native.SYMBOLS)) == 38
    assert set(re.findall(r"\b(bamd_[a-z_0-9]+)\s*\(", header)) == set(native.SYMBOLS)
    assert "#define BAMD_ABI_VERSION 1\n" in header
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "38 exported functions" in readme and "uint8" in readme
