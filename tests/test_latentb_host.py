"""Packed sub-byte latent codes, host side (no GPU): the bit layout (pack_rows / unpack_rows against np.packbits), the store rule qb,
the fold at levels = 2**b - 1 against the fp64 oracle, the band share of the cases the GPU tests use, config.latent_dtype =
"uint1" .. "uint7" parsing, the compressed.npz format with its refusals, and the header."""
import os
import re
import types

import numpy as np
import pytest
import torch

import latent8_cases as lc
import latentb_cases as lb
import pjconv_ref
from baler_amd import hostio, latent8, native
from baler_amd.modules import helper
from oracle import c_oracle as orc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rel = pjconv_ref.rel
FP64_BAR = 1e-11
Z_SET = (1, 2, 7, 8, 9, 15, 16, 17, 25, 63)
N_SET = (1, 3, 64)


@pytest.mark.parametrize("bits", lb.BITS)
def test_pack_rows_is_the_layout_rule(bits):
    rng = np.random.default_rng(100 + bits)
    for z in Z_SET:
        for n in N_SET:
            q = rng.integers(0, 2 ** bits, size=(n, z)).astype(np.uint8)
            q[0, :] = 2 ** bits - 1                      # every bit of a row set: the padding must still come out zero
            packed = latent8.pack_rows(q, bits)
            S = -(-z * bits // 8)
            assert packed.dtype == np.uint8 and packed.shape == (n, S) and packed.flags["C_CONTIGUOUS"], (z, n)
            assert S == latent8.row_bytes(z, bits) == hostio.packed_row_bytes(z, bits) == native.packed_row_bytes(z, bits)
            np.testing.assert_array_equal(packed, lb.packbits_rows(q, bits), err_msg=f"b={bits} z={z} n={n}")
            pad = 8 * S - z * bits
            assert 0 <= pad <= 7
            if pad:
                assert not (packed[:, -1] >> (8 - pad)).any(), f"b={bits} z={z}: padding bits are not zero"
            np.testing.assert_array_equal(latent8.unpack_rows(packed, z, bits), q)
            # padding bits are ignored on load
            dirty = packed.copy()
            if pad:
                dirty[:, -1] |= np.uint8((0xFF << (8 - pad)) & 0xFF)
            np.testing.assert_array_equal(latent8.unpack_rows(dirty, z, bits), q)
    # code k of a row occupies bits [k b, (k + 1) b): one code set, every other zero
    z = 17
    for k in range(z):
        q = np.zeros((1, z), dtype=np.uint8)
        q[0, k] = 2 ** bits - 1
        word = int.from_bytes(latent8.pack_rows(q, bits)[0].tobytes(), "little")
        assert word == (2 ** bits - 1) << (k * bits)
    with pytest.raises(ValueError):
        latent8.pack_rows(np.full((2, 3), 2 ** bits, dtype=np.uint8) if bits < 8 else np.zeros((2, 3)), bits)
    with pytest.raises(ValueError):
        latent8.unpack_rows(np.zeros((2, 5), dtype=np.uint8), 3, bits)      # 3 codes never take 5 bytes


def test_pack_rows_at_8_bits_is_the_identity():
    q = np.random.default_rng(1).integers(0, 256, size=(5, 9)).astype(np.uint8)
    np.testing.assert_array_equal(latent8.pack_rows(q, 8), q)
    np.testing.assert_array_equal(latent8.unpack_rows(q, 9, 8), q)


@pytest.mark.parametrize("bits", lb.BITS + (8,))
def test_qb_is_the_store_rule(bits):
    top = 2 ** bits - 1
    assert latent8.levels(bits) == top
    v = lb.value_set(bits)
    q = latent8.qb(v, bits)
    assert q.dtype == np.uint8 and q.shape == v.shape and q.max() == top
    np.testing.assert_array_equal(q, lb.qb_scalar(v, bits))
    one = lambda x: int(latent8.qb(np.array([x], dtype=np.float32), bits)[0])      # noqa: E731
    assert [one(x) for x in (np.nan, -np.inf, np.inf, -0.0, 0.0, -0.5, 0.5, -1.0, -1e9, 1e9, top + 0.5, top + 7.0)] == \
        [0, 0, top, 0, 0, 0, 0, 0, 0, top, top, top]
    for k in range(top):      # ties go to the even neighbour
        assert one(k + 0.5) == (k if k % 2 == 0 else k + 1)
        assert one(np.nextafter(np.float32(k + 0.5), np.float32(top + 1))) == k + 1
        assert one(np.nextafter(np.float32(k + 0.5), np.float32(-1))) == k
    # a float64 value is rounded to float32 FIRST: 0.5 + 2^-40 is 0.5 in float32 and ties to 0
    assert int(latent8.qb(np.array([0.5 + 2.0 ** -40]), bits)[0]) == 0
    np.testing.assert_array_equal(latent8.qb(np.arange(top + 1, dtype=np.float32), bits), np.arange(top + 1, dtype=np.uint8))


def test_qb_at_8_bits_is_q8():
    v = lc.value_set()
    np.testing.assert_array_equal(latent8.qb(v, 8), latent8.q8(v))
    for bad in (0, 9, -1):
        with pytest.raises(ValueError):
            latent8.levels(bad)


@pytest.mark.parametrize("bits", lb.BITS)
@pytest.mark.parametrize("name", ["ae24-15", "cfd625-7"])
def test_fold_at_levels_against_the_oracle(name, bits):
    """The oracle's folded latent is (z - lo) * levels / rng, and un-scaling it returns the unfolded oracle latent."""
    levels = latent8.levels(bits)
    dims, flat, lo, rng, z = lb.oracle_case(name)
    _, folded, _, _ = lb.folded_case(name, bits)
    s = latent8.scale_of(rng, levels)
    assert (rng > 0).all() and np.allclose(s * rng, float(levels))
    c = orc.encode(dims, folded, lb.rows(name))
    assert rel(c, (z - lo) * s) < FP64_BAR
    back = c / s + lo
    assert rel(back, z) < FP64_BAR
    # unscale() is that map on codes: exact on integer code values
    q = latent8.qb(c, bits)
    np.testing.assert_allclose(latent8.unscale(q, lo, rng, levels), q.astype(np.float64) / s + lo, rtol=0, atol=0)
    # decoding code units on the folded parameters is decoding the un-scaled latent on the plain ones
    codes = np.random.default_rng(3).uniform(0, levels, size=(64, len(lo)))
    assert rel(orc.decode(dims, folded, codes), orc.decode(dims, flat, codes / s + lo)) < FP64_BAR
    # the defaults are the 8-bit fold
    np.testing.assert_array_equal(latent8.fold_flat(flat, lc.layout(dims), lo, rng), latent8.fold_flat(flat, lc.layout(dims), lo, rng, 255))
    np.testing.assert_array_equal(latent8.scale_of(rng), latent8.scale_of(rng, 255))


@pytest.mark.parametrize("bits", lb.BITS)
@pytest.mark.parametrize("name", lb.ORACLE_CASES)
def test_band_share_of_the_committed_seeds(name, bits):
    """tests/test_gpu_latentb.py compares codes with qb(oracle) outside a band of 5e-3 around the half-integers (at ORACLE_BITS; every
    width is held to the share here): at most 3 % of the oracle's folded latents of the committed seeds lie inside it."""
    dims, folded, _, _ = lb.folded_case(name, bits)
    c = orc.encode(dims, folded, lb.rows(name))
    share, _ = lb.band_share(c, bits)
    print(f"{name} b={bits}: {100 * share:.2f} % of the folded oracle latents within {lb.BAND} of a half-integer")
    assert share <= lb.BAND_SHARE
    q = latent8.qb(c, bits)
    assert q.min() == 0 and q.max() == 2 ** bits - 1 and (c < 0).any() and (c > 2 ** bits - 1).any()      # the codes span the range, values lie beyond both ends


def test_latent_dtype_parsing_and_refusals_without_a_device(monkeypatch):
    def no_gpu():
        raise AssertionError("latent_dtype must be checked before any GPU work")
    monkeypatch.setattr(native, "require_gpu", no_gpu)
    for b in lb.BITS:
        name = f"uint{b}"
        assert helper.latent_dtype_of(types.SimpleNamespace(latent_dtype=name)) == name
        assert hostio.parse_latent_dtype(name) == name and hostio.LATENT_DTYPES[name] == torch.uint8
        assert hostio.latent_bits(name) == b
        assert native.UB(b) == 0x100 | b
    assert hostio.latent_bits("uint8") == 8 and hostio.parse_latent_dtype("uint8") == "uint8"
    for other in (None, "float16", "bfloat16", "uint0", "uint9", "uint16", 5):
        assert hostio.latent_bits(other) is None
    for bad in ("uint0", "uint9", "uint16", "Uint4", 4, "uint", "uint 4", "u4", "int4", 0x104):
        with pytest.raises(ValueError, match="latent_dtype"):
            helper.latent_dtype_of(types.SimpleNamespace(latent_dtype=bad))
    for bad in (0, 8, 9, -1, 1.0, "5", None, True):
        with pytest.raises(native.NativeError):
            native.UB(bad)
    # a uint8 tensor without code_bits is still one byte per code
    assert native.U8 == 8 and native._dt_latent(torch.empty(1, dtype=torch.uint8)) == native.U8


def _archive(tmp_path, **members):
    path = tmp_path / "compressed.npz"
    np.savez(path, names=np.array(["a", "b"]), normalization_features=np.zeros((2, 2)), **members)
    loaded = np.load(path)
    return hostio.open_npz_array(path, "data"), loaded.files, lambda k: loaded[k]


@pytest.mark.parametrize("bits", lb.BITS)
def test_packed_archive_round_trip(tmp_path, bits):
    n, z = 1000, 15
    S = -(-z * bits // 8)
    q = np.random.default_rng(bits).integers(0, 2 ** bits, size=(n, z)).astype(np.uint8)
    codes = latent8.pack_rows(q, bits)
    scale = np.stack([np.linspace(-3, 2, z), np.linspace(0.0, 7, z)])
    name = f"uint{bits}"
    fields = hostio.latent_to_archive(codes, name, scale=scale)
    assert sorted(fields) == ["data", "latent_dtype", "latent_scale"] and fields["data"] is codes
    data, keys, read = _archive(tmp_path, **fields)
    assert sorted(keys) == ["data", "latent_dtype", "latent_scale", "names", "normalization_features"]      # no new key
    assert data.dtype == np.uint8 and data.shape == (n, S) and data.nbytes == n * S
    assert str(read("latent_dtype")) == name
    assert read("latent_scale").dtype == np.float64 and read("latent_scale").shape == (2, z)
    carrier, code_dtype = hostio.latent_from_archive(data, keys, read)
    assert code_dtype == torch.uint8 and carrier.dtype == np.uint8 and carrier.shape == (n, S)
    got = hostio.latent_scale_from_archive(data, keys, read)
    np.testing.assert_array_equal(got, scale)
    assert got.shape[1] == z                                       # z comes from the scale
    # upload / download and a rank's row slice move packed rows verbatim: rows are byte-aligned
    t = hostio.upload_rows(carrier, device="cpu", keep_half=True)
    assert t.dtype == torch.uint8
    np.testing.assert_array_equal(latent8.unpack_rows(hostio.download_rows(t), z, bits), q)
    part = hostio.upload_rows(carrier, hostio.RowPlan.contiguous(n, 1, 3), device="cpu", keep_half=True)
    np.testing.assert_array_equal(latent8.unpack_rows(part.numpy(), z, bits), q[334:667])


def test_a_uint8_archive_is_what_it_was(tmp_path):
    n, z = 100, 15
    codes = np.random.default_rng(5).integers(0, 256, size=(n, z), dtype=np.uint8)
    scale = np.stack([np.linspace(-3, 2, z), np.linspace(0.0, 7, z)])
    fields = hostio.latent_to_archive(codes, "uint8", scale=scale)
    assert sorted(fields) == ["data", "latent_dtype", "latent_scale"] and fields["data"] is codes
    assert str(fields["latent_dtype"]) == "uint8" and fields["latent_dtype"].dtype == np.array("uint8").dtype
    data, keys, read = _archive(tmp_path, **fields)
    carrier, code_dtype = hostio.latent_from_archive(data, keys, read)
    assert code_dtype == torch.uint8 and carrier.shape == (n, z)
    np.testing.assert_array_equal(np.asarray(carrier), codes)
    np.testing.assert_array_equal(hostio.latent_scale_from_archive(data, keys, read), scale)
    with pytest.raises(ValueError):
        hostio.latent_to_archive(codes.astype(np.float16), "float16", scale=scale)


def test_malformed_packed_archives_are_refused(tmp_path, monkeypatch):
    def no_gpu():
        raise AssertionError("the archive must be refused before any GPU work")
    monkeypatch.setattr(native, "require_gpu", no_gpu)
    monkeypatch.setattr(hostio, "upload_rows", lambda *a, **k: no_gpu())
    monkeypatch.setattr(torch, "load", lambda *a, **k: no_gpu())      # ... and before any model is loaded
    n, z, bits = 50, 15, 5
    codes = latent8.pack_rows(np.random.default_rng(6).integers(0, 32, size=(n, z)).astype(np.uint8), bits)
    assert codes.shape == (n, 10)
    good = np.stack([np.zeros(z), np.ones(z)])
    key = np.array("uint5")
    nan, inf, neg = good.copy(), good.copy(), good.copy()
    nan[0, 3], inf[1, 2], neg[1, 5] = np.nan, np.inf, -1e-9
    bad_archives = {
        "no scale": dict(data=codes, latent_dtype=key),
        "transposed scale": dict(data=codes, latent_dtype=key, latent_scale=good.T),
        "flat scale": dict(data=codes, latent_dtype=key, latent_scale=good.reshape(-1)),
        "empty scale": dict(data=codes, latent_dtype=key, latent_scale=good[:, :0]),
        "integer scale": dict(data=codes, latent_dtype=key, latent_scale=good.astype(np.int64)),
        "NaN entry": dict(data=codes, latent_dtype=key, latent_scale=nan),
        "inf entry": dict(data=codes, latent_dtype=key, latent_scale=inf),
        "negative range": dict(data=codes, latent_dtype=key, latent_scale=neg),
        "one byte too few": dict(data=codes[:, :-1], latent_dtype=key, latent_scale=good),
        "one byte per code": dict(data=np.zeros((n, z), dtype=np.uint8), latent_dtype=key, latent_scale=good),
        "scale of another width": dict(data=codes, latent_dtype=key, latent_scale=good[:, :-2]),      # 13 codes of 5 bits: 9 bytes
        "data not uint8": dict(data=codes.astype(np.int8), latent_dtype=key, latent_scale=good),
        "uint16 data": dict(data=codes.astype(np.uint16), latent_dtype=key, latent_scale=good),
        "flat data": dict(data=codes.reshape(-1), latent_dtype=key, latent_scale=good),
        "uint0": dict(data=codes, latent_dtype=np.array("uint0"), latent_scale=good),
        "uint9": dict(data=codes, latent_dtype=np.array("uint9"), latent_scale=good),
    }
    for what, members in bad_archives.items():
        sub = tmp_path / what.replace(" ", "_")
        sub.mkdir()
        data, keys, read = _archive(sub, **members)
        with pytest.raises(ValueError):
            hostio.latent_from_archive(data, keys, read)
        if what not in ("uint0", "uint9"):      # (names that are no code type have no scale to ask for)
            with pytest.raises(ValueError):
                hostio.latent_scale_from_archive(data, keys, read)
        with pytest.raises(ValueError):
            helper.decompress("/nonexistent/model.pt", str(sub / "compressed.npz"), None, None, "AE", types.SimpleNamespace(), None, None)
    # the writer refuses the same things
    for scale in (None, good.T, nan, inf, neg, good[:, :-2]):
        with pytest.raises(ValueError):
            hostio.latent_to_archive(codes, "uint5", scale=scale)
    with pytest.raises(ValueError):
        hostio.latent_to_archive(codes.astype(np.uint16), "uint5", scale=good)
    with pytest.raises(ValueError):
        hostio.latent_to_archive(codes, "uint9", scale=good)


def test_header_and_binding():
    header = open(os.path.join(REPO, "include", "baler_amd.h")).read()
    m = re.search(r"typedef enum bamd_codeb \{([^}]*)\} bamd_codeb;", header)
    assert m, "the header declares no bamd_codeb"
    members = dict(e.strip().split(" = ") for e in m.group(1).split(","))
    assert {k: int(v, 0) for k, v in members.items()} == {f"BAMD_U{b}": 0x100 | b for b in lb.BITS}
    assert re.search(r"#define BAMD_UB\(bits\) \(0x100 \| \(bits\)\)", header)
    # what was pinned stays pinned
    assert re.search(r"typedef enum bamd_code8 \{\s*BAMD_U8 = 8\s*\} bamd_code8;", header)
    d = re.search(r"typedef enum bamd_dtype \{([^}]*)\} bamd_dtype;", header)
    assert [e.strip() for e in d.group(1).split(",")] == ["BAMD_F32 = 0", "BAMD_F64 = 1", "BAMD_F16 = 2", "BAMD_BF16 = 3"]
    assert len(native.SYMBOLS) == 38 and len(set(native.SYMBOLS)) == 38
    assert set(re.findall(r"\b(bamd_[a-z_0-9]+)\s*\(", header)) == set(native.SYMBOLS)
    assert "#define BAMD_ABI_VERSION 1\n" in header
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "38 exported functions" in readme and "uint1" in readme and "uint7" in readme
