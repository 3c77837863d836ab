"""16-bit latent codes, host side (no GPU): the ABI enum and the binding's dtype codes, config.latent_dtype parsing, and the
compressed.npz format for float16 / bfloat16 codes next to archives written before the key existed."""
import os
import re
import types

import numpy as np
import pytest
import torch

from baler_amd import hostio, native
from baler_amd.modules import helper

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_enum_and_binding_codes():
    header = open(os.path.join(REPO, "include", "baler_amd.h")).read()
    m = re.search(r"typedef enum bamd_dtype \{([^}]*)\} bamd_dtype;", header)
    assert m, "bamd_dtype enum not found"
    entries = [e.strip() for e in m.group(1).split(",")]
    assert entries == ["BAMD_F32 = 0", "BAMD_F64 = 1", "BAMD_F16 = 2", "BAMD_BF16 = 3"]
    assert (native.F32, native.F64, native.F16, native.BF16) == (0, 1, 2, 3)
    # the feature enters through bamd_encode / bamd_decode: no new export, ABI version unchanged
    assert len(native.SYMBOLS) == 38 and len(set(native.SYMBOLS)) == 38
    assert "#define BAMD_ABI_VERSION 1\n" in header
    # 16-bit tensors are latent codes only: every other tensor argument of the binding refuses them on the host
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(native.NativeError):
            native._dt(torch.empty(1, dtype=dt))
    assert native._dt_latent(torch.empty(1, dtype=torch.float16)) == native.F16
    assert native._dt_latent(torch.empty(1, dtype=torch.bfloat16)) == native.BF16
    assert native._dt_latent(torch.empty(1, dtype=torch.float32)) == native.F32
    assert native._dt_latent(torch.empty(1, dtype=torch.float64)) == native.F64


def test_latent_dtype_parsing(monkeypatch):
    def no_gpu():
        raise AssertionError("latent_dtype must be checked before any GPU work")
    monkeypatch.setattr(native, "require_gpu", no_gpu)
    assert helper.latent_dtype_of(types.SimpleNamespace()) is None
    assert helper.latent_dtype_of(types.SimpleNamespace(latent_dtype=None)) is None
    assert helper.latent_dtype_of(types.SimpleNamespace(latent_dtype="float16")) == "float16"
    assert helper.latent_dtype_of(types.SimpleNamespace(latent_dtype="bfloat16")) == "bfloat16"
    for bad in ("float32", "fp16", "half", "Float16", "", 16, torch.float16, np.float16):
        with pytest.raises(ValueError, match="latent_dtype"):
            helper.latent_dtype_of(types.SimpleNamespace(latent_dtype=bad))
    # the compress entry points fail on the value alone: no table is opened, no device is asked for
    cfg = types.SimpleNamespace(latent_dtype="int8", input_path="/nonexistent/table.npz", save_error_bounded_deltas=False)
    with pytest.raises(ValueError, match="latent_dtype"):
        helper.compress("/nonexistent/model.pt", cfg)
    from baler_amd import baler
    cfg.model_name, cfg.model_type = "AE", "dense"
    with pytest.raises(ValueError, match="latent_dtype"):
        baler.perform_compression("/nonexistent/output", cfg, False)


def _value_set():
    """float32 values that exercise every branch of a round-to-nearest-even narrowing: NaN, +-inf, +-0, float32 and bfloat16
    subnormals, ties (to even, both directions), just off ties, the largest finite values (rounding up to inf) and random bits."""
    f = lambda bits: np.array(bits, dtype=np.uint32).view(np.float32)      # noqa: E731
    special = f([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000,
                 0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x00010000, 0x007FFFFF, 0x00800000,
                 0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x3F817FFF, 0x3F818001,      # ties at 1.0: to even down / up, off ties
                 0xBF808000, 0xBF818000,
                 0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0xFF7FFFFF,                               # rounds up to +-inf / stays finite
                 0x477FE000, 0x477FF000, 0x33800000, 0x387FC000])
    rng = np.random.default_rng(16)
    rand = rng.integers(0, 2**32, size=20000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return np.concatenate([special, rand])


def test_bfloat16_archive_round_trip_matches_torch(tmp_path):
    v = _value_set()
    bits = hostio.bf16_bits(v)
    want = torch.from_numpy(v).to(torch.bfloat16)
    want_bits = want.view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(v)
    assert nan.sum() >= 3
    # every non-NaN value: the very bit pattern torch.bfloat16 holds (round to nearest even, subnormals kept, overflow -> inf)
    np.testing.assert_array_equal(bits[~nan], want_bits[~nan])
    # NaN stays NaN (torch's own conversions do not agree on one payload: its vectorised CPU path and its scalar path differ)
    assert np.isnan(hostio.bf16_widen(bits[nan])).all() and torch.isnan(want[torch.from_numpy(nan)]).all()
    assert (bits[nan] == 0x7FC0).all()
    np.testing.assert_array_equal(hostio.bf16_widen(bits[~nan]).view(np.uint32), want.float().numpy()[~nan].view(np.uint32))

    codes = np.ascontiguousarray(bits[:15000].reshape(-1, 15))      # (the special values lead)
    path = tmp_path / "compressed.npz"
    names = np.array(["a", "b"])
    np.savez(path, names=names, normalization_features=np.zeros((2, 2)), **hostio.latent_to_archive(codes, "bfloat16"))
    loaded = np.load(path)
    assert sorted(loaded.files) == ["data", "latent_dtype", "names", "normalization_features"]
    assert loaded["data"].dtype == np.uint16 and str(loaded["latent_dtype"]) == "bfloat16"
    assert loaded["data"].nbytes == codes.shape[0] * codes.shape[1] * 2
    data = hostio.open_npz_array(path, "data")
    carrier, code_dtype = hostio.latent_from_archive(data, loaded.files, lambda k: loaded[k])
    assert code_dtype == torch.bfloat16 and carrier.dtype == np.float16 and carrier.shape == codes.shape
    # the upload path (CPU tensors take the same gather): the float16-typed carrier moves the bit patterns verbatim, NaNs included
    t = hostio.upload_rows(carrier, device="cpu", keep_half=True)
    assert t.dtype == torch.float16
    back = t.view(torch.bfloat16)
    np.testing.assert_array_equal(back.view(torch.int16).numpy().view(np.uint16), codes)
    # ... and the download side's view back
    np.testing.assert_array_equal(hostio.download_rows(back.view(torch.float16)).view(np.uint16), codes)


def test_float16_archive_round_trip(tmp_path):
    v = _value_set()
    with np.errstate(over="ignore"):
        codes = v.astype(np.float16)[:15000].reshape(-1, 15)
    path = tmp_path / "compressed.npz"
    np.savez(path, names=np.array(["a"]), normalization_features=np.zeros((2, 1)), **hostio.latent_to_archive(codes, "float16"))
    loaded = np.load(path)
    assert sorted(loaded.files) == ["data", "names", "normalization_features"]       # float16 needs no key: data.dtype says it
    assert loaded["data"].dtype == np.float16 and loaded["data"].nbytes == codes.size * 2
    carrier, code_dtype = hostio.latent_from_archive(hostio.open_npz_array(path, "data"), loaded.files, lambda k: loaded[k])
    assert code_dtype == torch.float16
    t = hostio.upload_rows(carrier, device="cpu", keep_half=True)
    assert t.dtype == torch.float16
    np.testing.assert_array_equal(t.view(torch.int16).numpy(), codes.view(np.int16))
    with pytest.raises(ValueError):
        hostio.latent_to_archive(codes.astype(np.float32), "float16")
    with pytest.raises(ValueError):
        hostio.latent_to_archive(codes, "bfloat16")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_archives_without_the_key_load_as_before(tmp_path, dtype):
    codes = np.random.default_rng(2).normal(size=(300, 15)).astype(dtype)
    path = tmp_path / "compressed.npz"
    fields = hostio.latent_to_archive(codes, None)
    assert list(fields) == ["data"] and fields["data"] is codes         # the default writes exactly what it always wrote
    np.savez(path, data=codes, names=np.array(["a"]), normalization_features=np.zeros((2, 1)))
    loaded = np.load(path)
    data = hostio.open_npz_array(path, "data")
    carrier, code_dtype = hostio.latent_from_archive(data, loaded.files, lambda k: loaded[k])
    assert code_dtype is None and carrier is data and carrier.dtype == dtype
    t = hostio.upload_rows(carrier, device="cpu")
    assert t.dtype == (torch.float32 if dtype == np.float32 else torch.float64)
    np.testing.assert_array_equal(t.numpy(), codes)
    # a float16 TABLE (not codes) still takes the float64 route of every non-float32 table
    assert hostio.upload_rows(codes.astype(np.float16), device="cpu").dtype == torch.float64
    # an unknown key value is refused rather than guessed at
    with pytest.raises(ValueError):
        hostio.latent_from_archive(codes.astype(np.float16).view(np.uint16), ["data", "latent_dtype"], lambda k: np.array("float8"))
