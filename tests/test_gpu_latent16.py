"""16-bit latent codes on MI355X (bamd_encode / bamd_decode with z_dtype BAMD_F16 / BAMD_BF16).

Bitwise: for every kernel family encode(x, out_dtype=h16) is encode(x, out_dtype=float32).to(h16) and decode(z16) is
decode(z16.to(float32)), the fused un-normalise / int-mask epilogue included.  Oracle: the codes against oracle/c_oracle within the
half-ulp of the format plus the compute mode's existing bar.  Refusals: every other dtype argument returns BAMD_ERR_INVALID for the
two new codes and leaves its output buffer alone.

FPGA_prototype_model and PJ_Conv_AE have no restatement in oracle/c_oracle (LeakyReLU dense models only): their 16-bit codes are
checked bitwise against their own float32 codes, and those float32 codes against their references in tests/test_gpu_fpga.py
(fpga_ref.py, fixture g17) and tests/test_gpu_pjconv.py (pjconv_ref.py, fixture g19).  The bitwise identity carries the half-ulp bound
over only as long as those tests stand."""
import ctypes

import numpy as np
import pytest
import torch

import fpga_ref
from baler_amd import native, synth
from baler_amd.modules import models
from oracle import c_oracle as orc

pytestmark = pytest.mark.gpu

H16 = (torch.float16, torch.bfloat16)
# round to nearest even: half an ulp, relative, in the format's normal range (11 / 8 significand bits) -- derived, not tuned
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
# the existing bars of the compute modes (tests/test_gpu_parity.py, include/baler_amd.h: "a THROUGHPUT mode with its own 2e-2 bar")
TOL = {"fp32": 1e-5, "fp64": 1e-11, "bf16": 2e-2}
IN_DT = {"fp32": torch.float32, "fp64": torch.float64, "bf16": torch.float32}
ROWS = (1, 17, 513, 5000)


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(_bits(a), _bits(b)), f"{what}: {int((_bits(a) != _bits(b)).sum())} of {a.numel()} elements differ"


def _params(flat, mode):
    return torch.from_numpy(np.concatenate([flat, [0.0]])).to(torch.float64 if mode == "fp64" else torch.float32).cuda()


def ae_handle(F, Z, mode, seed=99, flat=None):
    dims = orc.ae_dims(F, Z)
    flat = orc.formula_params(dims, seed) if flat is None else flat
    h = native.Handle(dims, mode)
    p = _params(flat, mode)
    h.load_params(p)
    return h, dims, flat, p


def rows_of(n, F, mode, seed=5):
    x = np.random.default_rng(seed).random((n, F))
    return torch.from_numpy(x).to(IN_DT[mode]).cuda()


def renorm_args(F, seed=7):
    rng = np.random.default_rng(seed)
    feats = torch.from_numpy(np.stack([rng.normal(size=F) * 10, rng.uniform(0.5, 300.0, size=F)])).cuda()
    mask = torch.from_numpy((rng.random(F) < 0.3).astype(np.uint8)).cuda()
    return feats, mask


def check_bitwise(h, x, what, renorm=True):
    """The two identities of the feature on one handle and one batch, for both 16-bit types."""
    z32 = h.encode(x, out_dtype=torch.float32)
    F = h.dims[-1]
    for h16 in H16:
        z16 = h.encode(x, out_dtype=h16)
        assert z16.dtype == h16 and tuple(z16.shape) == (x.shape[0], h.z_dim)
        assert_same_bits(z16, z32.to(h16), f"{what} encode {h16}")
        wide = z16.to(torch.float32)
        got = h.decode(z16)
        assert got.dtype == torch.float32
        assert_same_bits(got, h.decode(wide), f"{what} decode {h16}")
        assert_same_bits(h.decode(z16, out_dtype=torch.float64), h.decode(wide, out_dtype=torch.float64), f"{what} decode f64 {h16}")
        if renorm:
            feats, mask = renorm_args(F)
            assert_same_bits(h.decode(z16, features=feats, int_mask=mask, out_dtype=torch.float64),
                             h.decode(wide, features=feats, int_mask=mask, out_dtype=torch.float64), f"{what} decode + renorm {h16}")
    return z32


# ---- the dense families ------------------------------------------------------------------------------------------------------
DENSE = [
    pytest.param(24, 15, "fp32", "fused", id="ae24-fp32-chain"),
    pytest.param(24, 15, "fp64", "fused", id="ae24-fp64-chain"),
    pytest.param(24, 15, "bf16", "bf16", id="ae24-bf16"),
    pytest.param(24, 8, "bf16", "bf16", id="ae24z8-bf16-aligned-rows"),
    pytest.param(24, 8, "fp32", "fused", id="ae24z8-fp32-chain"),
    pytest.param(40, 10, "fp32", "fused", id="class-63-columns"),
    pytest.param(100, 12, "fp32", "fused", id="class-64-127-columns"),
    pytest.param(40, 10, "fp64", "fused", id="class-63-columns-fp64"),
    pytest.param(625, 7, "fp32", "fused", id="cfd-625-7"),
    pytest.param(625, 7, "bf16", None, id="cfd-625-7-bf16"),
    pytest.param(2500, 25, "fp32", "fused", id="cfd-2500-25"),
    pytest.param(2500, 25, "bf16", None, id="cfd-2500-25-bf16"),
    pytest.param(512, 6, "fp32", "fused", id="wide-512-6"),
    pytest.param(300, 20, "fp32", "fused", id="wide-class-300-20"),
]


@pytest.mark.parametrize("F,Z,mode,path", DENSE)
def test_dense_families_bitwise_and_oracle(F, Z, mode, path):
    h, dims, flat, _ = ae_handle(F, Z, mode, seed=100 + F + Z)
    assert path is None or h.path == path
    cmode = {native.MODE_F32: "fp32", native.MODE_F64: "fp64", native.MODE_BF16: "bf16"}[h.compute_mode]
    for n in ROWS:
        x = rows_of(n, F, mode, seed=n)
        z32 = check_bitwise(h, x, f"{F}-{Z} {mode} n={n}")
        if n != 513:
            continue
        xr = x.cpu().numpy().astype(np.float64)
        z_ref = orc.encode(dims, flat, xr)
        zmax = np.abs(z_ref).max()
        for h16 in H16:
            z16 = h.encode(x, out_dtype=h16)
            got = z16.to(torch.float64).cpu().numpy()
            err = np.abs(got - z_ref)
            # half an ulp: u |z_ref| in the format's normal range; below float16's (|z| < 2^-14, spacing 2^-24) it is 2^-25 absolute
            half_ulp = np.maximum(U[h16] * np.abs(z_ref), 2.0 ** -25) if h16 == torch.float16 else U[h16] * np.abs(z_ref)
            bound = half_ulp + TOL[cmode] * zmax
            print(f"{F}-{Z} {mode} {h16}: worst |z16 - z_ref| / bound = {(err / bound).max():.3f}")
            assert (err <= bound).all()
            dec = h.decode(z16, out_dtype=IN_DT[mode]).cpu().numpy().astype(np.float64)      # (an fp64 handle's bar is on its float64 output)
            ref = orc.decode(dims, flat, got)
            rel = np.linalg.norm(dec - ref) / np.linalg.norm(ref)
            print(f"{F}-{Z} {mode} {h16}: decode rel-L2 against the oracle on the widened codes = {rel:.3e}")
            assert rel <= TOL[cmode]
        del z32


def test_rows_above_the_chunk_boundaries():
    """One row count above the family's own chunk: the wide-layer staging chunk (262144 rows), the bf16 kernel's persistent grid,
    and the layer-wise workspace chunk (1048576 rows).  Results stay bitwise those of the float32 codes."""
    h, *_ = ae_handle(625, 7, "fp32")
    check_bitwise(h, rows_of((1 << 18) + 77, 625, "fp32"), "625-7 above the staging chunk", renorm=False)
    del h
    torch.cuda.empty_cache()
    for mode in ("fp32", "bf16", "fp64"):
        h, *_ = ae_handle(24, 15, mode)
        check_bitwise(h, rows_of(300001, 24, mode), f"ae24 {mode} 300001 rows", renorm=mode != "fp64")


def test_layerwise_handle(monkeypatch):
    monkeypatch.setenv("BALER_AMD_FORCE_GENERIC", "1")
    monkeypatch.setenv("BALER_AMD_QUIET", "1")
    for mode in ("fp32", "fp64"):
        h, dims, flat, _ = ae_handle(24, 15, mode)
        assert h.path == "generic"
        for n in ROWS:
            check_bitwise(h, rows_of(n, 24, mode, seed=n), f"layer-wise {mode} n={n}")
        if mode == "fp32":
            check_bitwise(h, rows_of((1 << 20) + 100, 24, mode), "layer-wise above its workspace chunk", renorm=False)
    # a shape no fused family serves (other hidden widths): layer-wise without the switch
    monkeypatch.delenv("BALER_AMD_FORCE_GENERIC")
    dims = [30, 64, 32, 9, 32, 64, 30]
    flat = orc.formula_params(dims, 3)
    h = native.Handle(dims, "fp32")
    h.load_params(_params(flat, "fp32"))
    assert h.path == "generic"
    check_bitwise(h, rows_of(513, 30, "fp32"), "layer-wise 30-64-32-9")


@pytest.mark.parametrize("mode", ["fp32", "fp64"])
def test_fpga_family(mode, monkeypatch):
    """FPGA_prototype_model keeps its float32 / float64 stores: float32 workspace + one row conversion (several workspace chunks
    at 5000 rows with the test knob)."""
    n_f, z = 24, 15
    rng = np.random.default_rng(17)
    d = fpga_ref.dims(n_f, z)
    flat = np.concatenate([np.concatenate([rng.uniform(-1, 1, d[l + 1] * d[l]) / np.sqrt(d[l]), rng.uniform(-1, 1, d[l + 1]) / np.sqrt(d[l])])
                           for l in range(6)])
    h = native.Handle(d, mode, act="relu")
    h.load_params(_params(flat, mode))
    assert h.path == "fused" and h.act == "relu"
    for n in ROWS:
        check_bitwise(h, rows_of(n, n_f, mode, seed=n), f"fpga {mode} n={n}")
    monkeypatch.setenv("BALER_AMD_LAT32_ROWS", "1024")
    check_bitwise(h, rows_of(5000, n_f, mode), f"fpga {mode}, 1024-row workspace chunks")


def test_pjconv_family(monkeypatch):
    z = 10
    torch.manual_seed(4)
    flat = models.pj_conv_init(z).numpy()
    h = native.Handle.pj_conv(z, "fp32")
    h.load_params(torch.from_numpy(np.concatenate([flat, [0.0]]).astype(np.float32)).cuda())
    for n in ROWS:
        x = torch.from_numpy(np.random.default_rng(n).random((n, 784)).astype(np.float32)).cuda()
        check_bitwise(h, x, f"PJ_Conv_AE n={n}")
    monkeypatch.setenv("BALER_AMD_LAT32_ROWS", "1024")
    x = torch.from_numpy(np.random.default_rng(9).random((2500, 784)).astype(np.float32)).cuda()
    check_bitwise(h, x, "PJ_Conv_AE, 1024-row workspace chunks", renorm=False)


def _scaled_last_encoder_layer(dims, flat, s):
    """The latent is linear in the last encoder layer (no activation follows it): scaling W3, b3 by s scales every latent by s."""
    f = flat.copy()
    off = sum(dims[l + 1] * dims[l] + dims[l + 1] for l in range(3))
    f[off:off + dims[4] * dims[3] + dims[4]] *= s
    return f


@pytest.mark.parametrize("mode", ["fp32", "fp64", "bf16"])
def test_float16_subnormal_latents(mode):
    """Parameters scaled down (last encoder layer x 2^-11) so that the latents straddle the float16 subnormal range.  Measured on the
    oracle's own latents (CMS rows, formula parameters seed 99): 86.7 % of the entries are below 2^-14 in magnitude and none is below
    2^-24, so most codes are float16 subnormals and must be produced, not flushed.  The test re-measures the share (>= 10 %)."""
    dims = orc.ae_dims(24, 15)
    flat = _scaled_last_encoder_layer(dims, orc.formula_params(dims, 99), 2.0 ** -11)
    raw = orc.normalize(synth.cms_rows(5000))
    z_ref = orc.encode(dims, flat, raw)
    share = float((np.abs(z_ref) < 2.0 ** -14).mean())
    print(f"share of oracle latents below 2^-14: {share:.4f}; largest {np.abs(z_ref).max():.3e}")
    assert share >= 0.1 and (np.abs(z_ref) >= 2.0 ** -14).mean() > 0.01
    h, *_ = ae_handle(24, 15, mode, flat=flat)
    x = torch.from_numpy(raw).to(IN_DT[mode]).cuda()
    check_bitwise(h, x, f"subnormal latents {mode}")
    z16 = h.encode(x, out_dtype=torch.float16)
    got = z16.to(torch.float64).cpu().numpy()
    sub = (np.abs(got) < 2.0 ** -14) & (got != 0)
    assert sub.mean() >= 0.1, "float16 subnormals were flushed"
    # half an ulp: relative 2^-11 in the normal range, absolute 2^-25 below it (the subnormal spacing is 2^-24).  The rounding rule
    # goes through float32 first (two roundings for an fp64 handle), so float32's own half ulp, 2^-24 |z|, is part of the bound: it
    # is 3e-12 here, far above the fp64 mode's 1e-11 * max|z| = 1e-15, and far below the fp32 / bf16 modes' bars.
    bound = np.maximum(U[torch.float16] * np.abs(z_ref), 2.0 ** -25) + 2.0 ** -24 * np.abs(z_ref) + TOL[mode] * np.abs(z_ref).max()
    assert (np.abs(got - z_ref) <= bound).all()


@pytest.mark.parametrize("mode", ["fp32", "fp64", "bf16"])
def test_float16_overflow_gives_inf(mode):
    """Parameters scaled up (last encoder layer x 2^19): measured on the oracle's latents, 13.3 % of the entries exceed 65504 in
    magnitude (largest 9.9e4).  float16 codes overflow to +-inf (no saturation) exactly where the float32 codes round to it;
    bfloat16 codes of the same latents stay finite."""
    dims = orc.ae_dims(24, 15)
    flat = _scaled_last_encoder_layer(dims, orc.formula_params(dims, 99), 2.0 ** 19)
    raw = orc.normalize(synth.cms_rows(5000))
    z_ref = orc.encode(dims, flat, raw)
    over = float((np.abs(z_ref) > 65504).mean())
    print(f"share of oracle latents above 65504: {over:.4f}")
    assert over > 0.01
    h, *_ = ae_handle(24, 15, mode, flat=flat)
    x = torch.from_numpy(raw).to(IN_DT[mode]).cuda()
    z32 = check_bitwise(h, x, f"overflowing latents {mode}", renorm=False)
    z16 = h.encode(x, out_dtype=torch.float16)
    inf = torch.isinf(z16)
    assert torch.equal(inf, z32.abs() >= 65520.0) and bool(inf.any())        # 65520 is the tie that rounds to inf
    assert torch.equal(torch.sign(z16[inf]).float(), torch.sign(z32[inf]))
    assert bool(torch.isfinite(h.encode(x, out_dtype=torch.bfloat16)).all())


def test_nan_and_inf_inputs_stay_nan_and_inf():
    h, *_ = ae_handle(24, 15, "fp32")
    x = rows_of(64, 24, "fp32")
    x[3, 5] = float("nan")
    x[9, 1] = float("inf")
    z32 = h.encode(x)
    for h16 in H16:
        z16 = h.encode(x, out_dtype=h16)
        assert torch.equal(torch.isnan(z16), torch.isnan(z32)) and bool(torch.isnan(z16[3]).all())
        ok = ~torch.isnan(z32)
        assert_same_bits(z16[ok], z32.to(h16)[ok], f"non-NaN codes {h16}")


def test_out_argument_and_row_blocks():
    """helper.compress's pattern: a preallocated 16-bit latent buffer filled row block by row block (odd offsets: 2-byte aligned rows)."""
    h, *_ = ae_handle(24, 15, "fp32")
    x = rows_of(1001, 24, "fp32")
    for h16 in H16:
        out = torch.zeros((1001, 15), dtype=h16, device="cuda")
        for s, e in ((0, 333), (333, 334), (334, 1001)):
            h.encode(x[s:e], out=out[s:e])
        assert_same_bits(out, h.encode(x, out_dtype=torch.float32).to(h16), f"row blocks {h16}")
        dec = torch.empty((1001, 24), dtype=torch.float32, device="cuda")
        for s, e in ((0, 333), (333, 334), (334, 1001)):
            h.decode(out[s:e], out=dec[s:e])
        assert_same_bits(dec, h.decode(out.float()), f"decode row blocks {h16}")


# ---- refusals ----------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5A


def _sentinel(nbytes):
    return torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")


def test_every_other_dtype_argument_refuses_the_new_codes():
    L = native.lib()
    h, dims, flat, params = ae_handle(24, 15, "fp32")
    hp = h._h
    n = 64
    x = rows_of(n, 24, "fp32")
    z = h.encode(x)
    feats = torch.from_numpy(orc.find_minmax(np.random.default_rng(1).random((50, 24)))).cuda()
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)      # noqa: E731
    S = ctypes.c_void_p(0)
    adam = native.AdamHP(1, 1e-3, 0.9, 0.999, 1e-8)
    nb = 1 << 16
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    rows_i = torch.zeros(4, dtype=torch.int64, device="cuda")
    cols_i = torch.zeros(4, dtype=torch.int32, device="cuda")
    del16 = torch.zeros(4, dtype=torch.float16, device="cuda")
    steps = ctypes.c_int64(0)
    batch_rows = (ctypes.c_int64 * 1)(n)
    calls = {
        "bamd_encode x_dtype": lambda c, o: L.bamd_encode(hp, P(x), c, n, None, P(o), native.F32, S),
        "bamd_decode out_dtype": lambda c, o: L.bamd_decode(hp, P(z), native.F32, n, None, None, P(o), c, S),
        "bamd_forward_loss x_dtype": lambda c, o: L.bamd_forward_loss(hp, P(x), c, n, None, None, native.F32, P(o), S),
        "bamd_forward_loss recon_dtype": lambda c, o: L.bamd_forward_loss(hp, P(x), native.F32, n, None, P(o), c, P(o[nb // 2:]), S),
        "bamd_fwd_bwd x_dtype": lambda c, o: L.bamd_fwd_bwd(hp, P(x), c, n, None, P(o), S),
        "bamd_fwd_bwd_latent x_dtype": lambda c, o: L.bamd_fwd_bwd_latent(hp, P(x), c, n, None, P(z), P(o), S),
        "bamd_train_step x_dtype": lambda c, o: L.bamd_train_step(hp, P(x), c, n, None, P(params), P(o), P(m), P(v), ctypes.byref(adam), None, S),
        "bamd_train_epoch x_dtype": lambda c, o: L.bamd_train_epoch(hp, P(x), c, n, 32, None, P(params), P(o), P(m), P(v), ctypes.byref(adam), None,
                                                                  ctypes.byref(steps), S),
        "bamd_train_epoch_dp x_dtype": lambda c, o: L.bamd_train_epoch_dp(hp, P(x), c, batch_rows, 1, None, P(params), P(o), P(m), P(v),
                                                                        ctypes.byref(adam), None, S),
        "bamd_load_params dtype": lambda c, o: L.bamd_load_params(hp, P(params), c, S),
        "bamd_activation_means x_dtype": lambda c, o: L.bamd_activation_means(hp, P(x), c, n, None, P(o), 200, S),
        "bamd_allreduce_sum dtype": lambda c, o: L.bamd_allreduce_sum(hp, P(o), c, 16, S),
        "bamd_minmax dtype": lambda c, o: L.bamd_minmax(P(x), c, n, 24, P(o), S),
        "bamd_col_minmax dtype": lambda c, o: L.bamd_col_minmax(P(x), c, n, 24, P(o), S),
        "bamd_normalize dtype": lambda c, o: L.bamd_normalize(P(x), c, n, 24, P(feats), P(o), native.F32, S),
        "bamd_normalize out_dtype": lambda c, o: L.bamd_normalize(P(x), native.F32, n, 24, P(feats), P(o), c, S),
        "bamd_renormalize dtype": lambda c, o: L.bamd_renormalize(P(x), c, n, 24, P(feats), None, P(o), S),
        "bamd_emd_rows dtype": lambda c, o: L.bamd_emd_rows(P(x), P(x), c, n, 24, P(o), S),
        "bamd_swd dtype": lambda c, o: L.bamd_swd(P(z), P(z), P(z), c, n, 15, 4, 1.0, P(o), P(o[nb // 2:]), S),
        "bamd_error_deltas dtype": lambda c, o: L.bamd_error_deltas(P(x), P(x), c, n * 24, 10.0, P(o), P(o[nb // 2:]), S),
        "bamd_apply_deltas dtype": lambda c, o: L.bamd_apply_deltas(P(o), c, 24, P(rows_i), P(cols_i), P(del16), 4, S),
        "bamd_column_moments dtype": lambda c, o: L.bamd_column_moments(P(x), P(x), c, n, 24, -1, 0.0, P(o), 0, S),
        "bamd_column_hist dtype": lambda c, o: L.bamd_column_hist(P(x), P(x), c, n, 24, -1, 0.0, P(feats), 2, P(o), None, 0, None, None, 0,
                                                                 None, None, 0, S),
    }
    before = params.clone()
    for what, call in calls.items():
        for code in (native.F16, native.BF16):
            out = _sentinel(nb)
            rc = call(code, out)
            torch.cuda.synchronize()
            msg = L.bamd_last_error().decode()
            assert rc == -1, (what, code, rc, msg)
            assert "dtype" in msg and what.split()[0] in msg, (what, msg)
            assert bool((out == SENTINEL).all()), f"{what}: the output buffer was written before the refusal"
    assert torch.equal(params, before) and not bool(m.any()) and not bool(v.any())
    # codes that name no dtype at all are refused by encode / decode too
    out = _sentinel(nb)
    assert L.bamd_encode(hp, P(x), native.F32, n, None, P(out), 4, S) == -1
    assert L.bamd_decode(hp, P(z), -1, n, None, None, P(out), native.F32, S) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    # the binding: 16-bit tensors are refused wherever they are not latent codes
    with pytest.raises(native.NativeError):
        h.encode(x.to(torch.float16))
    with pytest.raises(native.NativeError):
        h.decode(z, out_dtype=torch.bfloat16)
    # and the handle still works
    assert_same_bits(h.encode(x), z, "encode after the refusals")
