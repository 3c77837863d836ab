"""8-bit latent codes on MI355X (bamd_encode / bamd_decode with z_dtype BAMD_U8 = 8).

Store: encode(x, uint8) is q8(encode(x, float32)) of the same handle, exactly.  Load: decode(q) is decode(q.float()) bit for bit, the
fused un-normalise / int-mask epilogue included.  Both for every kernel family, through the float32 workspace in one chunk and in
64-row chunks with a ragged last one.  The handles carry parameters with a latent scale folded in (baler_amd.latent8), calibrated
on the 3rd / 97th percentile so that the codes span 0..255 and rows clamp at both ends.  fp32 / fp64 handles are also held to the
fp64 oracle on the folded parameters.  Refusals, guard bands, the caller's stream and parameter refresh as for the 16-bit codes."""
import ctypes

import numpy as np
import pytest
import torch

import guard_bands as gb
import latent8_cases as lc
import stream_gate as sg
from baler_amd import latent8, native
from baler_amd.modules import models
from oracle import c_oracle as orc

pytestmark = pytest.mark.gpu

ROWS = (1, 17, 257, 4100)
CHUNKED = {"BALER_AMD_LAT32_ROWS": "64"}       # several workspace chunks and a ragged last one at 257 and 4100 rows
TOL = {"fp32": 1e-5, "fp64": 1e-11}            # the existing bars of the two parity modes (tests/test_gpu_parity.py)

# name -> (case of latent8_cases.DENSE or "pj", mode, expected path or None, row counts)
FAMILIES = {
    "ae24-15-fp32": ("ae24-15", "fp32", "fused", ROWS),
    "ae24-2-fp32": ("ae24-2", "fp32", "fused", ROWS),
    "ae24-15-bf16": ("ae24-15", "bf16", "bf16", ROWS),
    "ae24-15-fp16": ("ae24-15", "fp16", "f16", ROWS),
    "ae24-15-fp16x3": ("ae24-15", "fp16x3", "f16x3", ROWS),
    "ae40-10-fp32": ("ae40-10", "fp32", "fused", ROWS),
    "ae100-10-fp32": ("ae100-10", "fp32", "fused", ROWS),
    "cfd625-7-fp32": ("cfd625-7", "fp32", "fused", ROWS),
    "cfd2500-25-fp32": ("cfd2500-25", "fp32", "fused", (33,)),
    "layerwise-400-9-fp32": ("layerwise-400-9", "fp32", "generic", ROWS),
    "ae24-15-fp64": ("ae24-15", "fp64", "fused", ROWS),
    "ae100-40-fp64": ("ae100-40", "fp64", None, ROWS),
    "ae130-9-fp64": ("ae130-9", "fp64", None, ROWS),
    "fpga24-15-fp32": ("fpga24-15", "fp32", "fused", ROWS),
    "pjconv-z10": ("pj", "fp32", None, ROWS),
}
ORACLE = [k for k, v in FAMILIES.items() if v[1] in TOL and v[0] not in ("fpga24-15", "pj")]      # LeakyReLU dense models in a parity mode
PARITY = [k for k, v in FAMILIES.items() if v[1] in TOL]


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(_bits(a), _bits(b)), f"{what}: {int((_bits(a) != _bits(b)).sum())} of {a.numel()} elements differ"


def _pdt(mode):
    return torch.float64 if mode == "fp64" else torch.float32


def dev_params(flat, mode):
    return torch.from_numpy(np.concatenate([np.asarray(flat, dtype=np.float64), [0.0]])).to(_pdt(mode)).cuda()


def new_handle(name):
    case, mode, path, _ = FAMILIES[name]
    if case == "pj":
        h = native.Handle.pj_conv(10, mode)
    else:
        h = native.Handle(lc.DENSE[case][0], mode, act="relu" if case.startswith("fpga") else "leaky_relu")
    assert path is None or h.path == path, (name, h.path)
    return h


def plain_params(name):
    case = FAMILIES[name][0]
    if case == "pj":
        torch.manual_seed(4)
        return models.pj_conv_init(10).numpy().astype(np.float64)
    dims, pseed, _ = lc.DENSE[case]
    return orc.formula_params(dims, pseed)


def layout_of(name):
    case = FAMILIES[name][0]
    return models.pj_conv_layout(10)[0] if case == "pj" else lc.layout(lc.DENSE[case][0])


def rows_of(name, n=lc.ROWS_MAX):
    case, mode = FAMILIES[name][:2]
    x = np.random.default_rng(19).random((lc.ROWS_MAX, 784))[:n] if case == "pj" else lc.rows(case, n)
    return torch.from_numpy(x).to(_pdt(mode)).cuda()


_folded = {}


def folded_params(name):
    """The family's folded parameter vector (float64) with its scale.  LeakyReLU dense models: latent8_cases.folded_case (calibrated on
    the oracle).  FPGA_prototype_model (ReLU) and PJ_Conv_AE have no oracle restatement in c_oracle: calibrated the same way on the
    unfolded handle's own float32 latent."""
    if name in _folded:
        return _folded[name]
    case, mode = FAMILIES[name][:2]
    if case != "pj" and not case.startswith("fpga"):
        _, _, folded, lo, rng = lc.folded_case(case)
    else:
        h = new_handle(name)
        h.load_params(dev_params(plain_params(name), mode))
        lo, rng = lc.clamping_scale(h.encode(rows_of(name, 257), out_dtype=torch.float32).double().cpu().numpy())
        folded = latent8.fold_flat(plain_params(name), layout_of(name), lo, rng)
        h.close()
    _folded[name] = (folded, lo, rng)
    return _folded[name]


def folded_handle(name):
    h = new_handle(name)
    h.load_params(dev_params(folded_params(name)[0], FAMILIES[name][1]))
    return h


def renorm_args(F, seed=7):
    rng = np.random.default_rng(seed)
    feats = torch.from_numpy(np.stack([rng.normal(size=F) * 10, rng.uniform(0.5, 300.0, size=F)])).cuda()
    mask = torch.from_numpy((rng.random(F) < 0.3).astype(np.uint8)).cuda()
    return feats, mask


def check_store_and_load(h, x, what, chunk=None):
    """The two identities on one handle and one batch; -> (float32 latent, codes).  chunk: the rows per workspace chunk that
    BALER_AMD_LAT32_ROWS sets -- the family is then called once per chunk, and "the value the same handle would have stored as
    float32" is that of the same call: the layer-wise path picks its GEMM by the call's row count, and the float32 latent of a
    64-row call differs from that of a 4100-row call in the last bit of a few elements (1 code of 36,900 sat on a tie)."""
    n = x.shape[0]
    step = chunk or n

    def per_call(fn, t):      # the reference side, called with the rows of one workspace chunk at a time
        return torch.cat([fn(t[s:s + step]) for s in range(0, n, step)])
    z32 = per_call(lambda t: h.encode(t, out_dtype=torch.float32), x)
    z8 = h.encode(x, out_dtype=torch.uint8)
    assert z8.dtype == torch.uint8 and tuple(z8.shape) == (x.shape[0], h.z_dim)
    want = latent8.q8(z32.cpu().numpy())
    got = z8.cpu().numpy()
    assert np.array_equal(got, want), f"{what} store: {int((got != want).sum())} of {got.size} codes differ from q8(float32 latent)"
    wide = z8.to(torch.float32)
    dec = h.decode(z8)
    assert dec.dtype == torch.float32
    assert_same_bits(dec, per_call(h.decode, wide), f"{what} load")
    assert_same_bits(h.decode(z8, out_dtype=torch.float64), per_call(lambda t: h.decode(t, out_dtype=torch.float64), wide),
                     f"{what} load, float64 output")
    feats, mask = renorm_args(h.dims[-1])
    assert_same_bits(h.decode(z8, features=feats, int_mask=mask, out_dtype=torch.float64),
                     per_call(lambda t: h.decode(t, features=feats, int_mask=mask, out_dtype=torch.float64), wide),
                     f"{what} load + renorm + int_mask")
    assert_same_bits(h.decode(z8, features=feats, out_dtype=torch.float64),
                     per_call(lambda t: h.decode(t, features=feats, out_dtype=torch.float64), wide), f"{what} load + renorm")
    return z32, z8


@pytest.mark.parametrize("name", list(FAMILIES))
def test_store_and_load_are_exact(name, monkeypatch):
    monkeypatch.setenv("BALER_AMD_QUIET", "1")
    h = folded_handle(name)
    counts = FAMILIES[name][3]
    x_all = rows_of(name, max(counts))
    for n in counts:
        x = x_all[:n].contiguous()
        z32, z8 = check_store_and_load(h, x, f"{name} n={n}")
        if n >= 33:      # the codes span the byte and rows clamp at both ends
            q = z8.cpu().numpy()
            assert q.min() == 0 and q.max() == 255 and len(np.unique(q)) > (20 if n == 33 else 100), f"{name} n={n}: codes do not span 0..255"
            assert bool((z32 < -0.5).any()) and bool((z32 > 255.5).any()), f"{name} n={n}: no row clamps"
        if n in (257, 33, 4100):     # the same call in 64-row workspace chunks: the same bytes
            with monkeypatch.context() as m:
                m.setenv("BALER_AMD_LAT32_ROWS", "64")
                _, z8c = check_store_and_load(h, x, f"{name} n={n}, 64-row workspace chunks", chunk=64)
            if FAMILIES[name][2] != "generic":      # (see check_store_and_load: the layer-wise float32 latent depends on the call's rows)
                assert_same_bits(z8c, z8, f"{name} n={n}: chunked codes against one chunk")


def test_special_values_through_the_kernel():
    """The value set of the store rule through bamd_encode itself: a 2-layer handle [15, 15, 15] with W = I, b = 0, whose latent is
    its input (x * 1 plus zeros: exact, up to the sign of zero and a flushed subnormal, which the rule maps to 0 anyway).  A
    non-finite input turns the other latents of ITS row into NaN (0 * inf), so +-inf and NaN each get a row of their own."""
    v = lc.value_set()
    v = v[np.isfinite(v)]
    v = v[: (len(v) // 15) * 15].reshape(-1, 15)
    odd = np.tile(np.arange(15, dtype=np.float32) + np.float32(0.5), (3, 1))
    odd[0, 4], odd[1, 7], odd[2, 11] = np.inf, -np.inf, np.nan
    v = np.concatenate([v, odd])
    dims = [15, 15, 15]
    flat = np.concatenate([np.eye(15).reshape(-1), np.zeros(15), np.eye(15).reshape(-1), np.zeros(15)])
    h = native.Handle(dims, "fp32")
    h.load_params(dev_params(flat, "fp32"))
    x = torch.from_numpy(v).cuda()
    z32 = h.encode(x, out_dtype=torch.float32).cpu().numpy()
    got = h.encode(x, out_dtype=torch.uint8).cpu().numpy()
    assert np.array_equal(got, latent8.q8(z32))
    assert np.array_equal(got[:-3], latent8.q8(v[:-3])), "finite values: the codes of the inputs themselves"
    assert z32[-3, 4] == np.inf and got[-3, 4] == 255 and z32[-2, 7] == -np.inf and got[-2, 7] == 0
    assert np.isnan(z32[-1]).all() and (got[-1] == 0).all() and np.isnan(z32[-3, 0]) and got[-3, 0] == 0
    # load: every byte widens to its value
    q = torch.arange(256, dtype=torch.uint8, device="cuda").repeat(15)[: 255 * 15].reshape(-1, 15).contiguous()
    assert_same_bits(h.decode(q), h.decode(q.float()), "identity decode")
    assert torch.equal(h.decode(q), q.float())


@pytest.mark.parametrize("name", ORACLE)
def test_against_the_oracle(name, monkeypatch):
    monkeypatch.setenv("BALER_AMD_QUIET", "1")
    case, mode, _, counts = FAMILIES[name]
    dims = lc.DENSE[case][0]
    folded, lo, rng = folded_params(name)
    h = folded_handle(name)
    n = max(counts)
    x = rows_of(name, n)
    c_ref = orc.encode(dims, folded, lc.rows(case, n))
    # the latent at the handle's own precision meets the handle's bar
    lat = h.encode(x, out_dtype=_pdt(mode)).cpu().numpy().astype(np.float64)
    rel = np.linalg.norm(lat - c_ref) / np.linalg.norm(c_ref)
    worst = np.abs(lat - c_ref).max()
    share, near = lc.band_share(c_ref)
    print(f"{name}: folded latent rel-L2 against the oracle {rel:.2e} (bar {TOL[mode]:.0e}), worst |difference| {worst:.2e} code units; "
          f"{100 * share:.2f} % of the oracle's values within {lc.BAND} of a half-integer")
    assert rel < TOL[mode]
    assert share <= lc.BAND_SHARE
    got = h.encode(x, out_dtype=torch.uint8).cpu().numpy()
    want = latent8.q8(c_ref)
    bad = (got != want) & ~near
    assert not bad.any(), f"{name}: {int(bad.sum())} codes outside the band differ from q8(oracle); first at {np.argwhere(bad)[0]}"
    assert (np.abs(got[near].astype(int) - want[near].astype(int)) <= 1).all()
    # decode of the codes against the oracle's decode of the same codes, at the handle's bar
    dec = h.decode(torch.from_numpy(got).cuda(), out_dtype=_pdt(mode)).cpu().numpy().astype(np.float64)
    ref = orc.decode(dims, folded, got.astype(np.float64))
    assert np.linalg.norm(dec - ref) / np.linalg.norm(ref) < TOL[mode]


@pytest.mark.parametrize("name", PARITY)
def test_latent_error_is_half_a_step(name, monkeypatch):
    """compress's own calibration (min and range of the float32 latent over the rows, nothing clamps): the latent a code stands for,
    q / s + lo, is within 0.51 steps of the float32 code of the UNFOLDED handle -- half a step of rounding plus the 5e-3 band of
    the fp32 bar.  fp32 / fp64 handles only: a bf16 / fp16 handle rounds the FOLDED weights to 8 / 11 bits, which moves its latent
    by far more than a hundredth of a step."""
    monkeypatch.setenv("BALER_AMD_QUIET", "1")
    case, mode, _, counts = FAMILIES[name]
    n = max(counts)
    x = rows_of(name, n)
    h = new_handle(name)
    h.load_params(dev_params(plain_params(name), mode))
    z32 = h.encode(x, out_dtype=torch.float32).cpu().numpy().astype(np.float64)
    lo, rng = z32.min(axis=0), z32.max(axis=0) - z32.min(axis=0)
    assert (rng > 0).all()
    h.load_params(dev_params(latent8.fold_flat(plain_params(name), layout_of(name), lo, rng), mode))
    q = h.encode(x, out_dtype=torch.uint8).cpu().numpy()
    err = np.abs(latent8.unscale(q, lo, rng) - z32) / (rng / 255.0)
    print(f"{name}: worst |q / s + lo - z32| = {err.max():.4f} steps; codes {q.min()}..{q.max()}")
    assert q.min() == 0 and q.max() == 255
    assert (err <= 0.51).all()


GUARDED = ["ae24-15-fp32", "ae24-15-bf16", "ae100-10-fp32", "cfd625-7-fp32", "layerwise-400-9-fp32", "ae24-15-fp64", "ae130-9-fp64",
           "fpga24-15-fp32", "pjconv-z10"]


@pytest.mark.parametrize("route", ["default", "lat32-64"])
@pytest.mark.parametrize("name", GUARDED)
def test_guard_bands(name, route, monkeypatch):
    """The (n, z) byte block inside a poisoned arena, 3 lead rows (an odd byte offset for z = 15, 7, 9): the bytes before and after
    it -- the neighbouring row blocks of a sliced call -- are untouched, inputs are only read, and the results are those of the
    unframed call."""
    monkeypatch.setenv("BALER_AMD_QUIET", "1")
    if route == "lat32-64":
        monkeypatch.setenv("BALER_AMD_LAT32_ROWS", "64")
    h = folded_handle(name)
    n, lead = 257, 3
    x = rows_of(name, n)
    z_ref = h.encode(x, out_dtype=torch.uint8)
    d_ref = h.decode(z_ref)
    xv, xa = gb.framed(x, lead, fill=gb.NAN)
    zv, za = gb.framed(torch.empty((n, h.z_dim), dtype=torch.uint8, device="cuda"), lead, fill=gb.POISON)
    snap = xa.clone()
    h.encode(xv, out=zv)
    torch.cuda.synchronize()
    gb.assert_guards_intact(za, lead, n, f"{name} {route} encode to uint8")
    gb.assert_inputs_untouched(xa, snap, f"{name} {route} encode input")
    assert_same_bits(zv, z_ref, f"{name} {route} framed encode")
    qv, qa = gb.framed(z_ref, lead, fill=gb.NAN)
    ov, oa = gb.framed(torch.empty_like(d_ref), lead, fill=gb.POISON)
    snap = qa.clone()
    h.decode(qv, out=ov)
    torch.cuda.synchronize()
    gb.assert_guards_intact(oa, lead, n, f"{name} {route} decode of uint8")
    gb.assert_inputs_untouched(qa, snap, f"{name} {route} decode input")
    assert_same_bits(ov, d_ref, f"{name} {route} framed decode")
    # compress's pattern: a preallocated byte buffer filled row block by row block
    out = gb.poisoned((n, h.z_dim), torch.uint8, "cuda")
    for s, e in ((0, 85), (85, 86), (86, n)):
        h.encode(x[s:e], out=out[s:e])
        torch.cuda.synchronize()
        assert_same_bits(out[s:e], h.encode(x[s:e].clone(), out_dtype=torch.uint8), f"{name} {route} rows {s}:{e}")      # (the same call, unsliced)
        assert e == n or bool((out[e:] == gb.GUARD_BYTE).all()), f"{name} {route}: rows behind block {s}:{e} were written"


# ---- refusals ----------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5A


def _sentinel(nbytes):
    return torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")


def test_every_other_dtype_argument_refuses_code_8():
    L = native.lib()
    dims = orc.ae_dims(24, 15)
    flat = orc.formula_params(dims, 99)
    h = native.Handle(dims, "fp32")
    params = dev_params(flat, "fp32")
    h.load_params(params)
    hp = h._h
    n = 64
    x = rows_of("ae24-15-fp32", n)
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
        out = _sentinel(nb)
        rc = call(native.U8, out)
        torch.cuda.synchronize()
        msg = L.bamd_last_error().decode()
        assert rc == -1, (what, rc, msg)
        assert "dtype" in msg and what.split()[0] in msg, (what, msg)
        assert bool((out == SENTINEL).all()), f"{what}: the output buffer was written before the refusal"
    assert torch.equal(params, before) and not bool(m.any()) and not bool(v.any())
    # codes that name no dtype at all stay refused by encode / decode
    out = _sentinel(nb)
    for code in (4, -1, 5, 7, 9, 16):
        assert L.bamd_encode(hp, P(x), native.F32, n, None, P(out), code, S) == -1
        assert L.bamd_decode(hp, P(z), code, n, None, None, P(out), native.F32, S) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    # the binding: uint8 tensors are refused wherever they are not latent codes
    with pytest.raises(native.NativeError):
        h.encode(x.to(torch.uint8))
    with pytest.raises(native.NativeError):
        h.decode(z, out_dtype=torch.uint8)
    with pytest.raises(native.NativeError):
        native.minmax(x.to(torch.uint8))
    with pytest.raises(native.NativeError):
        h.load_params(params.to(torch.uint8))
    # and the handle still works, with code 8 where it belongs
    assert_same_bits(h.encode(x), z, "encode after the refusals")
    assert np.array_equal(h.encode(x, out_dtype=torch.uint8).cpu().numpy(), latent8.q8(z.cpu().numpy()))


# ---- the caller's stream -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,env", [("ae24-15-fp32", {}), ("cfd625-7-fp32", CHUNKED)])
def test_uint8_encode_and_decode_run_on_the_callers_stream(name, env, monkeypatch):
    monkeypatch.setenv("BALER_AMD_QUIET", "1")
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    mode = FAMILIES[name][1]
    h = new_handle(name)
    p = dev_params(folded_params(name)[0], mode)
    other = (p * 0.5 + 0.01).contiguous()
    n = 129
    F, Z = h.dims[0], h.z_dim

    def seq(t):
        o = {}
        h.load_params(t["p"])
        o["z8"] = h.encode(t["x"], out=sg.out((n, Z), torch.uint8))
        o["d8"] = h.decode(o["z8"], out=sg.out((n, F), torch.float32))
        return o
    got = sg.run_gated(seq, {"p": p, "x": rows_of(name, n)}, reset=lambda: h.load_params(other), same={None: assert_same_bits},
                       what=f"uint8 codes {name}")
    q = got["outs"]["z8"].cpu().numpy()
    assert q.min() == 0 and q.max() == 255
    print(f"[streams] uint8 codes {name} {env}: host enqueue {got['warm_ms']:.2f} ms")


# ---- parameter refresh -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ae24-15-fp32", "ae24-15-bf16", "ae24-15-fp16x3", "ae100-10-fp32", "cfd625-7-fp32", "ae130-9-fp64",
                                  "fpga24-15-fp32", "pjconv-z10"])
def test_a_differently_folded_vector_is_seen_by_the_next_call(name, monkeypatch):
    """load_flat of another fold on a model whose handle has already run: the next encode / decode gives, bit for bit, what a
    freshly created handle with that vector gives (compress folds after its calibration pass on the same handle)."""
    monkeypatch.setenv("BALER_AMD_QUIET", "1")
    case, mode = FAMILIES[name][:2]
    folded, lo, rng = folded_params(name)
    second = latent8.fold_flat(plain_params(name), layout_of(name), lo - 0.25 * rng, 1.5 * rng)
    x = rows_of(name, 257)
    h = new_handle(name)
    h.load_params(dev_params(plain_params(name), mode))
    h.encode(x, out_dtype=torch.float32)                      # the calibration pass
    h.load_params(dev_params(folded, mode))
    z_a = h.encode(x, out_dtype=torch.uint8)
    d_a = h.decode(z_a)
    h.load_params(dev_params(second, mode))
    z_b = h.encode(x, out_dtype=torch.uint8)
    d_b = h.decode(z_b)
    assert not torch.equal(z_a, z_b)
    for vec, z, d in ((folded, z_a, d_a), (second, z_b, d_b)):
        fresh = new_handle(name)
        fresh.load_params(dev_params(vec, mode))
        assert_same_bits(fresh.encode(x, out_dtype=torch.uint8), z, f"{name}: codes against a fresh handle")
        assert_same_bits(fresh.decode(z), d, f"{name}: decode against a fresh handle")
        fresh.close()
