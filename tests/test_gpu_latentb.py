"""Packed sub-byte latent codes on MI355X (bamd_encode / bamd_decode with z_dtype BAMD_UB(b) = 0x100 | b, b = 1 .. 7).

Store: encode(x, code_bits=b) is pack_rows(qb(encode(x, float32), b), b) of the same handle, byte for byte -- the bit layout and the
rounding rule as baler_amd.latent8 states them in NumPy.  Load: decode(bytes, code_bits=b) is decode(float32 of unpack_rows(bytes))
bit for bit, the fused un-normalise / int-mask epilogue included.  Both for every kernel family, through the float32 workspace in
one chunk and in 64-row chunks with a one-row last chunk.  The handles carry parameters with a latent scale for 2**b - 1 levels
folded in (calibrated on the 3rd / 97th percentile, so codes span the range and rows clamp at both ends).  The fp32 families are
also held to the fp64 oracle at b = 5.  Refusals, guard bands and the caller's stream as for the 8-bit codes."""
import ctypes

import numpy as np
import pytest
import torch

import latent8_cases as lc
import latentb_cases as lb
import stream_gate as sg
from baler_amd import latent8, native
from baler_amd.modules import models
from oracle import c_oracle as orc

pytestmark = pytest.mark.gpu

ROWS = (1, 2, 65, 257)
SOME_BITS = (1, 3, 5, 7)

# name -> (case of latentb_cases.DENSE or "pj", mode, expected path or None, widths)
FAMILIES = {
    "ae24-15-fp32": ("ae24-15", "fp32", "fused", lb.BITS),            # the fp32 register chain: all seven widths
    "ae30-7-fp32": ("ae30-7", "fp32", "fused", SOME_BITS),            # the run-time-width class
    "ae130-9-fp32": ("ae130-9", "fp32", None, SOME_BITS),             # wide tables, z = 9
    "cfd625-7-fp32": ("cfd625-7", "fp32", "fused", SOME_BITS),        # the wide-layer kernels, z = 7 ...
    "cfd2500-25-fp32": ("cfd2500-25", "fp32", "fused", SOME_BITS),    # ... and z = 25
    "ae24-15-fp64": ("ae24-15", "fp64", "fused", SOME_BITS),
    "ae130-9-fp64": ("ae130-9", "fp64", None, SOME_BITS),             # the wide fp64 class
    "ae24-15-bf16": ("ae24-15", "bf16", "bf16", SOME_BITS),
    "ae24-15-fp16": ("ae24-15", "fp16", "f16", SOME_BITS),
    "ae24-15-fp16x3": ("ae24-15", "fp16x3", "f16x3", SOME_BITS),
    "fpga24-15-fp32": ("fpga24-15", "fp32", "fused", SOME_BITS),      # ReLU
    "pjconv-z10": ("pj", "fp32", None, SOME_BITS),
    "layerwise-400-9-fp32": ("layerwise-400-9", "fp32", "generic", SOME_BITS),
}
ROW_DEPENDENT = ("layerwise-400-9-fp32",)      # the layer-wise path picks its GEMM by the rows of a call: its float32 latent depends on them


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
        h = native.Handle(lb.DENSE[case][0], mode, act="relu" if case.startswith("fpga") else "leaky_relu")
    assert path is None or h.path == path, (name, h.path)
    return h


def plain_params(name):
    case = FAMILIES[name][0]
    if case == "pj":
        torch.manual_seed(4)
        return models.pj_conv_init(10).numpy().astype(np.float64)
    dims, pseed, _ = lb.DENSE[case]
    return orc.formula_params(dims, pseed)


def layout_of(name):
    case = FAMILIES[name][0]
    return models.pj_conv_layout(10)[0] if case == "pj" else lc.layout(lb.DENSE[case][0])


def rows_of(name, n=lb.ROWS_MAX):
    case, mode = FAMILIES[name][:2]
    x = np.random.default_rng(19).random((lb.ROWS_MAX, 784))[:n] if case == "pj" else lb.rows(case, n)
    return torch.from_numpy(x).to(_pdt(mode)).cuda()


_scale = {}


def scale_of_family(h, name):
    """[lo ; rng] of the family, the 3rd / 97th percentile of the UNFOLDED handle's own float32 latent of the case's 257 rows (the
    handle is left with the plain parameters loaded)."""
    if name not in _scale:
        h.load_params(dev_params(plain_params(name), FAMILIES[name][1]))
        _scale[name] = lc.clamping_scale(h.encode(rows_of(name), out_dtype=torch.float32).double().cpu().numpy())
    return _scale[name]


def load_folded(h, name, bits):
    lo, rng = scale_of_family(h, name)
    h.load_params(dev_params(latent8.fold_flat(plain_params(name), layout_of(name), lo, rng, latent8.levels(bits)), FAMILIES[name][1]))


def renorm_args(F, seed=7):
    rng = np.random.default_rng(seed)
    feats = torch.from_numpy(np.stack([rng.normal(size=F) * 10, rng.uniform(0.5, 300.0, size=F)])).cuda()
    mask = torch.from_numpy((rng.random(F) < 0.3).astype(np.uint8)).cuda()
    return feats, mask


def check_store_and_load(h, x, bits, what, chunk=None, epilogue=True):
    """The two identities on one handle and one batch; -> (float32 latent, packed bytes).  chunk: the rows per workspace chunk that
    BALER_AMD_LAT32_ROWS sets -- the family is then called once per chunk, so the float32 reference is taken with the same row
    chunks (the layer-wise path picks its GEMM by the rows of a call)."""
    n, z = x.shape[0], h.z_dim
    S = -(-z * bits // 8)
    step = chunk or n

    def per_call(fn, t):
        return torch.cat([fn(t[s:s + step]) for s in range(0, n, step)])
    z32 = per_call(lambda t: h.encode(t, out_dtype=torch.float32), x)
    zb = h.encode(x, out_dtype=torch.uint8, code_bits=bits)
    assert zb.dtype == torch.uint8 and tuple(zb.shape) == (n, S), (what, tuple(zb.shape))
    got = zb.cpu().numpy()
    want = latent8.pack_rows(latent8.qb(z32.cpu().numpy(), bits), bits)
    assert np.array_equal(got, want), f"{what} store: {int((got != want).sum())} of {got.size} bytes differ from pack_rows(qb(float32 latent))"
    wide = torch.from_numpy(latent8.unpack_rows(got, z, bits).astype(np.float32)).cuda()
    dec = h.decode(zb, code_bits=bits)
    assert dec.dtype == torch.float32
    assert_same_bits(dec, per_call(h.decode, wide), f"{what} load")
    if epilogue:
        feats, mask = renorm_args(h.dims[-1])
        assert_same_bits(h.decode(zb, features=feats, int_mask=mask, out_dtype=torch.float64, code_bits=bits),
                         per_call(lambda t: h.decode(t, features=feats, int_mask=mask, out_dtype=torch.float64), wide),
                         f"{what} load + renorm + int_mask")
    return z32, zb


@pytest.mark.parametrize("name", list(FAMILIES))
def test_store_and_load_are_exact(name, monkeypatch):
    monkeypatch.setenv("BALER_AMD_QUIET", "1")
    h = new_handle(name)
    x_all = rows_of(name)
    for bits in FAMILIES[name][3]:
        load_folded(h, name, bits)
        top = 2 ** bits - 1
        for n in ROWS:
            x = x_all[:n].contiguous()
            z32, zb = check_store_and_load(h, x, bits, f"{name} b={bits} n={n}", epilogue=n in (2, 257))
            if n == 257:
                q = latent8.unpack_rows(zb.cpu().numpy(), h.z_dim, bits)
                assert q.min() == 0 and q.max() == top and len(np.unique(q)) > top // 2, f"{name} b={bits}: codes do not span 0..{top}"
                assert bool((z32 < 0).any()) and bool((z32 > top).any()), f"{name} b={bits}: no latent beyond the ends of the code range"
                # the same call in 64-row workspace chunks (five chunks, the last of one row): the same bytes
                with monkeypatch.context() as m:
                    m.setenv("BALER_AMD_LAT32_ROWS", "64")
                    _, zc = check_store_and_load(h, x, bits, f"{name} b={bits} n={n}, 64-row workspace chunks", chunk=64, epilogue=False)
                if name not in ROW_DEPENDENT:
                    assert_same_bits(zc, zb, f"{name} b={bits}: chunked bytes against one chunk")
    h.close()


def test_narrow_latent_sweep(monkeypatch):
    """Every phase of a code against a byte boundary: the layer-wise path with latent widths 1 .. 17, every b, 67 rows."""
    monkeypatch.setenv("BALER_AMD_QUIET", "1")
    monkeypatch.setenv("BALER_AMD_FORCE_GENERIC", "1")
    x = torch.from_numpy(np.random.default_rng(23).random((67, 8))).float().cuda()
    for z in range(1, 18):
        dims = [8, 16, 16, 16, z, 16, 16, 16, 8]
        flat = orc.formula_params(dims, 70 + z)
        h = native.Handle(dims, "fp32")
        assert h.path == "generic" and h.z_dim == z
        h.load_params(dev_params(flat, "fp32"))
        lo, rng = lc.clamping_scale(h.encode(x, out_dtype=torch.float32).double().cpu().numpy())
        for bits in lb.BITS:
            h.load_params(dev_params(latent8.fold_flat(flat, lc.layout(dims), lo, rng, latent8.levels(bits)), "fp32"))
            _, zb = check_store_and_load(h, x, bits, f"z={z} b={bits}", epilogue=False)
            q = latent8.unpack_rows(zb.cpu().numpy(), z, bits)
            assert q.min() == 0 and q.max() == 2 ** bits - 1
        h.close()


def test_clamp_and_special_values_through_the_kernel():
    """AE(24, 15) whose last encoder bias drives five latent columns to +1e9, -1e9, NaN, +inf and -inf: the codes are 2**b - 1, 0, 0,
    2**b - 1 and 0 in every row; the other columns keep their codes."""
    dims = orc.ae_dims(24, 15)
    flat = orc.formula_params(dims, 99)
    (_, be), _ = latent8.latent_tensors(lc.layout(dims))
    drive = {2: 1e9, 5: -1e9, 7: np.nan, 11: np.inf, 14: -np.inf}
    x = torch.from_numpy(lb.rows("ae24-15", 65)).float().cuda()
    h = native.Handle(dims, "fp32")
    for bits in lb.BITS:
        top = 2 ** bits - 1
        lo, rng = lb.oracle_case("ae24-15")[2:4]
        f = latent8.fold_flat(flat, lc.layout(dims), lo, rng, top)
        for k, v in drive.items():
            f[be[1] + k] = v
        h.load_params(dev_params(f, "fp32"))
        z32 = h.encode(x, out_dtype=torch.float32).cpu().numpy()
        assert (z32[:, 2] > 1e8).all() and (z32[:, 5] < -1e8).all() and np.isnan(z32[:, 7]).all()
        assert (z32[:, 11] == np.inf).all() and (z32[:, 14] == -np.inf).all()
        got = h.encode(x, out_dtype=torch.uint8, code_bits=bits).cpu().numpy()
        q = latent8.unpack_rows(got, 15, bits)
        for k, want in {2: top, 5: 0, 7: 0, 11: top, 14: 0}.items():
            assert (q[:, k] == want).all(), f"b={bits} column {k}: {np.unique(q[:, k])} instead of {want}"
        assert np.array_equal(got, latent8.pack_rows(latent8.qb(z32, bits), bits))
    # the value set of the store rule through an identity handle (W = I, b = 0: the latent is the input)
    eye = np.concatenate([np.eye(15).reshape(-1), np.zeros(15), np.eye(15).reshape(-1), np.zeros(15)])
    hi = native.Handle([15, 15, 15], "fp32")
    hi.load_params(dev_params(eye, "fp32"))
    for bits in lb.BITS:
        v = lb.value_set(bits)
        v = v[np.isfinite(v)]
        v = v[: (len(v) // 15) * 15].reshape(-1, 15)
        got = hi.encode(torch.from_numpy(v).cuda(), out_dtype=torch.uint8, code_bits=bits).cpu().numpy()
        assert np.array_equal(got, latent8.pack_rows(latent8.qb(v, bits), bits)), f"b={bits}: the codes of the inputs themselves"
        # load: every code widens to its value, padding bits of the last byte are ignored
        q = (np.arange(15 * 40).reshape(40, 15) % (2 ** bits)).astype(np.uint8)
        packed = latent8.pack_rows(q, bits)
        pad = 8 * packed.shape[1] - 15 * bits
        dirty = packed.copy()
        if pad:
            dirty[:, -1] |= np.uint8((0xFF << (8 - pad)) & 0xFF)
        for rows in (packed, dirty):
            assert torch.equal(hi.decode(torch.from_numpy(rows).cuda(), code_bits=bits), torch.from_numpy(q.astype(np.float32)).cuda())


GUARDED = ["ae24-15-fp32", "cfd625-7-fp32", "ae130-9-fp64", "ae24-15-bf16", "pjconv-z10", "layerwise-400-9-fp32"]


@pytest.mark.parametrize("route", ["default", "lat32-64"])
@pytest.mark.parametrize("name", GUARDED)
def test_guard_bands(name, route, monkeypatch):
    """The (n, S) byte block inside a flat arena of poison bytes, starting at an ODD byte offset: encode leaves every byte outside
    the block untouched (a lane that packed one byte too many, or a wider store, would show) and writes the bytes of the unframed
    call.  Decode: the block sits in an arena of 0xFF bytes and once more in an arena of zero bytes; both give the bits of the
    unframed call and leave the arena as it was.  A load of a byte outside the block whose bits are then masked away cannot be seen
    by any arena; what the two fills rule out is that such bits reach a result."""
    monkeypatch.setenv("BALER_AMD_QUIET", "1")
    if route == "lat32-64":
        monkeypatch.setenv("BALER_AMD_LAT32_ROWS", "64")
    h = new_handle(name)
    n, off, tail = 257, 4097, 8192
    x = rows_of(name, n)
    for bits in SOME_BITS:
        load_folded(h, name, bits)
        S = -(-h.z_dim * bits // 8)
        z_ref = h.encode(x, out_dtype=torch.uint8, code_bits=bits)
        d_ref = h.decode(z_ref, code_bits=bits)
        arena = torch.full((off + n * S + tail,), 0x5A, dtype=torch.uint8, device="cuda")
        block = arena[off:off + n * S].view(n, S)
        assert block.data_ptr() % 2 == 1 and block.is_contiguous()
        h.encode(x, out=block, code_bits=bits)
        torch.cuda.synchronize()
        assert bool((arena[:off] == 0x5A).all()) and bool((arena[off + n * S:] == 0x5A).all()), f"{name} {route} b={bits}: bytes outside the block were written"
        assert_same_bits(block, z_ref, f"{name} {route} b={bits} framed encode")
        for fill in (0xFF, 0x00):
            arena.fill_(fill)
            block.copy_(z_ref)
            snap = arena.clone()
            assert_same_bits(h.decode(block, code_bits=bits), d_ref, f"{name} {route} b={bits} framed decode, arena of {fill:#x}")
            torch.cuda.synchronize()
            assert torch.equal(arena, snap), f"{name} {route} b={bits}: decode wrote to its input arena"
        # compress's pattern: a preallocated byte buffer filled row block by row block
        out = torch.full((n, S), 0x5A, dtype=torch.uint8, device="cuda")
        for s, e in ((0, 85), (85, 86), (86, n)):
            h.encode(x[s:e], out=out[s:e], code_bits=bits)
            torch.cuda.synchronize()
            if name not in ROW_DEPENDENT:
                assert_same_bits(out[s:e], z_ref[s:e], f"{name} {route} b={bits} rows {s}:{e}")
            assert e == n or bool((out[e:] == 0x5A).all()), f"{name} {route} b={bits}: rows behind block {s}:{e} were written"
    h.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5A


def _sentinel(nbytes):
    return torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")


def test_every_other_dtype_argument_refuses_packed_codes():
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
    for code in (native.UB(1), native.UB(5), native.UB(7), 0x100, 0x108):
        for what, call in calls.items():
            out = _sentinel(nb)
            rc = call(code, out)
            torch.cuda.synchronize()
            msg = L.bamd_last_error().decode()
            assert rc == -1, (what, hex(code), rc, msg)
            assert "dtype" in msg and what.split()[0] in msg, (what, hex(code), msg)
            assert bool((out == SENTINEL).all()), f"{what} {code:#x}: the output buffer was written before the refusal"
    assert torch.equal(params, before) and not bool(m.any()) and not bool(v.any())
    # kinds that name nothing, and the codes that were refused before, stay refused by encode / decode, naming z_dtype
    out = _sentinel(nb)
    for code in (0x100, 0x108, 0x109, 0x205, 0x1FF, 4, -1, 5, 7, 9, 16):
        for rc in (L.bamd_encode(hp, P(x), native.F32, n, None, P(out), code, S),
                   L.bamd_decode(hp, P(z), code, n, None, None, P(out), native.F32, S)):
            assert rc == -1 and "z_dtype" in L.bamd_last_error().decode(), hex(code)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    # the binding: a z buffer whose width is not S = ceil(15 b / 8) is refused, naming z, before the library is called
    for bits, width in ((5, 15), (5, 9), (5, 11), (1, 1), (7, 15)):
        with pytest.raises(native.NativeError, match="z"):
            h.decode(torch.zeros((n, width), dtype=torch.uint8, device="cuda"), code_bits=bits)
        o = torch.full((n, width), SENTINEL, dtype=torch.uint8, device="cuda")
        with pytest.raises(native.NativeError):
            h.encode(x, out=o, code_bits=bits)
        assert bool((o == SENTINEL).all())
    with pytest.raises(native.NativeError):
        h.encode(x, out_dtype=torch.float32, code_bits=5)
    for bad in (0, 8, 9):
        with pytest.raises(native.NativeError):
            h.encode(x, out_dtype=torch.uint8, code_bits=bad)
    # n_rows = 0 and null pointers behave as for BAMD_U8
    assert L.bamd_encode(hp, None, native.F32, 0, None, None, native.UB(5), S) == 0
    assert L.bamd_decode(hp, None, native.UB(5), 0, None, None, None, native.F32, S) == 0
    assert L.bamd_encode(hp, P(x), native.F32, n, None, None, native.UB(5), S) == -1
    assert L.bamd_decode(hp, None, native.UB(5), n, None, None, P(out), native.F32, S) == -1
    # and the handle still works: a uint8 tensor without code_bits is still BAMD_U8, one byte per code
    assert_same_bits(h.encode(x), z, "encode after the refusals")
    z8 = h.encode(x, out_dtype=torch.uint8)
    assert tuple(z8.shape) == (n, 15) and np.array_equal(z8.cpu().numpy(), latent8.q8(z.cpu().numpy()))
    assert_same_bits(h.decode(z8), h.decode(z8.float()), "uint8 codes without code_bits")


# ---- the caller's stream -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,env,bits", [("ae24-15-fp32", {}, 5), ("cfd625-7-fp32", {"BALER_AMD_LAT32_ROWS": "64"}, 3)])
def test_packed_encode_and_decode_run_on_the_callers_stream(name, env, bits, monkeypatch):
    monkeypatch.setenv("BALER_AMD_QUIET", "1")
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    mode = FAMILIES[name][1]
    h = new_handle(name)
    lo, rng = scale_of_family(h, name)
    p = dev_params(latent8.fold_flat(plain_params(name), layout_of(name), lo, rng, latent8.levels(bits)), mode)
    other = (p * 0.5 + 0.01).contiguous()
    n = 129
    F, Z = h.dims[0], h.z_dim
    S = -(-Z * bits // 8)

    def seq(t):
        o = {}
        h.load_params(t["p"])
        o["zb"] = h.encode(t["x"], out=sg.out((n, S), torch.uint8), code_bits=bits)
        o["db"] = h.decode(o["zb"], out=sg.out((n, F), torch.float32), code_bits=bits)
        return o
    got = sg.run_gated(seq, {"p": p, "x": rows_of(name, n)}, reset=lambda: h.load_params(other), same={None: assert_same_bits},
                       what=f"packed {bits}-bit codes {name}")
    q = latent8.unpack_rows(got["outs"]["zb"].cpu().numpy(), Z, bits)
    assert q.min() == 0 and q.max() == 2 ** bits - 1
    print(f"[streams] packed {bits}-bit codes {name} {env}: host enqueue {got['warm_ms']:.2f} ms")


# ---- the oracle --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lb.ORACLE_CASES)
def test_against_the_oracle(name, monkeypatch):
    """b = 5, fp32: with q* = qb of the oracle's folded float64 latent, |q - q*| <= 1 everywhere and q == q* wherever the oracle's
    latent is farther than BAND from a half-integer; the share left out is within BAND_SHARE (also asserted on the CPU,
    tests/test_latentb_host.py)."""
    monkeypatch.setenv("BALER_AMD_QUIET", "1")
    bits = lb.ORACLE_BITS
    dims, folded, lo, rng = lb.folded_case(name, bits)
    h = native.Handle(dims, "fp32")
    h.load_params(dev_params(folded, "fp32"))
    x = torch.from_numpy(lb.rows(name)).float().cuda()
    c_ref = orc.encode(dims, folded, lb.rows(name))
    share, near = lb.band_share(c_ref, bits)
    got = latent8.unpack_rows(h.encode(x, out_dtype=torch.uint8, code_bits=bits).cpu().numpy(), dims[len(dims) // 2], bits)
    want = latent8.qb(c_ref, bits)
    diff = np.abs(got.astype(int) - want.astype(int))
    print(f"{name} b={bits}: {int((diff != 0).sum())} of {diff.size} codes differ from qb(oracle), worst {diff.max()}; "
          f"{100 * share:.2f} % of the oracle's values within {lb.BAND} of a half-integer")
    assert share <= lb.BAND_SHARE
    assert diff.max() <= 1
    bad = (got != want) & ~near
    assert not bad.any(), f"{name}: {int(bad.sum())} codes outside the band differ from qb(oracle); first at {np.argwhere(bad)[0]}"
    # decode of the packed codes against the oracle's decode of the same codes, at the fp32 bar
    dec = h.decode(torch.from_numpy(latent8.pack_rows(got, bits)).cuda(), code_bits=bits).cpu().numpy().astype(np.float64)
    ref = orc.decode(dims, folded, got.astype(np.float64))
    assert np.linalg.norm(dec - ref) / np.linalg.norm(ref) < 1e-5
