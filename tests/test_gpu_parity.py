"""GPU parity tests: the HIP path, called through the C ABI (ctypes), against the CPU oracle on the
same seeded inputs and against the golden vectors generated from the imported reference.

Tolerances (BASELINE.json north_star: 1e-5 relative fp32 tolerance vs the fp64 reference):
  fp32 mode  rel-L2 <= 1e-5 on encode/decode/forward/loss/gradients/first Adam steps
  fp64 mode  rel-L2 <= 1e-11 (summation order differs from the scalar oracle), loss curve 1e-9
  integer/exact work (min/max, normalise in fp64, truncation)  bit-exact
"""
import numpy as np
import pytest
import torch

import grad_tensors as gt
from baler_amd import native, synth
from oracle import c_oracle as orc

pytestmark = pytest.mark.gpu

TOL32 = 1e-5
TOL64 = 1e-11


def rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def rel(a, b):
    """THE error measure of the fp32 / fp64 parity assertions below: the larger of the rel-L2 error and the max-norm error
    max|a - b| / max|b| of the tensor pair.  A single element off by 1e-3 in a million-element tensor passes a 1e-5 rel-L2 bar;
    it does not pass this one.  (The bf16 throughput mode is held to rel-L2 only, `rel_l2`: its bar is a statistical one.)"""
    return max(rel_l2(a, b), maxerr(a, b))


def maxerr(a, b):
    """max |a - b| / max |b|: a single outlier of 1e-3 in a million-element tensor passes a 1e-5 rel-L2 bar; this one sees it."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300) if b.size else 0.0


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def make_handle(dims, flat, mode):
    h = native.Handle(dims, mode)
    p = dev(np.concatenate([flat, [0.0]]), torch.float64 if mode == "fp64" else torch.float32)
    h.load_params(p)
    return h, p


def off_the_kink(dims, flat, n, seed, margin=2e-5):
    """n uniform random rows none of whose LeakyReLU pre-activations lies within `margin` of 0 (fp64 forward in numpy).  A float32
    pre-activation whose sign differs from the float64 one's flips that element's derivative between 1 and 0.01 -- one such row in
    300 moves the gradient of the layers below it by 1e-3, an error of the COMPARISON (float32 vs float64 data), not of the
    kernels; measured: AE(40, 20) 300 rows seed 300: 8.6e-4 on en1 / en2 only, AE(24, 16) 12289 rows: 3e-5 on every layer but
    de4.  The max-norm bars below are held on rows that stay clear of the kink."""
    rng = np.random.default_rng(seed)
    x = rng.random((2 * n + 64, dims[0]))
    a, off, keep = x, 0, np.ones(x.shape[0], dtype=bool)
    for l in range(len(dims) - 1):
        K, N = dims[l], dims[l + 1]
        W, b = flat[off:off + K * N].reshape(N, K), flat[off + K * N:off + K * N + N]
        off += K * N + N
        a = a @ W.T + b
        if l not in (3, 7):                       # en4 and de4 have no activation (models.py:148-165)
            keep &= np.abs(a).min(axis=1) > margin
            a = np.where(a > 0, a, 0.01 * a)
    x = x[keep]
    assert x.shape[0] >= n
    return np.ascontiguousarray(x[:n])


@pytest.fixture(scope="module")
def data10k():
    return orc.normalize(synth.cms_rows(10000))


# ---- normalisation --------------------------------------------------------------------------------
def test_minmax_normalize_bit_exact(golden):
    g = golden("g1_normalize.npz")
    raw = dev(g["raw"])
    feats = native.minmax(raw)
    assert np.array_equal(feats.cpu().numpy(), g["features"])
    normed = native.normalize(raw, feats, torch.float64)
    assert np.array_equal(normed.cpu().numpy(), g["normalized"])
    ren = native.renormalize(normed, feats)
    assert np.array_equal(ren.cpu().numpy(), g["renormalized"])


@pytest.mark.parametrize("data,expected", [
    ([[1, 2, 3], [4, 5, 6], [7, 8, 9]], [[1, 2, 3], [6, 6, 6]]),
    ([[-1, -2, -3], [-4, -5, -6], [-7, -8, -9]], [[-7, -8, -9], [6, 6, 6]]),
    ([[0, 0, 0], [1, 1, 1], [2, 2, 2]], [[0, 0, 0], [2, 2, 2]]),
])
def test_find_minmax_reference_vectors(data, expected):
    # reference tests/test_data_processing.py:52-67, through the product's data_processing mirror
    from baler_amd.modules import data_processing
    out = data_processing.find_minmax(np.array(data, dtype=np.float64))
    assert np.array_equal(out, np.array(expected, dtype=np.float64))


def test_normalize_renormalize_reference_vectors():
    # reference tests/test_data_processing.py:70-121
    from baler_amd.modules import data_processing
    out = data_processing.normalize(np.array([1.0, 2.0, 3.0, 4.0, 5.0]), False)
    np.testing.assert_almost_equal(out, [0.0, 0.25, 0.5, 0.75, 1.0])
    assert np.array_equal(data_processing.normalize(np.array([1, 2, 3, 4, 5]), True), [1, 2, 3, 4, 5])
    r = data_processing.renormalize_std(np.array([0.1, 0.2, 0.3, 0.4, 0.5]), 1, 2)
    np.testing.assert_array_equal(r, np.array([1.2, 1.4, 1.6, 1.8, 2.0]))
    data = np.array([[-1, 2], [-0.5, 6], [0, 10], [1, 18]], dtype=float)
    normed = (data - data.min(0)) / (data.max(0) - data.min(0))
    np.testing.assert_array_equal(data_processing.renormalize_func(normed, [-1, 2], [2, 16]), data)


def test_minmax_large_and_wide():
    x = synth.cms_rows(200_003)
    feats = native.minmax(dev(x)).cpu().numpy()
    assert np.array_equal(feats[0], x.min(0)) and np.array_equal(feats[1], x.max(0) - x.min(0))
    w = synth.wide_rows(777, 2500)
    fw = native.minmax(dev(w)).cpu().numpy()
    assert np.array_equal(fw[0], w.min(0)) and np.array_equal(fw[1], w.max(0) - w.min(0))
    f32 = native.minmax(dev(x, torch.float32)).cpu().numpy()
    x32 = x.astype(np.float32).astype(np.float64)
    assert np.array_equal(f32[0], x32.min(0))


# ---- encode / decode / loss -----------------------------------------------------------------------
@pytest.mark.parametrize("mode,tol", [("fp32", TOL32), ("fp64", TOL64)])
def test_encode_decode_forward_golden(golden, mode, tol):
    g = golden("g2_ae24_io.npz")
    dims = orc.ae_dims(24, 15)
    h, _ = make_handle(dims, orc.formula_params(dims, int(g["seed"])), mode)
    x = dev(g["x"])
    z = h.encode(x)
    assert z.dtype == torch.float64 and rel(z.cpu().numpy(), g["z"]) < tol
    dec = h.decode(dev(g["z"]))
    assert rel(dec.cpu().numpy(), g["decoded"]) < tol
    recon, loss = h.forward_loss(x)
    assert rel(recon.cpu().numpy(), g["forward"]) < tol
    assert abs(loss.item() - g["loss"]) < tol * abs(g["loss"])
    # fp32 I/O gives the same numbers to fp32 precision
    z32 = h.encode(dev(g["x"], torch.float32))
    assert z32.dtype == torch.float32 and rel(z32.cpu().numpy(), g["z"]) < TOL32


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 65, 511, 1000])
def test_encode_ragged_sizes(n, data10k):
    dims = orc.ae_dims(24, 15)
    flat = orc.formula_params(dims, 21)
    h, _ = make_handle(dims, flat, "fp32")
    x = data10k[:n]
    assert rel(h.encode(dev(x)).cpu().numpy(), orc.encode(dims, flat, x)) < TOL32
    z = orc.encode(dims, flat, x)
    assert rel(h.decode(dev(z)).cpu().numpy(), orc.decode(dims, flat, z)) < TOL32


def test_encode_empty():
    dims = orc.ae_dims(24, 15)
    h, _ = make_handle(dims, orc.formula_params(dims, 21), "fp32")
    z = h.encode(torch.empty((0, 24), dtype=torch.float64, device="cuda"))
    assert tuple(z.shape) == (0, 15)


def test_encode_fused_normalisation(data10k):
    """encode(raw, features) == encode(normalize(raw)) -- the fused form of helper.py:500-504."""
    dims = orc.ae_dims(24, 15)
    flat = orc.formula_params(dims, 22)
    h, _ = make_handle(dims, flat, "fp32")
    raw = synth.cms_rows(4096)
    feats = native.minmax(dev(raw))
    z = h.encode(dev(raw), features=feats)
    want = orc.encode(dims, flat, orc.normalize(raw))
    assert rel(z.cpu().numpy(), want) < TOL32


def test_decode_renorm_and_int_cast(golden):
    g = golden("g8_decompress.npz")
    dims = orc.ae_dims(24, 15)
    h, _ = make_handle(dims, orc.formula_params(dims, int(g["seed"])), "fp64")
    nf = dev(g["normalization_features"])
    mask = torch.as_tensor(g["int_mask"].astype(np.uint8)).cuda()
    pre = h.decode(dev(g["z"]), features=nf)
    assert rel(pre.cpu().numpy(), g["pre_cast"]) < TOL64
    post = h.decode(dev(g["z"]), features=nf, int_mask=mask).cpu().numpy()
    cols = g["int_mask"].astype(bool)
    # float columns: untouched by the cast; int columns: truncated toward zero, equal to the reference
    # except where the pre-cast value sits within rounding of an integer (the cast is discontinuous)
    assert rel(post[:, ~cols], g["post_cast"][:, ~cols]) < TOL64
    near_int = np.abs(g["pre_cast"] - np.round(g["pre_cast"])) < 1e-9 * np.maximum(1, np.abs(g["pre_cast"]))
    assert ((post == g["post_cast"]) | near_int)[:, cols].all()
    assert np.array_equal(post[:, cols], np.trunc(post[:, cols]))
    # fp32 mode: compare before the cast at 1e-5
    h32, _ = make_handle(dims, orc.formula_params(dims, int(g["seed"])), "fp32")
    pre32 = h32.decode(dev(g["z"]), features=nf)
    assert rel(pre32.cpu().numpy(), g["pre_cast"]) < TOL32
    # the standalone renormalise kernel is exact given the same decoded input
    post2 = native.renormalize(dev(g["decoded"]), nf, mask).cpu().numpy()
    assert np.array_equal(post2, g["post_cast"])


# ---- gradients / Adam -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode,tol", [("fp32", TOL32), ("fp64", TOL64)])
def test_gradients_golden(golden, data10k, mode, tol):
    g = golden("g5_ae24_grads.npz")
    dims = orc.ae_dims(24, 15)
    flat = orc.formula_params(dims, int(g["seed"]))
    h, p = make_handle(dims, flat, mode)
    x = data10k[int(g["row0"]):int(g["row0"]) + int(g["n_rows"])]
    grads = torch.zeros_like(p)
    h.fwd_bwd(dev(x), grads)
    gh = grads.cpu().numpy().astype(np.float64)
    assert abs(gh[-1] - g["loss"]) < tol * abs(g["loss"])
    assert rel(gh[:-1][g["sample_idx"]], g["sample_val"]) < tol
    norms, off = [], 0
    for l in range(8):
        for n in (dims[l + 1] * dims[l], dims[l + 1]):
            norms.append(np.linalg.norm(gh[off:off + n]))
            off += n
    assert rel(norms, g["tensor_l2"]) < tol
    # full vector against the oracle on the same inputs, per tensor
    _, go = orc.fwd_bwd(dims, flat, x)
    gt.assert_per_tensor(gh[:-1], go, dims, tol, f"golden {mode}")
    # bitwise reproducible run to run (fixed-order reductions)
    grads2 = torch.zeros_like(p)
    h.fwd_bwd(dev(x), grads2)
    assert torch.equal(grads, grads2)


@pytest.mark.parametrize("path", ["small-batch", "throughput"])
@pytest.mark.parametrize("n", [1, 7, 100, 272, 513, 4099, 9999])
def test_gradients_ragged(n, path, data10k, monkeypatch):
    """Both fused training paths on ragged batch sizes: the small-batch kernels (chain + weight-gradient tiles, the
    default up to 12288 rows) and the throughput pair (forced by BALER_AMD_LATENCY_ROWS=0, read at bamd_create)."""
    if path == "throughput":
        monkeypatch.setenv("BALER_AMD_LATENCY_ROWS", "0")
    dims = orc.ae_dims(24, 15)
    flat = orc.formula_params(dims, 31)
    h, p = make_handle(dims, flat, "fp32")
    grads = torch.zeros_like(p)
    h.fwd_bwd(dev(data10k[:n]), grads)
    lo, go = orc.fwd_bwd(dims, flat, data10k[:n])
    gh = grads.cpu().numpy().astype(np.float64)
    assert rel(gh[:-1], go) < TOL32 and abs(gh[-1] - lo) < TOL32 * lo


@pytest.mark.parametrize("n", [1, 7, 16, 17, 272, 513, 1009, 1040, 4099, 12288, 12289, 70001])
def test_fp64_fused_step_ragged(n, data10k):
    """fp64 mode: every batch runs on the fused fp64 step (chain + weight-gradient tiles on v_mfma_f64_16x16x4_f64, fused64.hip; from
    1024 rows on the tiles in 2 x 4 blocks over 8 or 16 block ranges + a finishing launch; beyond 262144 rows chunk after chunk:
    test_fp64_fused_step_beyond_one_chunk); within 1e-11 of the scalar fp64 oracle, and bamd_train_step == bamd_fwd_bwd + bamd_adam_step
    bit for bit."""
    dims = orc.ae_dims(24, 15)
    flat = orc.formula_params(dims, 23)
    x = data10k[:n] if n <= 10000 else orc.normalize(synth.cms_rows(n, row0=11))
    h, p = make_handle(dims, flat, "fp64")
    grads = torch.zeros_like(p)
    h.fwd_bwd(dev(x), grads)
    lo, go = orc.fwd_bwd(dims, flat, x)
    gh = grads.cpu().numpy()
    assert rel(gh[:-1], go) < TOL64 and abs(gh[-1] - lo) < TOL64 * lo
    gt.assert_per_tensor(gh[:-1], go, dims, TOL64, f"fp64 n={n}")
    g2 = torch.zeros_like(p)
    h.fwd_bwd(dev(x.astype(np.float32)), g2)                                 # float32 rows are widened on load
    lo32, go32 = orc.fwd_bwd(dims, flat, x.astype(np.float32).astype(np.float64))
    assert rel(g2.cpu().numpy()[:-1], go32) < TOL64
    gt.assert_per_tensor(g2.cpu().numpy()[:-1], go32, dims, TOL64, f"fp64 n={n} float32 rows")
    # one-call step == two-call step
    m1, v1, m2, v2 = (torch.zeros_like(p) for _ in range(4))
    p1, p2 = p.clone(), p.clone()
    h1, _ = make_handle(dims, flat, "fp64")
    h1.train_step(dev(x), p1, m1, v1, 1, 1e-3)
    h.adam_step(p2, grads, m2, v2, 1, 1e-3)
    assert torch.equal(p1[:-1], p2[:-1]) and torch.equal(m1[:-1], m2[:-1]) and torch.equal(v1[:-1], v2[:-1])
    # ... and the next step uses the refreshed packed weights
    g3, g4 = torch.zeros_like(p), torch.zeros_like(p)
    h1.fwd_bwd(dev(x), g3)
    h.fwd_bwd(dev(x), g4)
    assert torch.equal(g3, g4)
    _, go2 = orc.fwd_bwd(dims, p2.cpu().numpy()[:-1], x)
    assert rel(g4.cpu().numpy()[:-1], go2) < TOL64
    gt.assert_per_tensor(g4.cpu().numpy()[:-1], go2, dims, TOL64, f"fp64 n={n} after the step")


@pytest.mark.parametrize("F,Z", [(30, 8), (25, 10), (47, 12), (63, 15), (16, 4), (1, 1), (33, 15), (24, 16), (40, 20), (63, 31), (31, 17)])
def test_fp64_any_narrow_table_runs_fused(F, Z):
    """The fp64 mode -- the reference's own dtype (models.py:128-136) -- for tables other than the 24-column one: class instantiations
    of the fp64 kernels with run-time widths (Impl64<31|47|63, 15|31, true>: register-chained inference, both training chains, the
    weight-gradient tile blocks, the fused Adam step), against the scalar fp64 oracle at 1e-11: encode / decode (+ fused
    un-normalisation and int truncation) / forward + loss, gradients at 1 .. 20,001 rows (exchange chain, register chain, tile blocks),
    float32 and float64 rows, normalise-on-load, the one-call step == fwd_bwd + adam_step bit for bit."""
    dims = orc.ae_dims(F, Z)
    flat = orc.formula_params(dims, 300 + F)
    h, p = make_handle(dims, flat, "fp64")
    assert h.path == "fused"
    rng = np.random.default_rng(F * 10 + Z)
    for n in (1, 17, 333, 4099):
        x = rng.random((n, F))
        z_ref = orc.encode(dims, flat, x)
        assert rel(h.encode(dev(x)).cpu().numpy(), z_ref) < TOL64, n
        x32 = x.astype(np.float32)
        assert rel(h.encode(dev(x32)).cpu().numpy(), orc.encode(dims, flat, x32.astype(np.float64))) < 1e-6      # float32 output of float32 rows
        assert rel(h.decode(dev(z_ref)).cpu().numpy(), orc.decode(dims, flat, z_ref)) < TOL64
        recon, loss = h.forward_loss(dev(x))
        fw = orc.forward(dims, flat, x)
        assert rel(recon.cpu().numpy(), fw) < TOL64 and abs(loss.item() - orc.loss(x, fw)) < TOL64 * loss.item()
    raw = rng.normal(size=(777, F)) * 50 + 7
    mn, rg = raw.min(0), raw.max(0) - raw.min(0)
    feats = dev(np.stack([mn, rg]))
    xn = (raw - mn) / rg
    zn = orc.encode(dims, flat, xn)
    assert rel(h.encode(dev(raw), features=feats).cpu().numpy(), zn) < TOL64
    mask = np.zeros(F, dtype=np.uint8)
    mask[::3] = 1
    out = h.decode(dev(zn), features=feats, int_mask=dev(mask)).cpu().numpy()
    want = orc.cast_int_cols(orc.renormalize(orc.decode(dims, flat, zn), mn, rg), mask)
    edge = np.abs(want - np.round(want)) < 1e-9
    assert np.array_equal(np.isnan(out), np.isnan(want)) and rel(out[~edge], want[~edge]) < TOL64
    for n in (1, 100, 513, 20001):
        x = rng.random((n, F))
        lo, go = orc.fwd_bwd(dims, flat, x)
        grads = torch.full_like(p, 3.0)
        h.fwd_bwd(dev(x), grads)
        gh = grads.cpu().numpy()
        assert rel(gh[:-1], go) < TOL64 and abs(gh[-1] - lo) < TOL64 * lo, n
        gt.assert_per_tensor(gh[:-1], go, dims, TOL64, f"fp64 AE({F}, {Z}) n={n}")
    lo2, go2 = orc.fwd_bwd(dims, flat, xn)
    g2 = torch.zeros_like(p)
    h.fwd_bwd(dev(raw), g2, features=feats)
    assert rel(g2.cpu().numpy()[:-1], go2) < TOL64
    gt.assert_per_tensor(g2.cpu().numpy()[:-1], go2, dims, TOL64, f"fp64 AE({F}, {Z}) normalise-on-load")
    x = rng.random((512, F))
    m1, v1, m2, v2 = (torch.zeros_like(p) for _ in range(4))
    p1, p2 = p.clone(), p.clone()
    h1, _ = make_handle(dims, flat, "fp64")
    h1.train_step(dev(x), p1, m1, v1, 1, 1e-3)
    g = torch.zeros_like(p)
    h.fwd_bwd(dev(x), g)
    h.adam_step(p2, g, m2, v2, 1, 1e-3)
    assert torch.equal(p1[:-1], p2[:-1]) and torch.equal(m1[:-1], m2[:-1]) and torch.equal(v1[:-1], v2[:-1])
    st = orc.FitState(dims, flat)
    _, g_o = orc.fwd_bwd(dims, flat, x)
    orc.adam_step(st.params, g_o, st.m, st.v, 1, 1e-3)
    assert rel_l2(p1.cpu().numpy()[:-1], st.params) < 1e-9
    assert rel(h1.encode(dev(x)).cpu().numpy(), orc.encode(dims, st.params, x)) < 1e-9


@pytest.mark.parametrize("F,Z", [(64, 16), (80, 16), (100, 31), (127, 1), (96, 20), (100, 63), (40, 40), (127, 32)])
def test_fp64_mid_width_small_batch_step_is_fused(F, Z, monkeypatch, capfd):
    """64 .. 127 columns in the reference's own dtype (models.py:128-136 builds AE(n_features, z_dim) in float64 for any table) at the
    reference's batch size and beyond: every training batch runs on the 4-row chain (chain64q_kernel, two input slots per thread) +
    dw64_kernel, chunk after chunk with the gradients added in order -- against the oracle at 1e-11 at ragged sizes and over several
    chunks, against the layer-wise kernels on the same batch (the switch is read per call), train_step == fwd_bwd + adam_step bit for bit
    with the packed copies following the step; encode / decode / forward + loss on the register-chained inference kernel (fused64j.hip),
    normalisation and the int mask fused."""
    dims = orc.ae_dims(F, Z)
    flat = orc.formula_params(dims, 600 + F)
    h, p = make_handle(dims, flat, "fp64")
    assert h.path == "fused" and "layer by layer" not in capfd.readouterr().err
    rng = np.random.default_rng(F)
    for n in (1, 37, 512, 513, 1536, 1537):
        x = rng.random((n, F))
        lo, go = orc.fwd_bwd(dims, flat, x)
        g = torch.full_like(p, 5.0)
        h.fwd_bwd(dev(x), g)
        gh = g.cpu().numpy()
        assert rel(gh[:-1], go) < TOL64 and abs(gh[-1] - lo) < TOL64 * lo, (F, Z, n)
        gt.assert_per_tensor(gh[:-1], go, dims, TOL64, f"fp64 AE({F}, {Z}) n={n}")
        if n in (37, 512):
            monkeypatch.setenv("BALER_AMD_F64_QCHAIN_BLKS", "0")       # the layer-wise kernels on the same batch
            g2 = torch.zeros_like(p)
            h.fwd_bwd(dev(x), g2)
            monkeypatch.delenv("BALER_AMD_F64_QCHAIN_BLKS")
            assert rel(g2.cpu().numpy(), gh) < 1e-12 and not np.array_equal(g2.cpu().numpy(), gh)      # two different kernels
            g3 = torch.zeros_like(p)
            h.fwd_bwd(dev(x.astype(np.float32)), g3)                   # float32 rows are widened on load
            _, go32 = orc.fwd_bwd(dims, flat, x.astype(np.float32).astype(np.float64))
            assert rel(g3.cpu().numpy()[:-1], go32) < TOL64
            gt.assert_per_tensor(g3.cpu().numpy()[:-1], go32, dims, TOL64, f"fp64 AE({F}, {Z}) n={n} float32 rows")
    # several chunks (ragged last one), gradients added in chunk order; a batch beyond one chunk through train_step (fwd_bwd + the Adam kernel)
    monkeypatch.setenv("BALER_AMD_F64_QCHAIN_BLKS", "300")
    x = rng.random((20001, F))
    lo, go = orc.fwd_bwd(dims, flat, x)
    g = torch.zeros_like(p)
    h.fwd_bwd(dev(x), g)
    assert rel(g.cpu().numpy()[:-1], go) < TOL64 and abs(g.cpu().numpy()[-1] - lo) < TOL64 * lo
    gt.assert_per_tensor(g.cpu().numpy()[:-1], go, dims, TOL64, f"fp64 AE({F}, {Z}) n=20001 in chunks")
    pa, ma, va = p.clone(), torch.zeros_like(p), torch.zeros_like(p)
    ha, _ = make_handle(dims, flat, "fp64")
    ha.train_step(dev(x), pa, ma, va, 1, 1e-3)
    pb, mb_, vb = p.clone(), torch.zeros_like(p), torch.zeros_like(p)
    h.adam_step(pb, g, mb_, vb, 1, 1e-3)
    assert torch.equal(pa[:-1], pb[:-1])
    h.load_params(p)
    monkeypatch.delenv("BALER_AMD_F64_QCHAIN_BLKS")
    # inference: ragged sizes, float32 rows, fused (un)normalisation and int truncation, the loss of forward + loss
    for n in (1, 37, 4099):
        x = rng.random((n, F))
        z_ref = orc.encode(dims, flat, x)
        assert rel(h.encode(dev(x)).cpu().numpy(), z_ref) < TOL64, (F, Z, n)
        assert rel(h.decode(dev(z_ref)).cpu().numpy(), orc.decode(dims, flat, z_ref)) < TOL64
        recon, loss = h.forward_loss(dev(x))
        want = orc.forward(dims, flat, x)
        assert rel(recon.cpu().numpy(), want) < TOL64 and abs(loss.item() - ((want - x) ** 2).sum() / F) < TOL64 * max(1.0, ((want - x) ** 2).sum() / F)
    raw = rng.uniform(-40, 90, size=(257, F))
    feats = orc.find_minmax(raw)
    z1 = h.encode(dev(raw), features=dev(feats)).cpu().numpy()
    assert rel(z1, orc.encode(dims, flat, orc.normalize(raw))) < TOL64
    mask = np.zeros(F, dtype=np.uint8)
    mask[[0, F - 1]] = 1
    outd = h.decode(dev(z1), features=dev(feats), int_mask=dev(mask)).cpu().numpy()
    wantd = orc.renormalize(orc.decode(dims, flat, z1), feats[0], feats[1])
    assert rel(outd[:, mask == 0], wantd[:, mask == 0]) < TOL64 and np.mean(outd[:, mask == 1] == np.trunc(wantd[:, mask == 1])) > 0.99
    # normalise-on-load
    raw = rng.uniform(-3, 9, size=(300, F))
    feats = orc.find_minmax(raw)
    g = torch.zeros_like(p)
    h.fwd_bwd(dev(raw), g, features=dev(feats))
    lo, go = orc.fwd_bwd(dims, flat, orc.normalize(raw))
    assert rel(g.cpu().numpy()[:-1], go) < TOL64
    gt.assert_per_tensor(g.cpu().numpy()[:-1], go, dims, TOL64, f"fp64 AE({F}, {Z}) normalise-on-load")
    # the one-call step == the two-call step, and the next step (and the layer-wise encode) see the new weights
    x = rng.random((512, F))
    g = torch.zeros_like(p)
    h.fwd_bwd(dev(x), g)
    m1, v1, m2, v2 = (torch.zeros_like(p) for _ in range(4))
    p1, p2 = p.clone(), p.clone()
    h1, _ = make_handle(dims, flat, "fp64")
    h1.train_step(dev(x), p1, m1, v1, 1, 1e-3)
    h.adam_step(p2, g, m2, v2, 1, 1e-3)
    assert torch.equal(p1[:-1], p2[:-1]) and torch.equal(m1[:-1], m2[:-1]) and torch.equal(v1[:-1], v2[:-1])
    g3, g4 = torch.zeros_like(p), torch.zeros_like(p)
    h1.fwd_bwd(dev(x), g3)
    h.fwd_bwd(dev(x), g4)
    assert torch.equal(g3, g4)
    pn = p2.cpu().numpy()[:-1]
    _, go2 = orc.fwd_bwd(dims, pn, x)
    assert rel(g4.cpu().numpy()[:-1], go2) < TOL64
    gt.assert_per_tensor(g4.cpu().numpy()[:-1], go2, dims, TOL64, f"fp64 AE({F}, {Z}) after the step")
    assert rel(h1.encode(dev(x)).cpu().numpy(), orc.encode(dims, pn, x)) < TOL64


@pytest.mark.parametrize("n", [1, 33, 1000, 16385, 70001])
def test_fp64_register_chain_equals_exchange_chain(n, monkeypatch):
    """The fp64 training chains -- one workgroup per 16-row block exchanging every layer through LDS (chain64_kernel), one workgroup
    per FOUR rows on the 4x4x4 MFMA (chain64q_kernel: the 512-row step, up to 1,536 rows by default) and one WAVE per block with the activations in registers and the LeakyReLU signs in bit masks (chain64r_kernel: from 1,024
    blocks on) -- write the same images bit for bit (every output element accumulates its k blocks in the same order), so the
    gradients are IDENTICAL and only the loss sum (another order over the block's lanes) may differ in its last bits.  Both against
    the oracle at 1e-11; normalise-on-load through both."""
    dims = orc.ae_dims(24, 15)
    flat = orc.formula_params(dims, 23)
    raw = synth.cms_rows(n, row0=11)
    feats = orc.find_minmax(synth.cms_rows(max(n, 64), row0=11))
    x = (raw - feats[0]) / feats[1]
    h, p = make_handle(dims, flat, "fp64")
    lo, go = orc.fwd_bwd(dims, flat, x)
    got = {}
    for tag, blks, qblks in (("registers", "0", "0"), ("exchange", "1000000000", "0"), ("four-rows", "1000000000", "1000000000")):
        monkeypatch.setenv("BALER_AMD_F64_REGCHAIN_BLKS", blks)
        monkeypatch.setenv("BALER_AMD_F64_QCHAIN_BLKS", qblks)
        g = torch.zeros_like(p)
        h.fwd_bwd(dev(raw), g, features=dev(feats))
        got[tag] = g.cpu().numpy()
        assert rel(got[tag][:-1], go) < TOL64 and abs(got[tag][-1] - lo) < TOL64 * max(lo, 1e-300), tag
        gt.assert_per_tensor(got[tag][:-1], go, dims, TOL64, f"fp64 n={n} {tag}")
    assert np.array_equal(got["registers"][:-1], got["exchange"][:-1])
    assert abs(got["registers"][-1] - got["exchange"][-1]) <= 1e-13 * max(abs(got["exchange"][-1]), 1e-300)
    # the 4-row chain (chain64q_kernel, v_mfma_f64_4x4x4: four rows per workgroup) sums every contraction in two interleaved chains and
    # splits en4 / de4 over the waves: the same numbers to rounding, not to the bit
    assert rel(got["four-rows"], got["exchange"]) < 1e-13


@pytest.mark.parametrize("n,chunk", [(70001, 4096), (20000, 16), (300_001, None), (1_000_003, None)])
def test_fp64_fused_step_beyond_one_chunk(n, chunk, monkeypatch):
    """fp64 batches beyond 262,144 rows (the images of the fused pair take 13 KB per row) run chunk after chunk over the same image
    buffer, the partial weight-gradient tiles of all chunks added in order by one finishing launch: 300,001 and 1,000,003 rows (the
    headline workload in the reference's own dtype) against the scalar fp64 oracle at 1e-11, the one-call step == fwd_bwd + adam_step bit
    for bit, bitwise reproducible; small chunks (BALER_AMD_F64_CHUNK_ROWS) force many chunks incl. a ragged last one."""
    if chunk:
        monkeypatch.setenv("BALER_AMD_F64_CHUNK_ROWS", str(chunk))
    dims = orc.ae_dims(24, 15)
    flat = orc.formula_params(dims, 29)
    x = orc.normalize(synth.cms_rows(n, row0=5))
    h, p = make_handle(dims, flat, "fp64")
    assert h.path == "fused"
    xd = dev(x)
    grads, g2 = torch.zeros_like(p), torch.zeros_like(p)
    h.fwd_bwd(xd, grads)
    h.fwd_bwd(xd, g2)
    assert torch.equal(grads, g2)
    lo, go = orc.fwd_bwd(dims, flat, x)
    gh = grads.cpu().numpy()
    assert rel(gh[:-1], go) < TOL64 and abs(gh[-1] - lo) < TOL64 * lo
    gt.assert_per_tensor(gh[:-1], go, dims, TOL64, f"fp64 n={n} chunk={chunk}")
    m1, v1, m2, v2 = (torch.zeros_like(p) for _ in range(4))
    p1, p2 = p.clone(), p.clone()
    h1, _ = make_handle(dims, flat, "fp64")
    h1.train_step(xd, p1, m1, v1, 1, 1e-3)
    h.adam_step(p2, grads, m2, v2, 1, 1e-3)
    assert torch.equal(p1[:-1], p2[:-1]) and torch.equal(m1[:-1], m2[:-1]) and torch.equal(v1[:-1], v2[:-1])
    if chunk:      # the same batch in one chunk: another summation order, same numbers to 1e-13
        monkeypatch.delenv("BALER_AMD_F64_CHUNK_ROWS")
        h2, _ = make_handle(dims, flat, "fp64")
        g3 = torch.zeros_like(p)
        h2.fwd_bwd(xd, g3)
        assert rel(g3.cpu().numpy(), gh) < 1e-13


def test_empty_shard_gives_zero_grad():
    dims = orc.ae_dims(24, 15)
    h, p = make_handle(dims, orc.formula_params(dims, 31), "fp32")
    grads = torch.ones_like(p)
    h.fwd_bwd(torch.empty((0, 24), dtype=torch.float64, device="cuda"), grads)
    assert float(grads.abs().sum()) == 0.0


@pytest.mark.parametrize("mode,tol", [("fp32", TOL32), ("fp64", 1e-10)])
def test_adam_trajectory_golden(golden, data10k, mode, tol):
    g = golden("g6_ae24_adam.npz")
    dims = orc.ae_dims(24, 15)
    h, p = make_handle(dims, orc.formula_params(dims, int(g["seed"])), mode)
    m, v, grads = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    acc = torch.zeros(1, dtype=torch.float64, device="cuda")
    for step in range(1, 13):
        lr = 1e-3 if step < 11 else 5e-4
        h.fwd_bwd(dev(data10k[(step - 1) * 512: step * 512]), grads)
        h.adam_step(p, grads, m, v, step, lr, loss_accum=acc)
        assert abs(float(grads[-1]) - g["losses"][step - 1]) < tol * g["losses"][step - 1]
        if step in (1, 2, 3, 10, 12):
            ph = p.cpu().numpy().astype(np.float64)[:-1]
            assert rel(ph[g["sample_idx"]], g[f"p{step}"]) < tol, step
    assert abs(acc.item() - g["losses"].sum()) < tol * g["losses"].sum()


def test_big_batch_dp_equivalent(golden):
    """3 steps at batch 4096 == what an 8 x 512 data-parallel step must equal;
    also: the gradient of a batch is the SUM of the gradients of its row shards."""
    g = golden("g12_dp_bs4096.npz")
    dims = orc.ae_dims(24, 15)
    flat = orc.formula_params(dims, int(g["seed"]))
    data = orc.normalize(synth.cms_rows(int(g["n_rows"])))
    h, p = make_handle(dims, flat, "fp32")
    m, v, grads = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    shard_sum = torch.zeros_like(p)
    tmp = torch.zeros_like(p)
    for s in range(3):
        xb = dev(data[s * 4096:(s + 1) * 4096])
        if s == 0:
            for r in range(8):
                h.fwd_bwd(xb[r * 512:(r + 1) * 512], tmp)
                shard_sum += tmp
        h.fwd_bwd(xb, grads)
        if s == 0:
            assert rel(shard_sum.cpu().numpy(), grads.cpu().numpy()) < 1e-6
        assert abs(float(grads[-1]) - g["losses"][s]) < TOL32 * g["losses"][s]
        h.adam_step(p, grads, m, v, s + 1, 1e-3)
    assert rel(p.cpu().numpy().astype(np.float64)[:-1][g["sample_idx"]], g["sample"]) < TOL32


# ---- diagnostics ----------------------------------------------------------------------------------
def test_activation_means_golden(golden, data10k):
    g = golden("g9_activations.npz")
    dims = orc.ae_dims(24, 15)
    h, _ = make_handle(dims, orc.formula_params(dims, int(g["seed"])), "fp32")
    a = h.activation_means(dev(data10k[:int(g["n_rows"])])).cpu().numpy()
    assert a.shape == (6, 200)
    assert np.array_equal(np.isnan(a), np.isnan(g["activations"]))
    assert rel(np.nan_to_num(a), np.nan_to_num(g["activations"])) < TOL32


def test_emd_golden(golden):
    g = golden("g10_emd.npz")
    out = native.emd_rows(dev(g["x"]), dev(g["recon"]))
    assert abs(out.item() - g["emd"]) < 1e-12 * abs(g["emd"])


# ---- other configs --------------------------------------------------------------------------------
def test_cfd_dense_golden(golden):
    g = golden("g11_cfd_dense.npz")
    dims = orc.ae_dims(2500, 25)
    flat = orc.formula_params(dims, int(g["seed"]))
    h, p = make_handle(dims, flat, "fp32")
    x = dev(synth.cfd_field(int(g["n_frames"])).reshape(-1, 2500), torch.float32)
    z = h.encode(x)
    assert rel(z.cpu().numpy(), g["z"]) < TOL32
    dec = h.decode(dev(g["z"], torch.float32)).cpu().numpy()
    assert rel(dec[:, :64], g["decoded_head"]) < TOL32
    assert rel(dec.astype(np.float64).sum(axis=1), g["decoded_rowsum"]) < TOL32
    grads = torch.zeros_like(p)
    h.fwd_bwd(x, grads)
    gh = grads.cpu().numpy().astype(np.float64)
    # The reference computes CFD_dense_AE in float32 (models.py:186-209 builds it without dtype=float64), so ITS loss and per-tensor
    # gradient norms -- all the fixture can hold of a 1,037,575-element gradient -- carry float32 rounding of their own: 1e-4 against
    # those; the gradient ITSELF is held to the 1e-5 bar, per tensor, L2 and max-norm, against the fp64 oracle on the same frames.
    assert abs(gh[-1] - g["loss"]) < 1e-4 * abs(g["loss"])
    lo, go = orc.fwd_bwd(dims, flat, x.cpu().numpy().astype(np.float64))
    assert abs(gh[-1] - lo) < TOL32 * lo
    gt.assert_per_tensor(gh[:-1], go, dims, TOL32, "CFD_dense_AE golden")
    norms = [np.linalg.norm(gh[s]) for _, s in gt.tensor_slices(dims)]
    assert rel(norms, g["grad_tensor_l2"]) < 1e-4


@pytest.mark.parametrize("n", [1, 15, 16, 17, 100, 1037])
def test_cfd_dense_wide_layer_kernels_vs_oracle(n):
    """CFD_dense_AE(2500, 25) encode / decode on the fused wide-layer kernels (en1 / de4 streamed, the six narrow layers on the
    register chain) at ragged row counts, float32 and float64 rows, with and without the fused (un)normalisation, against the
    oracle and against the layer-wise path (BALER_AMD_FORCE_GENERIC, the independent cross-check)."""
    dims = orc.ae_dims(2500, 25)
    flat = orc.formula_params(dims, 17)
    h, _ = make_handle(dims, flat, "fp32")
    raw = synth.cfd_field(n + 3)[3:].reshape(n, 2500)
    mn, rg = raw.min(0) - 0.01, raw.max(0) - raw.min(0) + 0.02
    xn = (raw - mn) / rg
    z_ref = orc.encode(dims, flat, xn)
    feats = dev(np.stack([mn, rg]))
    # float32 RAW rows: the rounding of the raw value to float32 happens before the normalisation and is part of the input, not of
    # the kernel -- the oracle gets the same rounded rows, and the bar stays 1e-5 (it was 2e-4 against the unrounded rows)
    raw32 = raw.astype(np.float32).astype(np.float64)
    z_ref32 = orc.encode(dims, flat, (raw32 - mn) / rg)
    for xin, f, want in ((dev(xn, torch.float32), None, z_ref), (dev(xn), None, z_ref), (dev(raw), feats, z_ref),
                         (dev(raw, torch.float32), feats, z_ref32)):
        z = h.encode(xin, features=f, out_dtype=torch.float32)
        assert rel(z.cpu().numpy(), want) < TOL32, (xin.dtype, f is None)
    rec_ref = orc.decode(dims, flat, z_ref)
    for zin in (dev(z_ref, torch.float32), dev(z_ref)):
        assert rel(h.decode(zin).cpu().numpy(), rec_ref) < TOL32
    mask = np.zeros(2500, dtype=np.uint8)
    mask[::7] = 1
    dec = h.decode(dev(z_ref, torch.float32), features=feats, int_mask=torch.as_tensor(mask).cuda(), out_dtype=torch.float64).cpu().numpy()
    pre = rec_ref * rg + mn
    m1 = mask == 1
    assert rel(dec[:, ~m1], pre[:, ~m1]) < TOL32
    # int columns: trunc() of a float32-accurate value equals trunc() of the exact one unless the value sits within its own
    # rounding error of an integer; those cells (a handful) may flip by one, every other cell must match exactly
    edge = np.abs(pre[:, m1] - np.round(pre[:, m1])) < 1e-4 * np.maximum(1.0, np.abs(pre[:, m1]))
    got_i, want_i = dec[:, m1], np.trunc(pre[:, m1])
    assert np.array_equal(got_i[~edge], want_i[~edge]) and np.all(np.abs(got_i[edge] - want_i[edge]) <= 1.0) and edge.mean() < 0.05


@pytest.mark.parametrize("n", [1, 17, 100, 1037])
def test_exafel_625_7_fused_vs_oracle(n):
    """CFD_dense_AE(625, 7) -- the exafel1 / exafel2 configs' 25 x 25 blocks at compression ratio 100
    (exafel1_config.py:14-15,33; data_processing.py:26-34) -- runs on the fused wide-layer kernels: encode, decode and
    forward + loss + backward against the oracle at ragged block counts."""
    dims = orc.ae_dims(625, 7)
    flat = orc.formula_params(dims, 23)
    h, p = make_handle(dims, flat, "fp32")
    assert h.path == "fused"
    x = synth.cfd_field(n + 2, 25, 25)[2:].reshape(n, 625) * 20.0
    z_ref = orc.encode(dims, flat, x)
    for xin in (dev(x, torch.float32), dev(x)):
        assert rel(h.encode(xin, out_dtype=torch.float32).cpu().numpy(), z_ref) < TOL32
    rec_ref = orc.decode(dims, flat, z_ref)
    assert rel(h.decode(dev(z_ref, torch.float32)).cpu().numpy(), rec_ref) < TOL32
    grads = torch.zeros_like(p)
    h.fwd_bwd(dev(x, torch.float32), grads)
    lo, go = orc.fwd_bwd(dims, flat, x)
    gh = grads.cpu().numpy().astype(np.float64)
    assert rel(gh[:-1], go) < TOL32 and abs(gh[-1] - lo) < TOL32 * lo
    # the bf16 mode of the same shape (en1 / de4 on the bf16 MFMA): its own 2e-2 bar
    hb, _ = make_handle(dims, flat, "bf16")
    assert rel_l2(hb.encode(dev(x, torch.float32), out_dtype=torch.float32).cpu().numpy(), z_ref) < 2e-2
    assert rel_l2(hb.decode(dev(z_ref, torch.float32)).cpu().numpy(), rec_ref) < 2e-2


@pytest.mark.parametrize("z", [10, 5, 4, 3, 2])
def test_ae24_other_latents_fused(z, monkeypatch):
    """The 24-column AE at the latent sizes of the other compression ratios (baler.py:117-123: latent = ceil(24 / ratio)) is
    served by the same fused kernels as latent 15: encode / decode, the small-batch step (512 rows), the throughput pair
    (4099 rows on a handle whose small-batch limit is lowered: at the default limit of 12288 rows fp32 summation noise alone
    reaches 1e-5), and bamd_train_step == bamd_fwd_bwd + bamd_adam_step bit for bit."""
    dims = orc.ae_dims(24, z)
    flat = orc.formula_params(dims, 100 + z)
    h, p = make_handle(dims, flat, "fp32")
    assert h.path == "fused"
    x = orc.normalize(synth.cms_rows(4099, row0=11))
    zr = orc.encode(dims, flat, x[:777])
    assert rel(h.encode(dev(x[:777])).cpu().numpy(), zr) < TOL32
    assert rel(h.decode(dev(zr)).cpu().numpy(), orc.decode(dims, flat, zr)) < TOL32
    monkeypatch.setenv("BALER_AMD_LATENCY_ROWS", "1024")
    hp, pp = make_handle(dims, flat, "fp32")
    monkeypatch.delenv("BALER_AMD_LATENCY_ROWS")
    for hh, n in ((h, 512), (hp, 4099)):
        grads = torch.zeros_like(p)
        hh.fwd_bwd(dev(x[:n]), grads)
        lo, go = orc.fwd_bwd(dims, flat, x[:n])
        gh = grads.cpu().numpy().astype(np.float64)
        assert rel(gh[:-1], go) < TOL32 and abs(gh[-1] - lo) < TOL32 * lo, n
    h2, p2 = make_handle(dims, flat, "fp32")
    m1, v1, m2, v2 = (torch.zeros_like(p) for _ in range(4))
    g2 = torch.zeros_like(p)
    h.train_step(dev(x[:512]), p, m1, v1, 1, 1e-3)
    h2.fwd_bwd(dev(x[:512]), g2)
    h2.adam_step(p2, g2, m2, v2, 1, 1e-3)
    assert torch.equal(p, p2)


@pytest.mark.parametrize("n", [1, 15, 64, 65, 1037, 70001])
def test_fp64_register_chain_inference(n, monkeypatch):
    """fp64 mode (the reference's own dtype, models.py:128-136): bamd_encode / bamd_decode / bamd_forward_loss of the 24-column
    AE on the register-chained fp64 kernel (infer64_kernel, v_mfma_f64_16x16x4_f64) against the scalar oracle at 1e-11 and
    against the layer-wise kernels (BALER_AMD_F64_INFER=0), ragged row counts, float32 / float64 rows, fused (un)normalisation."""
    dims = orc.ae_dims(24, 15)
    flat = orc.formula_params(dims, 29)
    raw = synth.cms_rows(n, row0=77)
    full = synth.cms_rows(2048)
    mn, rg = np.minimum(raw.min(0), full.min(0)), np.maximum(raw.max(0), full.max(0)) - np.minimum(raw.min(0), full.min(0))
    xn = (raw - mn) / rg
    feats = dev(np.stack([mn, rg]))
    h, _ = make_handle(dims, flat, "fp64")
    monkeypatch.setenv("BALER_AMD_F64_INFER", "0")
    hl, _ = make_handle(dims, flat, "fp64")          # (the switch is read once per process: checked through the results below)
    z_ref = orc.encode(dims, flat, xn)
    assert rel(h.encode(dev(xn)).cpu().numpy(), z_ref) < TOL64
    assert rel(h.encode(dev(raw), features=feats).cpu().numpy(), z_ref) < TOL64
    assert rel(h.encode(dev(xn, torch.float32), out_dtype=torch.float64).cpu().numpy(), orc.encode(dims, flat, xn.astype(np.float32).astype(np.float64))) < TOL64
    rec_ref = orc.decode(dims, flat, z_ref)
    assert rel(h.decode(dev(z_ref)).cpu().numpy(), rec_ref) < TOL64
    mask = np.array([1 if t == "int" else 0 for t in synth.CMS_TYPE_LIST], dtype=np.uint8)
    dec = h.decode(dev(z_ref), features=feats, int_mask=torch.as_tensor(mask).cuda()).cpu().numpy()
    want = rec_ref * rg + mn
    want[:, mask == 1] = np.trunc(want[:, mask == 1])
    assert np.isclose(dec, want, rtol=1e-10, atol=1e-12).mean() > 0.9999          # a truncation may flip where want sits on an integer
    recon, loss = h.forward_loss(dev(xn))
    assert rel(recon.cpu().numpy(), orc.decode(dims, flat, z_ref)) < TOL64
    loss_ref = float(((orc.decode(dims, flat, z_ref) - xn) ** 2).sum() / 24)
    assert abs(loss.item() - loss_ref) < 1e-11 * max(loss_ref, 1e-300)


def test_wide_512_encoder_vs_oracle():
    dims = orc.ae_dims(512, 6)
    flat = orc.formula_params(dims, 41)
    h, _ = make_handle(dims, flat, "fp32")
    x = synth.wide_rows(300, 512)
    z = orc.encode(dims, flat, x)
    assert rel(h.encode(dev(x, torch.float32)).cpu().numpy(), z) < TOL32
    assert rel(h.encode(dev(x)).cpu().numpy(), z) < TOL32
    # decode runs on the same streamed wide-layer kernel (de4: 200 -> 512)
    assert rel(h.decode(dev(z, torch.float32)).cpu().numpy(), orc.decode(dims, flat, z)) < TOL32


# ---- size-independent properties at BASELINE.json's full single-GPU size --------------------------
def test_full_size_properties():
    n = 1_000_000
    dims = orc.ae_dims(24, 15)
    flat = orc.formula_params(dims, 51)
    h, p = make_handle(dims, flat, "fp32")
    raw = dev(synth.cms_rows(n))
    feats = native.minmax(raw)
    x = native.normalize(raw, feats, torch.float32)
    # (1) encode is row-independent: whole == concatenation of ragged pieces, bit for bit
    z = h.encode(x)
    cut = 333_331
    z2 = torch.cat([h.encode(x[:cut]), h.encode(x[cut:])])
    assert torch.equal(z, z2)
    # (2) deterministic
    assert torch.equal(z, h.encode(x))
    # (3) sampled rows against the oracle
    idx = np.random.default_rng(0).choice(n, size=256, replace=False)
    xs = x[torch.as_tensor(idx).cuda()].cpu().numpy().astype(np.float64)
    assert rel(z[torch.as_tensor(idx).cuda()].cpu().numpy(), orc.encode(dims, flat, xs)) < TOL32
    # (4) loss and gradient are additive over row shards
    g_full, g_a, g_b = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    h.fwd_bwd(x, g_full)
    h.fwd_bwd(x[:cut], g_a)
    h.fwd_bwd(x[cut:], g_b)
    assert rel((g_a + g_b).cpu().numpy(), g_full.cpu().numpy()) < 1e-5
    # (5) forward loss equals the loss slot of fwd_bwd
    _, l = h.forward_loss(x, want_recon=False)
    assert abs(l.item() - float(g_full[-1])) < 1e-5 * l.item()
    # (6) decode(encode(x)) == forward(x)
    recon, _ = h.forward_loss(x[:4096])
    assert rel(h.decode(h.encode(x[:4096])).cpu().numpy(), recon.cpu().numpy()) < 1e-6


def _wide_full_size(shape, n, seed):
    """Size-independent properties of a wide model at SURVEY 8(d)'s full per-GPU size: row offsets beyond 2^32 bytes in the
    wide-layer kernels, sampled rows (first / last tile, either side of every 2^32-byte boundary) against the oracle, whole ==
    concatenation of parts (bit for bit: parts are cut on 128-row boundaries and stay on the same kernels), determinism, loss and
    gradient additive over row shards, forward loss == the loss slot of fwd_bwd."""
    F, Z = shape
    dims = orc.ae_dims(F, Z)
    flat = orc.formula_params(dims, seed)
    h, p = make_handle(dims, flat, "fp32")
    assert h.path == "fused"
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand((n, F), dtype=torch.float32, device="cuda", generator=gen)
    row_bytes = F * 4
    idx = {0, 1, 15, 16, n - 17, n - 16, n - 1, n // 2 + 7}
    for k in range(1, int(n * row_bytes >> 32) + 1):          # the rows either side of each 4-GiB boundary
        r = (k << 32) // row_bytes
        idx.update({r - 1, r, r + 1})
    idx = torch.as_tensor(sorted(i for i in idx if 0 <= i < n), device="cuda")
    xs = x[idx].cpu().numpy().astype(np.float64)
    # encode
    z = h.encode(x)
    assert rel(z[idx].cpu().numpy(), orc.encode(dims, flat, xs)) < TOL32
    assert torch.equal(z, h.encode(x))
    cut = (n // 3) & ~127
    assert cut >= 65536
    assert torch.equal(z, torch.cat([h.encode(x[:cut]), h.encode(x[cut:])]))
    assert torch.equal(z[idx], h.encode(x[idx].contiguous())) or rel(z[idx].cpu().numpy(), h.encode(x[idx].contiguous()).cpu().numpy()) < 2e-6
    # decode (the output is the n x F array: its store offsets pass 2^32 as well)
    d = h.decode(z)
    assert rel(d[idx].cpu().numpy(), orc.decode(dims, flat, z[idx].cpu().numpy().astype(np.float64))) < TOL32
    assert torch.equal(d[cut:], h.decode(z[cut:].contiguous()))
    assert bool(torch.isfinite(d).all())
    # forward + loss, and the training pass
    rec, loss = h.forward_loss(x)
    assert rel(rec[idx].cpu().numpy(), orc.forward(dims, flat, xs)) < TOL32
    del rec, d
    torch.cuda.empty_cache()
    g_full, g_a, g_b = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    h.fwd_bwd(x, g_full)
    assert abs(loss.item() - float(g_full[-1])) < 1e-5 * loss.item()
    h.fwd_bwd(x[:cut], g_a)
    h.fwd_bwd(x[cut:], g_b)
    assert rel((g_a.double() + g_b.double()).cpu().numpy(), g_full.cpu().numpy()) < 1e-5
    g2 = torch.zeros_like(p)
    h.fwd_bwd(x, g2)
    assert torch.equal(g2, g_full)                      # fixed-order reductions: bitwise reproducible
    # a small slice against the oracle: the same kernels, so the full-size sums above are sums of THESE per-row terms
    lo, go = orc.fwd_bwd(dims, flat, xs)
    gs = torch.zeros_like(p)
    h.fwd_bwd(x[idx].contiguous(), gs)
    gh = gs.cpu().numpy().astype(np.float64)
    assert rel(gh[:-1], go) < TOL32 and abs(gh[-1] - lo) < TOL32 * lo
    h.close()
    del x, z
    torch.cuda.empty_cache()


def test_c4_full_size_properties():
    """BASELINE configs[3] at SURVEY 8(d)'s throughput size: CFD_dense_AE(2500, 25), 262,144 frames = 2.6 GB of float32."""
    _wide_full_size((2500, 25), 262_144, 61)


def test_c5_full_size_properties():
    """BASELINE configs[4] at ONE GPU's share: the 512-column model, 4,194,304 rows x 512 float32 = 8.6 GB -- row offsets cross
    2^32 bytes twice in the wide kernels' loads (encode, training) and stores (decode, forward)."""
    _wide_full_size((512, 6), 4_194_304, 62)


def test_c3_shard_size_properties():
    """BASELINE configs[2] (100 M rows over 8 GPUs) at ONE rank's size: 12.5 M rows = 2.4 GB of float64 resident on one GPU
    (the 8-GPU run itself needs an 8-GPU node).  Size-independent properties: training and encode over the shard equal the
    sums / concatenations over its quarters, and sampled rows match the oracle; row offsets pass 2^31 bytes several times over."""
    n = 12_500_000
    dims = orc.ae_dims(24, 15)
    flat = orc.formula_params(dims, 77)
    h, p = make_handle(dims, flat, "fp32")
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand((n, 24), dtype=torch.float64, device="cuda", generator=gen)
    g_full = torch.zeros_like(p)
    h.fwd_bwd(x, g_full)
    parts = torch.zeros_like(p, dtype=torch.float64)
    q = n // 4
    for k in range(4):
        g = torch.zeros_like(p)
        h.fwd_bwd(x[k * q:(k + 1) * q], g)
        parts += g.double()
    assert rel(parts.cpu().numpy(), g_full.cpu().numpy()) < 1e-5
    z = h.encode(x, out_dtype=torch.float32)
    zq = h.encode(x[3 * q:], out_dtype=torch.float32)
    assert torch.equal(z[3 * q:], zq)
    idx = torch.as_tensor(np.random.default_rng(1).choice(n, size=128, replace=False)).cuda()
    assert rel(z[idx].cpu().numpy(), orc.encode(dims, flat, x[idx].cpu().numpy())) < TOL32
    # the same shard through the bf16 training kernels: additive too, and within the bf16 bar of the fp32 gradient
    hb, pb = make_handle(dims, flat, "bf16")
    gb = torch.zeros_like(pb)
    hb.fwd_bwd(x, gb)
    assert rel_l2(gb.cpu().numpy()[:-1], g_full.cpu().numpy()[:-1]) < 2e-2
    assert abs(float(gb[-1]) - float(g_full[-1])) < 2e-3 * float(g_full[-1])


@pytest.mark.parametrize("z", [6, 8, 12])
def test_other_latent_sizes_fused(z, data10k):
    """The fused kernels are instantiated for the usual CMS compression ratios (latent 15, 12, 8, 6)."""
    dims = orc.ae_dims(24, z)
    flat = orc.formula_params(dims, 60 + z)
    h, p = make_handle(dims, flat, "fp32")
    x = data10k[:777]
    zz = orc.encode(dims, flat, x)
    assert rel(h.encode(dev(x)).cpu().numpy(), zz) < TOL32
    assert rel(h.decode(dev(zz)).cpu().numpy(), orc.decode(dims, flat, zz)) < TOL32
    grads = torch.zeros_like(p)
    h.fwd_bwd(dev(x), grads)
    lo, go = orc.fwd_bwd(dims, flat, x)
    gh = grads.cpu().numpy().astype(np.float64)
    assert rel(gh[:-1], go) < TOL32 and abs(gh[-1] - lo) < TOL32 * lo
    # and the generic layer-wise path agrees with the fused one (independent implementations)
    import os
    os.environ["BALER_AMD_FORCE_GENERIC"] = "1"
    try:
        hg, pg = make_handle(dims, flat, "fp32")
        gg = torch.zeros_like(pg)
        hg.fwd_bwd(dev(x), gg)
    finally:
        del os.environ["BALER_AMD_FORCE_GENERIC"]
    # two float32 implementations with different summation orders: the fused one within 1e-5 of the oracle in L2 and max-norm (above),
    # the layer-wise one (split-K partial sums) 1e-5 in L2 and 1.3e-5 in the max-norm; 2e-5 between them
    assert rel_l2(gg.cpu().numpy()[:-1], go) < TOL32 and maxerr(gg.cpu().numpy()[:-1], go) < 2e-5 and rel(gg.cpu().numpy(), grads.cpu().numpy()) < 2e-5


@pytest.mark.parametrize("F,Z", [(16, 4), (25, 10), (30, 8), (31, 15), (17, 1), (20, 15), (7, 3), (1, 1)])
def test_any_narrow_table_runs_fused(F, Z):
    """models.py:122-139 builds AE(n_features, z_dim) for ANY column count and baler.py:117-123 derives any latent: every table of
    up to 31 columns with a latent of at most 15 runs on the fused kernels through ONE class instantiation with run-time widths
    (Impl<31, 15, true>: same tile counts as the 24-column model) -- encode, decode (+ fused un-normalisation and int truncation),
    forward + loss, the training pass on both paths (small-batch kernels, throughput pair) and the one-call step, float32 and float64
    rows, normalise-on-load, ragged row counts, against the fp64 oracle at the fp32 bar and against the layer-wise kernels."""
    dims = orc.ae_dims(F, Z)
    flat = orc.formula_params(dims, 100 + F)
    h, p = make_handle(dims, flat, "fp32")
    assert h.path == "fused"
    rng = np.random.default_rng(F * 100 + Z)
    for n in (1, 17, 333, 4099):
        x = rng.random((n, F))
        z_ref = orc.encode(dims, flat, x)
        for xin in (dev(x), dev(x, torch.float32)):
            want = z_ref if xin.dtype == torch.float64 else orc.encode(dims, flat, x.astype(np.float32).astype(np.float64))
            assert rel(h.encode(xin).cpu().numpy(), want) < TOL32, (n, xin.dtype)
        rec_ref = orc.decode(dims, flat, z_ref)
        assert rel(h.decode(dev(z_ref)).cpu().numpy(), rec_ref) < TOL32
        recon, loss = h.forward_loss(dev(x))
        fw = orc.forward(dims, flat, x)
        assert rel(recon.cpu().numpy(), fw) < TOL32 and abs(loss.item() - orc.loss(x, fw)) < TOL32 * loss.item()
    # normalise-on-load and un-normalise + truncation on store
    raw = rng.normal(size=(777, F)) * 50 + 7
    mn, rg = raw.min(0), raw.max(0) - raw.min(0)
    feats = dev(np.stack([mn, rg]))
    xn = (raw - mn) / rg
    zn = orc.encode(dims, flat, xn)
    assert rel(h.encode(dev(raw), features=feats).cpu().numpy(), zn) < TOL32
    mask = np.zeros(F, dtype=np.uint8)
    mask[::3] = 1
    out = h.decode(dev(zn), features=feats, int_mask=dev(mask), out_dtype=torch.float64).cpu().numpy()
    pre = orc.decode(dims, flat, zn) * rg + mn
    m1 = mask == 1
    assert rel(out[:, ~m1], pre[:, ~m1]) < TOL32
    edge = np.abs(pre[:, m1] - np.round(pre[:, m1])) < 1e-4 * np.maximum(1.0, np.abs(pre[:, m1]))
    assert np.array_equal(out[:, m1][~edge], np.trunc(pre[:, m1])[~edge])
    # training: small-batch kernels (<= 12288 rows) and the throughput pair
    for n in (1, 100, 513, 20000):
        x = rng.random((n, F))
        lo, go = orc.fwd_bwd(dims, flat, x)
        grads = torch.full_like(p, 3.0)
        h.fwd_bwd(dev(x), grads)
        gh = grads.cpu().numpy().astype(np.float64)
        assert rel(gh[:-1], go) < TOL32 and abs(gh[-1] - lo) < TOL32 * lo, n
        # per tensor too, up to the reference's batch size (at 20,000 uniform rows single tensors are sums of 20,000 cancelling float32
        # terms: 1e-5 .. 3e-5 on en1 / en2.weight; the whole vector holds 1e-5)
        if n <= 513:
            gt.assert_per_tensor(gh[:-1], go, dims, TOL32, f"AE({F}, {Z}) n={n}")
    lo2, go2 = orc.fwd_bwd(dims, flat, xn)
    g2 = torch.zeros_like(p)
    h.fwd_bwd(dev(raw), g2, features=feats)
    assert rel(g2.cpu().numpy().astype(np.float64)[:-1], go2) < TOL32
    # the one-call step == fwd_bwd + adam_step bit for bit, and it refreshes the packed weights
    x = rng.random((512, F))
    m1_, v1_, m2_, v2_ = (torch.zeros_like(p) for _ in range(4))
    p1, p2 = p.clone(), p.clone()
    h1, _ = make_handle(dims, flat, "fp32")
    h1.train_step(dev(x), p1, m1_, v1_, 1, 1e-3)
    g = torch.zeros_like(p)
    h.fwd_bwd(dev(x), g)
    h.adam_step(p2, g, m2_, v2_, 1, 1e-3)
    assert torch.equal(p1[:-1], p2[:-1]) and torch.equal(m1_[:-1], m2_[:-1])
    st = orc.FitState(dims, flat)
    _, g_o = orc.fwd_bwd(dims, flat, x)
    orc.adam_step(st.params, g_o, st.m, st.v, 1, 1e-3)
    # (rel-L2: the first Adam step moves a parameter by lr g / (|g| + eps) -- where |g| ~ eps a float32 gradient's last bits decide
    # the step of that one element, a max-norm bar would be measuring eps, not the kernels)
    assert rel_l2(p1.cpu().numpy().astype(np.float64)[:-1], st.params) < TOL32
    assert rel(h1.encode(dev(x)).cpu().numpy(), orc.encode(dims, st.params, x)) < 2 * TOL32


@pytest.mark.parametrize("F,Z,path", [(48, 12, "fused"), (33, 8, "fused"), (24, 16, "fused"), (63, 31, "fused"), (31, 31, "fused"),
                                      (32, 1, "fused"), (47, 15, "fused"), (47, 31, "fused"), (40, 20, "fused"), (63, 15, "fused"),
                                      (64, 16, "fused"), (79, 31, "fused"), (80, 8, "fused"), (63, 32, "fused"), (40, 40, "generic")])
def test_wider_narrow_tables_say_where_they_run(F, Z, path):
    """Up to 63 columns with a latent of up to 31: full class instantiations (every kernel; the 63-column class reads its bias
    fragments from L2 because images + biases would need 164 KB of LDS).  64..79 columns: encode / decode / forward + loss on the
    one-tile fused kernels, training on the small-batch kernels up to 12288 rows (two recon tiles per wave in the chain) and
    layer by layer beyond -- round 5: the same up to 127 columns for the small batches, with the run-time-width wide class as the handle's
    first state for inference and larger batches ("fused"); 48 .. 4096 columns with a latent of up to 63 that no narrow class takes:
    the wide class alone (tests/test_gpu_wide_class.py); anything else layer by layer.  Correct either way, and
    bamd_path_of says which."""
    dims = orc.ae_dims(F, Z)
    flat = orc.formula_params(dims, 7)
    h, p = make_handle(dims, flat, "fp32")
    assert h.path == path
    for n in (1, 37, 300, 4099):
        x = np.random.default_rng(n).random((n, F))
        z_ref = orc.encode(dims, flat, x)
        for xin in (dev(x), dev(x, torch.float32)):
            assert rel(h.encode(xin).cpu().numpy(), z_ref) < TOL32, (F, Z, n)
        assert rel(h.decode(dev(z_ref)).cpu().numpy(), orc.decode(dims, flat, z_ref)) < TOL32, (F, Z, n)
        recon, loss = h.forward_loss(dev(x))
        want = orc.forward(dims, flat, x)
        assert rel(recon.cpu().numpy(), want) < TOL32
        assert abs(loss.item() - ((want - x) ** 2).sum() / F) < TOL32 * max(1.0, ((want - x) ** 2).sum() / F)
    # fused (un)normalisation and the int mask through the class kernels
    raw = np.random.default_rng(3).uniform(-40, 90, size=(257, F))
    feats = orc.find_minmax(raw)
    z1 = h.encode(dev(raw), features=dev(feats)).cpu().numpy()
    assert rel(z1, orc.encode(dims, flat, orc.normalize(raw))) < TOL32
    mask = np.zeros(F, dtype=np.uint8)
    mask[[0, F - 1]] = 1
    out = h.decode(dev(z1), features=dev(feats), int_mask=dev(mask)).cpu().numpy()
    want = orc.renormalize(orc.decode(dims, flat, z1.astype(np.float64)), feats[0], feats[1])
    cols = mask == 0
    assert rel(out[:, cols], want[:, cols]) < TOL32
    assert np.mean(out[:, ~cols] == np.trunc(want[:, ~cols])) > 0.99
    # training behind the same entry points: the small-batch kernels up to 12288 rows (1 .. 513 rows: ragged 16-row blocks;
    # 12288 / 12289: either side of the switch), the throughput pair or the layer-wise kernels beyond; the fused copy of the
    # parameters follows the optimiser step
    for n in (1, 300, 513, 12288, 12289, 20001):
        x = off_the_kink(dims, flat, n, seed=n)
        lo, go = orc.fwd_bwd(dims, flat, x)
        grads = torch.zeros_like(p)
        h.fwd_bwd(dev(x), grads)
        gh = grads.cpu().numpy().astype(np.float64)
        assert rel_l2(gh[:-1], go) < 1e-5 and np.abs(gh[:-1] - go).max() < 2e-5 * np.abs(go).max(), (F, Z, n)
        assert abs(gh[-1] - lo) < TOL32 * lo
    x = np.random.default_rng(1).random((300, F))
    lo, go = orc.fwd_bwd(dims, flat, x)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    h.train_step(dev(x), p, m, v, 1, 1e-3)
    st = orc.FitState(dims, flat)
    orc.adam_step(st.params, go, st.m, st.v, 1, 1e-3)
    assert rel_l2(p.cpu().numpy().astype(np.float64)[:-1], st.params) < TOL32
    assert rel(h.encode(dev(x)).cpu().numpy(), orc.encode(dims, st.params, x)) < 2 * TOL32      # the fused copy follows the step


@pytest.mark.parametrize("z,n", [(15, 130), (15, 2048), (15, 5003), (6, 20000)])
def test_layer_wise_training_short_side_weight_gradients(z, n, data10k, monkeypatch):
    """Layer-wise float32 training pass (>= 128 rows): the weight gradients run on the short-side kernels (1, 2, 4, 7 and 13
    tiles on the short side, ones column on either side, ragged last block) -- against the oracle and against the LDS-tiled
    GEMM path (BALER_AMD_SHORT_DW=0)."""
    dims = orc.ae_dims(24, z)
    flat = orc.formula_params(dims, 31)
    x = np.concatenate([data10k, data10k[::-1] * 0.5])[:n]
    monkeypatch.setenv("BALER_AMD_FORCE_GENERIC", "1")
    h, p = make_handle(dims, flat, "fp32")
    monkeypatch.delenv("BALER_AMD_FORCE_GENERIC")
    lo, go = orc.fwd_bwd(dims, flat, x)
    grads = torch.zeros_like(p)
    h.fwd_bwd(dev(x), grads)
    gh = grads.cpu().numpy().astype(np.float64)
    assert rel(gh[:-1], go) < TOL32 and abs(gh[-1] - lo) < TOL32 * lo
    monkeypatch.setenv("BALER_AMD_SHORT_DW", "0")
    g2 = torch.zeros_like(p)
    h.fwd_bwd(dev(x), g2)
    assert rel(g2.cpu().numpy(), grads.cpu().numpy()) < 1e-5


@pytest.mark.parametrize("shape,n", [((2500, 25), 1), ((2500, 25), 17), ((2500, 25), 300), ((2500, 25), 1037), ((2500, 25), 2100), ((512, 6), 65),
                                     ((512, 6), 1000), ((512, 6), 4099)])
def test_wide_training_pass_vs_oracle(shape, n, monkeypatch):
    """Training pass of the wide models: forward + loss + input-gradient chain on the two fused wide-layer launches, weight
    gradients as split-K GEMMs -- loss and every gradient against the oracle and against the all-layer-wise pass
    (BALER_AMD_WIDE_TRAIN=0), float32 rows in place, float64 rows and normalise-on-load through the staging copy."""
    dims = orc.ae_dims(*shape)
    flat = orc.formula_params(dims, 23)
    h, p = make_handle(dims, flat, "fp32")
    rng = np.random.default_rng(n)
    x = rng.random((n, shape[0]))
    lo, go = orc.fwd_bwd(dims, flat, x)
    grads = torch.zeros_like(p)
    for xin in (dev(x, torch.float32), dev(x)):
        grads.fill_(7.0)
        h.fwd_bwd(xin, grads)
        gh = grads.cpu().numpy().astype(np.float64)
        assert rel(gh[:-1], go) < TOL32 and abs(gh[-1] - lo) < TOL32 * lo, xin.dtype
    monkeypatch.setenv("BALER_AMD_WIDE_TRAIN", "0")
    gl = torch.zeros_like(p)
    h.fwd_bwd(dev(x), gl)
    monkeypatch.delenv("BALER_AMD_WIDE_TRAIN")
    assert rel(gl.cpu().numpy(), grads.cpu().numpy()) < 1e-5
    mn, rg = x.min(0) - 0.5, x.max(0) - x.min(0) + 1.0
    lo2, go2 = orc.fwd_bwd(dims, flat, (x - mn) / rg)
    h.fwd_bwd(dev(x), grads, features=dev(np.stack([mn, rg])))
    gh = grads.cpu().numpy().astype(np.float64)
    assert rel(gh[:-1], go2) < 2e-5 and abs(gh[-1] - lo2) < 2e-5 * lo2


@pytest.mark.parametrize("shape,n", [((2500, 25), 1), ((2500, 25), 333), ((2500, 25), 70001), ((512, 6), 1000)])
def test_wide_validation_pass_vs_oracle(shape, n):
    """forward_loss (training.py:104-137) of the wide models on the fused forward kernel: loss and reconstruction, float32 and
    float64 rows, normalise-on-load, several 65536-row chunks."""
    dims = orc.ae_dims(*shape)
    flat = orc.formula_params(dims, 29)
    h, _ = make_handle(dims, flat, "fp32")
    rng = np.random.default_rng(n)
    x = rng.random((n, shape[0])).astype(np.float32).astype(np.float64)
    m = min(n, 2000)                                   # the oracle on a head and a tail slice; the loss on all rows
    rec_ref = np.concatenate([orc.forward(dims, flat, x[:m]), orc.forward(dims, flat, x[-m:])])
    for xin in (dev(x, torch.float32), dev(x)):
        rec, loss = h.forward_loss(xin)
        r = rec.cpu().numpy().astype(np.float64)
        assert rel(np.concatenate([r[:m], r[-m:]]), rec_ref) < TOL32
        want = ((r - x) ** 2).sum() / shape[0]
        assert abs(loss.item() - want) < 1e-5 * want
    _, loss2 = h.forward_loss(dev(x, torch.float32), want_recon=False)
    assert abs(loss2.item() - want) < 1e-5 * want
    mn, rg = x.min(0) - 0.5, x.max(0) - x.min(0) + 1.0
    rec3, loss3 = h.forward_loss(dev(x[:m]), features=dev(np.stack([mn, rg])))
    xn = (x[:m] - mn) / rg
    assert rel(rec3.cpu().numpy(), orc.forward(dims, flat, xn)) < 2e-5
    assert abs(loss3.item() - orc.loss(xn, orc.forward(dims, flat, xn))) < 2e-5 * loss3.item()


@pytest.mark.parametrize("shape,n", [((2500, 25), 1), ((2500, 25), 31), ((2500, 25), 33), ((2500, 25), 1000), ((512, 6), 17), ((512, 6), 70000)])
def test_wide_encode_two_row_tiles_per_wave(shape, n, monkeypatch):
    """The two-tile encode kernel of the wide models (taken from 65536 rows on; forced here) against the one-tile kernel (same
    fragments; the one-tile chain interleaves the steps of fragment pairs, so a one-tile-wide layer sums in another order) and
    within 1e-5 of the oracle, ragged pair counts, float32 / float64 rows."""
    dims = orc.ae_dims(*shape)
    flat = orc.formula_params(dims, 37)
    h, _ = make_handle(dims, flat, "fp32")
    x = np.random.default_rng(n).random((n, shape[0]))
    m = min(n, 1500)
    for xin in (dev(x, torch.float32), dev(x)):
        monkeypatch.setenv("BALER_AMD_WIDE2", "1")
        z2 = h.encode(xin, out_dtype=torch.float32)
        monkeypatch.setenv("BALER_AMD_WIDE2", "0")
        z1 = h.encode(xin, out_dtype=torch.float32)
        assert rel(z1.cpu().numpy(), z2.cpu().numpy()) < 2e-6
        assert rel(z2[:m].cpu().numpy(), orc.encode(dims, flat, x[:m].astype(np.float32 if xin.dtype == torch.float32 else np.float64))) < TOL32


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_wide_512_fused_encode_ragged(dtype):
    """Encode of the 512-column model runs on the fused register chain (vector row loads); decode/train on the
    generic path: both against the oracle, ragged row count, fp32 and fp64 rows, fused normalisation."""
    dims = orc.ae_dims(512, 6)
    flat = orc.formula_params(dims, 42)
    h, p = make_handle(dims, flat, "fp32")
    raw = synth.wide_rows(1003, 512) * 3.0 + 1.0
    xn = orc.normalize(raw)
    z = h.encode(dev(xn, dtype))
    assert rel(z.cpu().numpy(), orc.encode(dims, flat, xn)) < TOL32
    feats = native.minmax(dev(raw, dtype))
    z2 = h.encode(dev(raw, dtype), features=feats)
    assert rel(z2.cpu().numpy(), orc.encode(dims, flat, xn)) < (TOL32 if dtype == torch.float64 else 1e-4)
    zz = orc.encode(dims, flat, xn)
    assert rel(h.decode(dev(zz, dtype)).cpu().numpy(), orc.decode(dims, flat, zz)) < TOL32
    grads = torch.zeros_like(p)
    h.fwd_bwd(dev(xn[:200], dtype), grads)
    lo, go = orc.fwd_bwd(dims, flat, xn[:200])
    assert rel(grads.cpu().numpy().astype(np.float64)[:-1], go) < TOL32


def test_abi_error_paths():
    """Errors are negative statuses with a message, never exceptions across the ABI."""
    import ctypes
    L = native.lib()
    h = ctypes.c_void_p()
    dims = (ctypes.c_int * 9)(24, 200, 100, 50, 15, 50, 100, 200, 24)
    assert L.bamd_create(dims, 7, 0, 0, ctypes.byref(h)) == -1 and b"even" in L.bamd_last_error()
    assert L.bamd_create(dims, 8, 9, 0, ctypes.byref(h)) == -1
    other = (ctypes.c_int * 9)(100, 200, 100, 50, 10, 50, 100, 200, 100)
    # BAMD_MODE_BF16 of a shape without bf16 kernels is not an error: a float32 handle (notice on stderr), and the ABI says so
    assert L.bamd_create(other, 8, native.MODE_BF16, 0, ctypes.byref(h)) == 0 and L.bamd_mode_of(h) == native.MODE_F32
    L.bamd_destroy(h)
    # the data-parallel entry points without a communicator / with bad arguments
    assert L.bamd_comm_world(None) == 0 and L.bamd_comm_init(None, None, 0, 1) == -1
    assert L.bamd_create(dims, 8, 0, 99, ctypes.byref(h)) == -1
    bad = (ctypes.c_int * 9)(24, 200, 0, 50, 15, 50, 100, 200, 24)
    assert L.bamd_create(bad, 8, 0, 0, ctypes.byref(h)) == -1
    assert L.bamd_create(dims, 8, 0, 0, ctypes.byref(h)) == 0
    x = torch.zeros((4, 24), dtype=torch.float32, device="cuda")
    z = torch.zeros((4, 15), dtype=torch.float32, device="cuda")
    rc = L.bamd_encode(h, ctypes.c_void_p(x.data_ptr()), 0, 4, None, ctypes.c_void_p(z.data_ptr()), 0, None)
    assert rc == -1 and b"bamd_load_params" in L.bamd_last_error()      # parameters not loaded yet
    assert L.bamd_comm_world(h) == 0
    assert L.bamd_allreduce_sum(h, ctypes.c_void_p(x.data_ptr()), 0, 4, None) == -1 and b"communicator" in L.bamd_last_error()
    L.bamd_destroy(h)
    with pytest.raises(native.NativeError):
        make_handle(orc.ae_dims(24, 15), orc.formula_params(orc.ae_dims(24, 15), 1), "fp32")[0].encode(torch.zeros(4, 24))


@pytest.mark.parametrize("n", [16, 37, 512, 4096, 5000, 20000])
@pytest.mark.parametrize("mode", ["fp32", "fp64"])
def test_train_step_equals_fwd_bwd_then_adam(n, mode):
    """bamd_train_step (training.py:64-97 in one call) == bamd_fwd_bwd + bamd_adam_step, bit for bit, on the
    small-batch kernels (n <= 12288: Adam fused into the weight-gradient tiles), the throughput kernels and the
    generic fp64 path; and both follow the oracle's fit loop."""
    dims = orc.ae_dims(24, 15)
    p0 = orc.formula_params(dims, 11)
    x = orc.normalize(synth.cms_rows(n, row0=7))
    dt = torch.float32 if mode == "fp32" else torch.float64
    xd = torch.from_numpy(x).cuda()
    runs = []
    for fused in (False, True):
        h, flat = make_handle(dims, p0, mode)
        m, v = torch.zeros_like(flat), torch.zeros_like(flat)
        grads = torch.zeros(h.nparams + 1, dtype=dt, device="cuda")
        la = torch.zeros(1, dtype=torch.float64, device="cuda")
        for t in range(1, 5):
            if fused:
                h.train_step(xd, flat, m, v, t, 1e-3, loss_accum=la, grads=grads if t % 2 else None)
            else:
                h.fwd_bwd(xd, grads)
                h.adam_step(flat, grads, m, v, t, 1e-3, loss_accum=la)
        runs.append((flat.clone(), m.clone(), v.clone(), la.item(), h.encode(xd)))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b
    # oracle: four Adam steps on the same batch
    p = p0.copy(); mo = np.zeros_like(p); vo = np.zeros_like(p); tot = 0.0
    for t in range(1, 5):
        loss, g = orc.fwd_bwd(dims, p, x)
        tot += loss
        orc.adam_step(p, g, mo, vo, t, 1e-3)
    got = runs[1][0][:h.nparams].double().cpu().numpy()
    tol = 1e-5 if mode == "fp32" else 1e-11
    assert abs(runs[1][3] - tot) <= tol * tot
    # parameters: Adam's update lr*m/(sqrt(v)+eps) is scale-free, so a component whose gradient is ~1e-7 of the
    # largest one (fp32 rounding level) moves by a full +-lr whatever its sign: after 4 steps the fp32 parameters sit
    # within a few 1e-6 absolute of the fp64 oracle (measured 6.3e-6 at n=5000), i.e. 1e-4 of max|p|; the gradient
    # itself is pinned at 1e-5 by test_gradients_golden / test_gradients_ragged above
    ptol = 1e-4 if mode == "fp32" else 1e-11
    assert np.abs(got - p).max() <= ptol * np.abs(p).max()


# ---- bf16 inference mode (BAMD_MODE_BF16): a throughput mode with its own, looser bar -----------------------------
BF16_TOL = 2e-2    # measured on the trained C1 model: encode 1.9e-3, decode 6.4e-3, forward 8.2e-3 rel-L2 (8-bit significands)


@pytest.mark.parametrize("z_dim", [15, 12, 8, 6])
def test_bf16_mode_encode_decode_forward(z_dim, data10k):
    """bf16 MFMA inference (LDS-resident weights) against the fp64 oracle at the bf16 bar; the fp32 mode stays the
    parity mode.  I/O dtypes, fused (de)normalisation, int truncation and ragged sizes behave like the fp32 kernels."""
    dims = orc.ae_dims(24, z_dim)
    flat = orc.formula_params(dims, 41 + z_dim)
    h, _ = make_handle(dims, flat, "bf16")
    assert h.param_dtype == torch.float32
    x = data10k[:3001]
    zo = orc.encode(dims, flat, x)
    for dt in (torch.float64, torch.float32):
        z = h.encode(dev(x, dt))
        assert z.dtype == dt and rel(z.cpu().numpy(), zo) < BF16_TOL
        d = h.decode(dev(zo, dt))
        assert rel_l2(d.cpu().numpy(), orc.decode(dims, flat, zo)) < BF16_TOL
    recon, loss = h.forward_loss(dev(x))
    ro = orc.decode(dims, flat, zo)
    assert rel_l2(recon.cpu().numpy(), ro) < BF16_TOL
    assert abs(loss.item() - ((ro - x) ** 2).sum() / 24) < BF16_TOL * ((ro - x) ** 2).sum() / 24
    _, loss2 = h.forward_loss(dev(x), want_recon=False)
    assert loss2.item() == loss.item()                                  # reproducible, with or without the recon store
    for n in (1, 15, 16, 17, 63, 64, 65, 511, 513):
        assert rel_l2(h.encode(dev(x[:n])).cpu().numpy(), zo[:n]) < BF16_TOL
    assert h.encode(dev(x[:0])).shape == (0, z_dim)
    # fused normalisation on load, un-normalisation + int truncation on store
    raw = synth.cms_rows(3001)
    feats = orc.find_minmax(raw)
    zn = h.encode(dev(raw), features=dev(feats))
    assert rel_l2(zn.cpu().numpy(), orc.encode(dims, flat, orc.normalize(raw))) < BF16_TOL
    mask = np.array([t == "int" for t in synth.CMS_TYPE_LIST], dtype=np.uint8)
    out = h.decode(dev(zo), features=dev(feats), int_mask=torch.from_numpy(mask).cuda()).cpu().numpy()
    want = orc.renormalize(orc.decode(dims, flat, zo), feats[0], feats[1])
    fl = mask == 0
    assert rel_l2(out[:, fl], want[:, fl]) < BF16_TOL
    assert np.array_equal(out[:, ~fl], np.trunc(out[:, ~fl]))


@pytest.mark.parametrize("kernels", ["bf16", "fp32-layerwise"])
def test_bf16_mode_training_calls(data10k, kernels, monkeypatch):
    """Training entry points of a bf16 handle: the bf16 MFMA training kernels (their own 2e-2 bar, tests/test_gpu_bf16_train.py),
    or -- with BALER_AMD_BF16_TRAIN=0 (read at bamd_create), and for shapes without an instantiation -- the fp32 layer-wise
    kernels (1e-5 bar).  Either way the optimiser step reaches the packed bf16 weights that inference uses."""
    if kernels == "fp32-layerwise":
        monkeypatch.setenv("BALER_AMD_BF16_TRAIN", "0")
    dims = orc.ae_dims(24, 15)
    flat = orc.formula_params(dims, 9)
    h, p = make_handle(dims, flat, "bf16")
    x = data10k[:700]
    grads = torch.zeros_like(p)
    h.fwd_bwd(dev(x, torch.float64), grads)
    lo, go = orc.fwd_bwd(dims, flat, x)
    assert (rel_l2(grads.cpu().numpy()[:-1], go) < BF16_TOL) if kernels == "bf16" else (rel(grads.cpu().numpy()[:-1], go) < TOL32)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    z0 = h.encode(dev(x))
    h.adam_step(p, grads, m, v, 1, 1e-2)
    z1 = h.encode(dev(x))
    assert not torch.equal(z0, z1)                                       # the step reached the packed bf16 weights
    assert rel_l2(z1.cpu().numpy(), orc.encode(dims, p.cpu().numpy().astype(np.float64)[:-1], x)) < BF16_TOL


@pytest.mark.parametrize("n", [12288, 12289])
def test_small_batch_threshold_boundary(n):
    """12288 rows is the last batch size on the small-batch kernels, 12289 the first on the throughput pair: same
    gradient (1e-5 of the oracle, and of each other at fp32 rounding level)."""
    dims = orc.ae_dims(24, 15)
    flat = orc.formula_params(dims, 13)
    x = orc.normalize(synth.cms_rows(n, row0=3))
    h, p = make_handle(dims, flat, "fp32")
    grads = torch.zeros_like(p)
    h.fwd_bwd(dev(x), grads)
    lo, go = orc.fwd_bwd(dims, flat, x)
    gh = grads.cpu().numpy().astype(np.float64)
    assert rel(gh[:-1], go) < TOL32 and abs(gh[-1] - lo) < TOL32 * lo


def test_train_step_empty_batch_and_generic_fallback():
    """bamd_train_step with n_rows = 0 (an empty shard) is fwd_bwd's zero gradient + an Adam step; shapes without
    a fused path (CFD_dense_AE) take the fwd_bwd + adam_step route behind the same entry point."""
    dims = orc.ae_dims(24, 15)
    h, p = make_handle(dims, orc.formula_params(dims, 2), "fp32")
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    before = p.clone()
    h.train_step(torch.zeros((0, 24), dtype=torch.float64, device="cuda"), p, m, v, 1, 1e-3)
    assert torch.equal(p, before) and float(m.abs().max()) == 0.0       # zero gradient: Adam moves nothing
    dims2 = [400, 120, 60, 30, 9, 30, 60, 120, 400]     # not the reference's hidden widths: no fused instantiation, the layer-wise kernels
    f2 = orc.formula_params(dims2, 3)
    x = synth.cfd_field(4, 40, 40).reshape(16, 400)
    ha, pa = make_handle(dims2, f2, "fp32")
    assert ha.path == "generic"
    hb, pb = make_handle(dims2, f2, "fp32")
    ma, va, mb_, vb = (torch.zeros_like(pa) for _ in range(4))
    g = torch.zeros_like(pa)
    for t in (1, 2):
        ha.train_step(dev(x, torch.float32), pa, ma, va, t, 1e-3)
        hb.fwd_bwd(dev(x, torch.float32), g)
        hb.adam_step(pb, g, mb_, vb, t, 1e-3)
    assert torch.equal(pa, pb)


@pytest.mark.parametrize("case", ["bf16-wide-layerwise", "bf16-ae24-no-latency", "fp32-ae24-no-latency", "bf16-wide-split"])
def test_train_step_under_routing_knobs(case, monkeypatch):
    """bamd_train_step never returns OK without having stepped: under the documented routing knobs that take a handle off its default
    launches (BALER_AMD_WIDE_TRAIN=0 on a BF16 wide handle: weight gradients on the per-layer launches, no in-kernel Adam;
    BALER_AMD_LATENCY_ROWS=0 on a narrow handle: the throughput pair for every batch) the one-call step equals bamd_fwd_bwd +
    bamd_adam_step bit for bit, the parameters MOVE, and the next encode of a BF16 handle sees the new weights (round-5 advisor
    finding: the precheck and the body of fwd_bwd_T disagreed and the optimiser step was dropped)."""
    if case.startswith("bf16-wide"):
        shape, n, mode = (512, 6), 60, "bf16"
        if case == "bf16-wide-layerwise":
            monkeypatch.setenv("BALER_AMD_WIDE_TRAIN", "0")
    else:
        shape, n, mode = (24, 15), 512, case[:4]
        monkeypatch.setenv("BALER_AMD_LATENCY_ROWS", "0")      # read at bamd_create
    dims = orc.ae_dims(*shape)
    p0 = orc.formula_params(dims, 19)
    x = off_the_kink(dims, p0, n, 5)
    xd = dev(x, torch.float32)
    runs = []
    for one_call in (False, True):
        h, flat = make_handle(dims, p0, mode)
        m, v = torch.zeros_like(flat), torch.zeros_like(flat)
        grads = torch.zeros_like(flat)
        for t in range(1, 4):
            if one_call:
                h.train_step(xd, flat, m, v, t, 1e-2, grads=grads if t % 2 else None)
            else:
                h.fwd_bwd(xd, grads)
                h.adam_step(flat, grads, m, v, t, 1e-2)
        runs.append((flat.clone(), m.clone(), v.clone(), h.encode(xd, out_dtype=torch.float32)))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    got = runs[1][0][:-1].double().cpu().numpy()
    assert np.abs(got - p0).max() > 5e-3                       # three steps of lr 1e-2 moved the parameters
    assert float(runs[1][1].abs().max()) > 0 and float(runs[1][2].abs().max()) > 0
    z_new = orc.encode(dims, got, x)
    assert rel_l2(runs[1][3].cpu().numpy(), z_new) < (BF16_TOL if mode == "bf16" else TOL32)
    assert rel_l2(orc.encode(dims, p0, x), z_new) > 5e-2       # ... by far more than the tolerance the encode is held to


_ROUTE_THRESHOLDS = {
    # handle: dims, mode, activation, (knob, value) that brings the threshold down to a few rows, last row count below it
    "bf16-small-rows": (orc.ae_dims(24, 15), "bf16", "leaky_relu", ("BALER_AMD_BF16_SMALL_ROWS", "64"), 64),   # read per call
    "fpga-f32-rows": ([24, 20, 10, 15, 10, 20, 24], "fp32", "relu", None, 8192),                               # a constant of fpga.hip
    "two-state-latency": (orc.ae_dims(80, 16), "fp32", "leaky_relu", ("BALER_AMD_LATENCY_ROWS", "64"), 64),    # read at bamd_create
}


@pytest.mark.parametrize("above", [False, True], ids=["last-below", "first-above"])
@pytest.mark.parametrize("case", list(_ROUTE_THRESHOLDS))
def test_train_route_agrees_at_every_row_threshold(case, above, monkeypatch):
    """bamd_train_step and bamd_fwd_bwd read ONE training route (api.hip: train_family), so at the row counts either side of every
    threshold at which that route, or a family's decline behind it, changes kernels the one-call step == bamd_fwd_bwd + bamd_adam_step
    bit for bit: a BF16 handle (fp32 small-batch kernels up to BALER_AMD_BF16_SMALL_ROWS rows, the bf16 pair above), an fp32
    FPGA_prototype_model handle (fused up to 8,192 rows, layer-wise above) and a two-state 64..127-column handle (small-batch class up to
    BALER_AMD_LATENCY_ROWS rows, the wide launches above).  The fp32 AE(24, 15) handle's BALER_AMD_LATENCY_ROWS threshold is straddled
    with the same bit equalities by test_train_step_equals_fwd_bwd_then_adam (5,000 and 20,000 rows around 12,288)."""
    dims, mode, act, knob, rows = _ROUTE_THRESHOLDS[case]
    if knob:
        monkeypatch.setenv(*knob)
    n = rows + 1 if above else rows
    p0 = orc.formula_params(dims, 23)
    xd = dev(np.random.default_rng(n).random((n, dims[0])), torch.float32)
    runs = []
    for one_call in (False, True):
        h = native.Handle(dims, mode, act=act)
        flat = dev(np.concatenate([p0, [0.0]]), torch.float32)
        h.load_params(flat)
        m, v, grads = torch.zeros_like(flat), torch.zeros_like(flat), torch.zeros_like(flat)
        for t in range(1, 4):
            if one_call:
                h.train_step(xd, flat, m, v, t, 1e-2, grads=grads if t % 2 else None)
            else:
                h.fwd_bwd(xd, grads)
                h.adam_step(flat, grads, m, v, t, 1e-2)
        runs.append((flat.clone(), m.clone(), v.clone(), h.encode(xd, out_dtype=torch.float32)))
        h.close()
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    assert np.abs(runs[1][0][:-1].double().cpu().numpy() - p0).max() > 5e-3          # three steps of lr 1e-2 moved the parameters


@pytest.mark.parametrize("dims,path", [(orc.ae_dims(100, 10), "fused"), (orc.ae_dims(900, 9), "fused"), (orc.ae_dims(30, 7), "fused"),
                                       ([400, 120, 60, 30, 9, 30, 60, 120, 400], "generic")])
def test_bf16_mode_of_a_shape_without_bf16_kernels_runs_in_fp32(dims, path, capfd):
    """models.py:122-139, 192-209 build AE / CFD_dense_AE(n_features, z_dim) for any width; `BALER_AMD_MODE=bf16` on such a model is a
    slower path, not an error: the handle computes in float32 on whatever serves the shape there (fp32 bar, 1e-5), says so on stderr,
    and bamd_mode_of() reports fp32."""
    flat = orc.formula_params(dims, 23)
    h, p = make_handle(dims, flat, "bf16")
    assert "computes in float32" in capfd.readouterr().err
    assert h.compute_mode == native.MODE_NAMES["fp32"] and h.path == path
    x = off_the_kink(dims, flat, 77, 3)
    z_ref = orc.encode(dims, flat, x)
    assert rel(h.encode(dev(x), out_dtype=torch.float32).cpu().numpy(), z_ref) < TOL32
    assert rel(h.decode(dev(z_ref, torch.float32)).cpu().numpy(), orc.decode(dims, flat, z_ref)) < TOL32
    lo, go = orc.fwd_bwd(dims, flat, x)
    g = torch.zeros_like(p)
    h.fwd_bwd(dev(x), g)
    gh = g.cpu().numpy().astype(np.float64)
    assert rel(gh[:-1], go) < TOL32 and abs(gh[-1] - lo) < TOL32 * lo
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    h.train_step(dev(x), p, m, v, 1, 1e-2)
    pn, mo, vo = flat.copy(), np.zeros_like(flat), np.zeros_like(flat)
    orc.adam_step(pn, go, mo, vo, 1, 1e-2)
    live = np.abs(go) > 1e-6 * np.abs(go).max()
    assert rel((p.cpu().numpy().astype(np.float64)[:-1] - flat)[live], (pn - flat)[live]) < 1e-3
    assert rel(h.encode(dev(x), out_dtype=torch.float32).cpu().numpy(), orc.encode(dims, p.cpu().numpy().astype(np.float64)[:-1], x)) < TOL32


@pytest.mark.parametrize("shape,n", [((2500, 25), 1), ((2500, 25), 33), ((2500, 25), 1000), ((625, 7), 129), ((512, 6), 17), ((512, 6), 4100)])
def test_bf16_mode_wide_models(shape, n, monkeypatch):
    """BAMD_MODE_BF16 on the wide models: en1 / de4 on the bf16 MFMA (HBM-bound kernels), the narrow layers on the fp32 chain;
    bf16-level agreement with the oracle (inputs and the two wide weight matrices are rounded to bf16), ragged pair counts,
    float32 / float64 rows, fused (un)normalisation; training calls of such a handle run en1 / de4 / de4's input-gradient product on
    the bf16 MFMA too (bf16 bar 2e-2; BALER_AMD_BF16_WIDE_TRAIN=0: the fp32 launches, exact) and re-round the bf16 fragments before
    the next encode."""
    dims = orc.ae_dims(*shape)
    flat = orc.formula_params(dims, 41)
    h, p = make_handle(dims, flat, "bf16")
    x = off_the_kink(dims, flat, n, n)          # (the float32 launches below are held to a max-norm bar: rows clear of the LeakyReLU kink)
    z_ref = orc.encode(dims, flat, x)
    for xin in (dev(x, torch.float32), dev(x)):
        assert rel_l2(h.encode(xin, out_dtype=torch.float32).cpu().numpy(), z_ref) < 6e-3
    rec_ref = orc.decode(dims, flat, z_ref)
    for zin in (dev(z_ref, torch.float32), dev(z_ref)):
        assert rel_l2(h.decode(zin).cpu().numpy(), rec_ref) < 6e-3
    mn, rg = x.min(0) - 0.5, x.max(0) - x.min(0) + 1.0
    feats = dev(np.stack([mn, rg]))
    zn = orc.encode(dims, flat, (x - mn) / rg)
    assert rel_l2(h.encode(dev(x), features=feats, out_dtype=torch.float32).cpu().numpy(), zn) < 6e-3
    dec = h.decode(dev(zn, torch.float32), features=feats, out_dtype=torch.float64).cpu().numpy()
    assert rel_l2(dec, orc.decode(dims, flat, zn) * rg + mn) < 6e-3
    # training pass: bf16 wide products (bf16 bar), the fp32 launches behind the switch (exact), then an optimiser step: the next
    # encode must see the new weights
    grads = torch.zeros_like(p)
    lo, go = orc.fwd_bwd(dims, flat, x)
    for xin in (dev(x, torch.float32), dev(x)):
        grads.fill_(7.0)
        h.fwd_bwd(xin, grads)
        gh = grads.cpu().numpy().astype(np.float64)
        # (a single row: one hidden unit whose pre-activation changes sign under bf16 rounding moves whole gradient rows -- LeakyReLU kink)
        assert rel_l2(gh[:-1], go) < (5e-3 if n >= 33 else 1e-1) and abs(gh[-1] - lo) < 1e-3 * lo, xin.dtype
    monkeypatch.setenv("BALER_AMD_BF16_WIDE_TRAIN", "0")
    h.fwd_bwd(dev(x, torch.float32), grads)
    monkeypatch.delenv("BALER_AMD_BF16_WIDE_TRAIN")
    gh = grads.cpu().numpy().astype(np.float64)
    assert rel(gh[:-1], go) < TOL32 and abs(gh[-1] - lo) < TOL32 * lo
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    h.adam_step(p, grads, m, v, 1, 1e-2)
    z_new = orc.encode(dims, p.cpu().numpy().astype(np.float64)[:-1], x)
    assert rel_l2(h.encode(dev(x), out_dtype=torch.float32).cpu().numpy(), z_new) < 6e-3
    assert rel_l2(z_new, z_ref) > 2e-2          # the step moved the latents by far more than the bf16 tolerance


def test_two_handles_two_streams(data10k):
    """Handles are independent and every call is asynchronous on the caller's stream: two models driven from two
    torch streams interleave without cross-talk (scratch, packed weights and slabs are per handle)."""
    dims = orc.ae_dims(24, 15)
    fa, fb = orc.formula_params(dims, 51), orc.formula_params(dims, 52)
    ha, pa = make_handle(dims, fa, "fp32")
    hb, pb = make_handle(dims, fb, "fp32")
    x = dev(data10k[:4096])
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    ga, gb = torch.zeros_like(pa), torch.zeros_like(pb)
    outs = []
    for _ in range(3):
        with torch.cuda.stream(sa):
            za = ha.encode(x)
            ha.fwd_bwd(x, ga)
        with torch.cuda.stream(sb):
            zb = hb.encode(x)
            hb.fwd_bwd(x, gb)
        outs.append((za, zb))
    torch.cuda.synchronize()
    assert rel(outs[-1][0].cpu().numpy(), orc.encode(dims, fa, data10k[:4096])) < TOL32
    assert rel(outs[-1][1].cpu().numpy(), orc.encode(dims, fb, data10k[:4096])) < TOL32
    la, gra = orc.fwd_bwd(dims, fa, data10k[:4096])
    lb, grb = orc.fwd_bwd(dims, fb, data10k[:4096])
    assert rel(ga.cpu().numpy()[:-1], gra) < TOL32 and rel(gb.cpu().numpy()[:-1], grb) < TOL32


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_row_offsets_beyond_4gib(mode):
    """24M rows x 24 float64 columns = 4.6 GB in one call: byte offsets pass 2^32; rows at the far end encode / decode
    exactly like the same rows in a small call (size-independent property at beyond-BASELINE table sizes)."""
    dims = orc.ae_dims(24, 15)
    h, _ = make_handle(dims, orc.formula_params(dims, 5), mode)
    n = 24_000_000
    x = torch.rand((n, 24), dtype=torch.float64, device="cuda")
    idx = torch.tensor([0, 1, 17, 12_345_678, n - 33, n - 1], device="cuda")
    z = h.encode(x)
    assert torch.equal(z[idx], h.encode(x[idx].contiguous()))
    d = h.decode(z)
    assert torch.equal(d[idx], h.decode(z[idx].contiguous()))
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(d).all())
    del x, z, d
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n", [700, 20000])
def test_fused_normalisation_on_load_in_training(n):
    """features != NULL: the kernels normalise on load ((x - min)/range in float64, one rounding to float32), so
    training on raw rows + features equals training on pre-normalised rows bit for bit (small-batch and throughput
    kernels; the CLI pre-normalises like the reference, an FFI caller need not)."""
    dims = orc.ae_dims(24, 15)
    flat = orc.formula_params(dims, 19)
    raw = synth.cms_rows(n, row0=11)
    feats = orc.find_minmax(raw)
    h, p = make_handle(dims, flat, "fp32")
    ga, gb = torch.zeros_like(p), torch.zeros_like(p)
    h.fwd_bwd(dev(raw), ga, features=dev(feats))
    h.fwd_bwd(dev(orc.normalize(raw)), gb)
    assert torch.equal(ga, gb)
    _, la = h.forward_loss(dev(raw), features=dev(feats), want_recon=False)
    _, lb = h.forward_loss(dev(orc.normalize(raw)), want_recon=False)
    assert la.item() == lb.item()


def test_persistent_loop_remainder_on_small_batch_kernels(monkeypatch):
    """33,095 rows = 2 full rounds of 256 workgroups + 6 groups + 7 rows: the remainder is accumulated by the small-batch
    kernels (default) or run as a third, mostly idle round (BALER_AMD_TAIL_SPLIT=0): same gradient, both at the oracle bar."""
    dims = orc.ae_dims(24, 15)
    flat = orc.formula_params(dims, 23)
    n = 2 * 256 * 64 + 6 * 64 - 57
    x = orc.normalize(synth.cms_rows(n, row0=5))
    lo, go = orc.fwd_bwd(dims, flat, x)
    res = []
    for split in ("1", "0"):
        monkeypatch.setenv("BALER_AMD_TAIL_SPLIT", split)
        h, p = make_handle(dims, flat, "fp32")
        g = torch.zeros_like(p)
        h.fwd_bwd(dev(x), g)
        gh = g.cpu().numpy().astype(np.float64)
        assert rel(gh[:-1], go) < TOL32 and abs(gh[-1] - lo) < TOL32 * lo
        res.append(gh)
    assert rel(res[0], res[1]) < 1e-6 and not np.array_equal(res[0], res[1])     # two different summation orders


# ---- round-2 boundary additions ---------------------------------------------------------------------
def test_col_minmax_and_sharded_features_bit_exact():
    """bamd_col_minmax on row shards + min / max combination == bamd_minmax of the whole table, bit for bit (what the
    data-parallel helper.process does with one MIN and one MAX all-reduce)."""
    raw = synth.cms_rows(100_003)
    whole = native.minmax(dev(raw)).cpu().numpy()
    cuts = [0, 1, 33_334, 66_668, 100_003]
    mm = [native.col_minmax(dev(raw[a:b])).cpu().numpy() for a, b in zip(cuts[:-1], cuts[1:])]
    mn = np.min([m[0] for m in mm], axis=0)
    mx = np.max([m[1] for m in mm], axis=0)
    assert np.array_equal(np.stack([mn, mx - mn]), whole)
    assert np.array_equal(whole, np.stack([raw.min(0), raw.max(0) - raw.min(0)]))


def test_handle_free_kernels_on_two_streams():
    """The handle-free reductions keep their scratch per (device, stream): two streams reducing different tables at the same
    time do not overwrite each other's partial results."""
    a = dev(synth.cms_rows(400_000))
    b = dev(synth.cms_rows(400_000, row0=1_000_000) * 3.0 + 1.0)
    want_a, want_b = native.minmax(a).clone(), native.minmax(b).clone()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(20):
        with torch.cuda.stream(s1):
            ra = native.minmax(a)
        with torch.cuda.stream(s2):
            rb = native.minmax(b)
        torch.cuda.synchronize()
        assert torch.equal(ra, want_a) and torch.equal(rb, want_b)


def test_hostio_round_trip_with_block_events():
    """hostio on the device: rows go up through pinned staging (range, block-cyclic and index plans), come back with per-block
    producer events, and chunk boundaries that cut blocks at odd places change nothing."""
    from baler_amd import hostio
    src = synth.cms_rows(50_000)
    for plan, want in ((None, src), (hostio.RowPlan.contiguous(50_000, 1, 3), src[16_667:33_334]),
                       (hostio.RowPlan.cyclic(50_000, 512, 2, 8), None)):
        t = hostio.upload_rows(src, plan, "cuda:0", chunk_bytes=1 << 20)
        if want is None:
            want = hostio.upload_rows(src, plan, "cpu").numpy()
        assert np.array_equal(t.cpu().numpy(), want)
    x = dev(src)
    out = torch.empty_like(x)
    ready = []
    for s in range(0, 50_000, 7_000):
        e = min(s + 7_000, 50_000)
        out[s:e] = x[s:e] * 2.0
        ev = torch.cuda.Event()
        ev.record()
        ready.append((e, ev))
    back = hostio.download_rows(out, ready=ready, chunk_bytes=3 << 20)
    assert np.array_equal(back, src * 2.0)
    assert np.array_equal(hostio.download_rows(out[:0]), src[:0] * 2.0)


@pytest.mark.parametrize("mode,n,bs", [("fp32", 3000, 512), ("fp64", 1300, 512), ("fp32", 40000, 16384), ("bf16", 9000, 4096)])
def test_train_epoch_equals_the_per_step_loop(mode, n, bs, data10k):
    """bamd_train_epoch (the batch loop of training.fit, training.py:64-97, inside the library: ONE host call per epoch) is
    bit-identical to one bamd_train_step per batch: parameters, Adam moments, the running loss, the last batch's gradient and
    the step count -- over small-batch steps (4-row chain / fp64 chain), the throughput pair and the bf16 kernels, with the
    partial last batch the reference keeps (training.py:237-263)."""
    dims = orc.ae_dims(24, 15)
    flat = orc.formula_params(dims, 21)
    x = dev(np.concatenate([data10k] * 4)[:n])
    res = []
    for one_call in (False, True):
        h, p = make_handle(dims, flat, mode)
        m, v, g = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
        acc = torch.zeros(1, dtype=torch.float64, device="cuda")
        t = 4                                           # Adam's step counter does not have to start at 1
        for _ in range(2):                              # two epochs: the second starts from the first's state
            if one_call:
                t += h.train_epoch(x, bs, p, m, v, t + 1, 1e-3, loss_accum=acc, grads=g)
            else:
                for a in range(0, n, bs):
                    t += 1
                    h.train_step(x[a:a + bs], p, m, v, t, 1e-3, loss_accum=acc, grads=g)
        res.append((t, p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), g.cpu().numpy(), acc.item()))
        h.close()
    (t0, p0, m0, v0, g0, a0), (t1, p1, m1, v1, g1, a1) = res
    assert t0 == t1 == 4 + 2 * ((n + bs - 1) // bs)
    assert np.array_equal(p0, p1) and np.array_equal(m0, m1) and np.array_equal(v0, v1) and np.array_equal(g0, g1) and a0 == a1
    assert np.isfinite(a1) and a1 > 0
