"""FPGA_prototype_model on MI355X: the fused ReLU kernels (fpga.hip) and the layer-wise ReLU path against the reference fixture
g17 and the NumPy restatement (tests/fpga_ref.py), path reporting, the LeakyReLU families never serving a ReLU handle,
determinism, the CLI against g18, and throughput floors against the layer-wise path on the same handle."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

import fpga_ref
from baler_amd import native, synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {"fp32": 1e-5, "fp64": 1e-11}
DT = {"fp32": torch.float32, "fp64": torch.float64}


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def make(n, z, mode, flat, act="relu", dims=None):
    h = native.Handle(dims or fpga_ref.dims(n, z), mode, act=act)
    p = torch.from_numpy(np.concatenate([flat, [0.0]])).to(DT["fp64" if mode == "fp64" else "fp32"]).cuda()
    h.load_params(p)
    return h, p


def init_flat(n, z, seed):
    rng = np.random.default_rng(seed)
    d = fpga_ref.dims(n, z)
    parts = []
    for l in range(6):
        bound = 1.0 / np.sqrt(d[l])
        parts += [rng.uniform(-bound, bound, d[l + 1] * d[l]), rng.uniform(-bound, bound, d[l + 1])]
    return np.concatenate(parts)


def kink_free_rows(d, flat, rows, seed):
    rng = np.random.default_rng(seed)
    out, have = [], 0
    while have < rows:
        c = rng.random((max(2 * (rows - have), 64), d[0]))
        c = c[fpga_ref.off_the_kink(d, flat, c)]
        out.append(c)
        have += c.shape[0]
    return np.concatenate(out)[:rows]


@pytest.mark.parametrize("mode", ["fp32", "fp64"])
def test_reference_fixture(golden, mode):
    g = golden("g17_fpga.npz")
    for tag, (n, z) in (("", (24, 15)), ("_7_3", (7, 3))):
        h, p = make(n, z, mode, g["init" + tag])
        assert h.path == "fused" and h.act == "relu"
        x = torch.from_numpy(g["x" + tag]).cuda()
        assert rel(h.encode(x, out_dtype=torch.float64).cpu(), g["z" + tag]) < TOL[mode]
        zt = torch.from_numpy(g["z" + tag]).cuda()
        assert rel(h.decode(zt, out_dtype=torch.float64).cpu(), g["decoded" + tag]) < TOL[mode]
        recon, loss = h.forward_loss(x)
        assert rel(recon.cpu(), g["recon" + tag]) < TOL[mode]
        assert abs(float(loss) - float(g["loss" + tag])) < TOL[mode] * float(g["loss" + tag])
        grads = torch.zeros_like(p)
        h.fwd_bwd(x, grads)
        gh = grads.cpu().numpy().astype(np.float64)
        assert rel(gh[:-1], g["grad" + tag]) < TOL[mode]
        assert abs(gh[-1] - float(g["loss" + tag])) < TOL[mode] * float(g["loss" + tag])
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        for step in (1, 2, 3):
            h.train_step(x, p, m, v, step, 1e-2)
            if step in (1, 3):
                assert rel(p.cpu().numpy()[:-1], g[f"p{step}" + tag]) < 10 * TOL[mode]
                assert rel(m.cpu().numpy()[:-1], g[f"m{step}" + tag]) < 10 * TOL[mode]
                assert rel(v.cpu().numpy()[:-1], g[f"v{step}" + tag]) < 10 * TOL[mode]


@pytest.mark.parametrize("mode", ["fp32", "fp64"])
@pytest.mark.parametrize("io", [torch.float32, torch.float64])
def test_ragged_row_counts(mode, io):
    n, z = 24, 15
    d = fpga_ref.dims(n, z)
    flat = init_flat(n, z, 3)
    h, p = make(n, z, mode, flat)
    base = kink_free_rows(d, flat, 70000, 5)
    rng = np.random.default_rng(9)
    for rows in (1, 15, 16, 17, 511, 512, 513, 4099, 65537, 1 << 20):
        if rows <= base.shape[0]:
            xr = base[:rows]
        else:
            xr = base[rng.integers(0, base.shape[0], rows)]
        x = torch.from_numpy(xr).to(io).cuda()
        xh = x.cpu().numpy().astype(np.float64)
        sl = slice(None) if rows <= 4099 else slice(0, rows, max(1, rows // 4096))
        otol = TOL[mode] * 10 if io == torch.float64 else 1e-6      # (float32 outputs: their own rounding)
        zt = h.encode(x, out_dtype=io)
        assert rel(zt.cpu().numpy()[sl], fpga_ref.encode(d, flat, xh[sl])) < otol
        feats = torch.tensor(np.stack([np.full(n, -1.0), np.full(n, 3.0)]), dtype=torch.float64).cuda()
        mask = torch.tensor([1 if c % 3 == 0 else 0 for c in range(n)], dtype=torch.uint8).cuda()
        out = h.decode(zt, features=feats, int_mask=mask, out_dtype=torch.float64).cpu().numpy()
        plain = h.decode(zt, features=feats, out_dtype=torch.float64).cpu().numpy()
        dec = h.decode(zt, out_dtype=torch.float64).cpu().numpy()
        assert rel(dec[sl], fpga_ref.decode(d, flat, zt.cpu().numpy().astype(np.float64)[sl])) < 10 * TOL[mode]
        assert np.array_equal(plain, dec * 3.0 - 1.0)                    # un-normalise: x * range + min, two roundings
        int_cols = np.arange(n) % 3 == 0
        assert np.array_equal(out[:, int_cols], np.trunc(plain[:, int_cols]))
        assert np.array_equal(out[:, ~int_cols], plain[:, ~int_cols])
        recon, loss = h.forward_loss(x)
        r_ref = fpga_ref.forward(d, flat, xh)
        assert rel(recon.cpu().numpy()[sl], r_ref[sl]) < otol
        l_ref = float(np.sum((r_ref - xh) ** 2) / n)
        assert abs(float(loss) - l_ref) < 10 * TOL[mode] * l_ref
        grads = torch.zeros_like(p)
        h.fwd_bwd(x, grads)
        l_ref, g_ref = fpga_ref.fwd_bwd(d, flat, xh)
        gh = grads.cpu().numpy().astype(np.float64)
        assert rel(gh[:-1], g_ref) < 10 * TOL[mode]


@pytest.mark.parametrize("mode", ["fp32", "fp64"])
def test_fused_shapes_and_layerwise_shapes(mode, capfd):
    for (n, z) in ((1, 1), (7, 3), (24, 12), (24, 15), (33, 10), (64, 32), (65, 8), (24, 33)):
        d = fpga_ref.dims(n, z)
        flat = init_flat(n, z, n * 100 + z)
        capfd.readouterr()
        h, p = make(n, z, mode, flat)
        err = capfd.readouterr().err
        fused = n <= 64 and z <= 32
        assert h.path == ("fused" if fused else "generic"), (n, z)
        assert h.act == "relu"
        assert ("layer by layer" in err) == (not fused), err
        x = torch.from_numpy(kink_free_rows(d, flat, 777, n)).cuda()
        xh = x.cpu().numpy()
        assert rel(h.encode(x, out_dtype=torch.float64).cpu(), fpga_ref.encode(d, flat, xh)) < 10 * TOL[mode]
        recon, _ = h.forward_loss(x)
        assert rel(recon.cpu(), fpga_ref.forward(d, flat, xh)) < 10 * TOL[mode]
        grads = torch.zeros_like(p)
        h.fwd_bwd(x, grads)
        _, g_ref = fpga_ref.fwd_bwd(d, flat, xh)
        assert rel(grads.cpu().numpy()[:-1], g_ref) < 10 * TOL[mode]


@pytest.mark.parametrize("mode", ["fp32", "fp64"])
def test_fused_agrees_with_layerwise(mode, monkeypatch):
    n, z = 24, 15
    d = fpga_ref.dims(n, z)
    flat = init_flat(n, z, 11)
    x = torch.from_numpy(kink_free_rows(d, flat, 5000, 12)).cuda()
    res = {}
    for forced in (False, True):
        if forced:
            monkeypatch.setenv("BALER_AMD_FORCE_GENERIC", "1")
        h, p = make(n, z, mode, flat)
        assert h.path == ("generic" if forced else "fused")
        grads = torch.zeros_like(p)
        h.fwd_bwd(x, grads)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        for step in range(1, 4):
            h.train_step(x[:512], p, m, v, step, 1e-3)
        res[forced] = (h.encode(x).cpu().numpy(), h.forward_loss(x)[0].cpu().numpy(), grads.cpu().numpy(), p.cpu().numpy())
    for a, b in zip(res[False], res[True]):
        assert rel(a, b) < 10 * TOL[mode]


@pytest.mark.parametrize("mode", ["fp32", "fp64", "bf16"])
def test_relu_handle_with_ae_widths_runs_layerwise(mode):
    dims = [24, 200, 100, 50, 15, 50, 100, 200, 24]
    rng = np.random.default_rng(2)
    nps = sum(dims[l + 1] * dims[l] + dims[l + 1] for l in range(8))
    flat = rng.uniform(-0.1, 0.1, nps)
    h, p = make(0, 0, mode, flat, dims=dims)
    assert h.path == "generic" and h.act == "relu"
    assert h.compute_mode == (native.MODE_F64 if mode == "fp64" else native.MODE_F32)
    x = torch.from_numpy(rng.random((3000, 24))).cuda()
    xh = x.cpu().numpy()

    def fwd(xv):      # ReLU restatement of the 8-layer model
        y, off = xv, 0
        for l in range(8):
            w = flat[off:off + dims[l + 1] * dims[l]].reshape(dims[l + 1], dims[l])
            off += dims[l + 1] * dims[l]
            b = flat[off:off + dims[l + 1]]
            off += dims[l + 1]
            y = y @ w.T + b
            if l not in (3, 7):
                y = np.maximum(y, 0.0)
        return y
    tol = 1e-11 if mode == "fp64" else 1e-5
    recon, _ = h.forward_loss(x)
    assert rel(recon.cpu(), fwd(xh)) < 10 * tol
    grads = torch.zeros_like(p)
    h.fwd_bwd(x[:512], grads)
    xt = torch.from_numpy(xh[:512]).requires_grad_(False)
    ps = torch.from_numpy(flat).requires_grad_(True)
    y, off = xt, 0
    for l in range(8):
        w = ps[off:off + dims[l + 1] * dims[l]].view(dims[l + 1], dims[l])
        off += dims[l + 1] * dims[l]
        b = ps[off:off + dims[l + 1]]
        off += dims[l + 1]
        y = y @ w.T + b
        if l not in (3, 7):
            y = torch.relu(y)
    loss = ((y - xt) ** 2).sum() / 24
    loss.backward()
    assert rel(grads.cpu().numpy()[:-1], ps.grad.numpy()) < 10 * tol


@pytest.mark.parametrize("mode", ["fp32", "fp64"])
def test_explicit_leaky_is_bamd_create(mode):
    dims = [24, 200, 100, 50, 15, 50, 100, 200, 24]
    nps = sum(dims[l + 1] * dims[l] + dims[l + 1] for l in range(8))
    flat = np.random.default_rng(4).uniform(-0.1, 0.1, nps)
    x = torch.from_numpy(np.random.default_rng(5).random((2048, 24))).cuda()
    outs = []
    for explicit in (False, True):
        if explicit:
            h, p = make(0, 0, mode, flat, act="leaky_relu", dims=dims)
        else:
            h = native.Handle.__new__(native.Handle)
            import ctypes
            h.dims, h.mode = dims, native.MODE_NAMES[mode]
            h.device = torch.device("cuda", 0)
            arr = (ctypes.c_int * 9)(*dims)
            hh = ctypes.c_void_p()
            assert native.lib().bamd_create(arr, 8, h.mode, 0, ctypes.byref(hh)) == 0
            h._h = hh
            h.nparams = int(native.lib().bamd_param_count(hh))
            h.param_dtype = torch.float64 if mode == "fp64" else torch.float32
            h.compute_mode = int(native.lib().bamd_mode_of(hh))
            p = torch.from_numpy(np.concatenate([flat, [0.0]])).to(h.param_dtype).cuda()
            h.load_params(p)
        assert h.act == "leaky_relu"
        grads = torch.zeros_like(p)
        h.fwd_bwd(x[:512], grads)
        outs.append((h.path, h.encode(x).cpu().numpy(), grads.cpu().numpy()))
    assert outs[0][0] == outs[1][0]
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])


@pytest.mark.parametrize("mode", ["fp32", "fp64"])
@pytest.mark.parametrize("forced", [False, True])
def test_exact_zero_pre_activation_and_nan_rows(mode, forced, monkeypatch):
    if forced:
        monkeypatch.setenv("BALER_AMD_FORCE_GENERIC", "1")
    n, z = 24, 15
    d = fpga_ref.dims(n, z)
    flat = init_flat(n, z, 21)
    flat[:n * 20] = 0.0                  # en1 weights 0 ...
    flat[n * 20:n * 20 + 10] = 0.0       # ... and half its biases 0: those ten units sit exactly at the kink
    h, p = make(n, z, mode, flat)
    x = torch.from_numpy(np.random.default_rng(1).random((300, n))).cuda()
    grads = torch.zeros_like(p)
    h.fwd_bwd(x, grads)
    g = grads.cpu().numpy()
    _, g_ref = fpga_ref.fwd_bwd(d, flat, x.cpu().numpy())
    w1 = g[:n * 20].reshape(20, n)
    assert np.all(w1[:10] == 0.0) and np.all(g[n * 20:n * 20 + 10] == 0.0)
    assert rel(g[:-1], g_ref) < 10 * TOL[mode]
    flat2 = init_flat(n, z, 22)
    h2, _ = make(n, z, mode, flat2)
    xn = np.random.default_rng(2).random((200, n))
    xn[7, 3] = np.nan
    xn[150, 0] = np.nan
    xt = torch.from_numpy(xn).cuda()
    zt = h2.encode(xt).cpu().numpy()
    r, _ = h2.forward_loss(xt)
    r = r.cpu().numpy()
    bad = np.zeros(200, bool)
    bad[[7, 150]] = True
    assert np.all(np.isnan(zt[bad])) and np.all(np.isfinite(zt[~bad]))
    assert np.all(np.isnan(r[bad])) and np.all(np.isfinite(r[~bad]))


@pytest.mark.parametrize("mode", ["fp32", "fp64"])
def test_repeatable_and_epoch_equals_steps(mode):
    n, z = 24, 15
    flat = init_flat(n, z, 31)
    x = torch.from_numpy(np.random.default_rng(3).random((70001, n))).cuda()
    h, p = make(n, z, mode, flat)
    g1, g2 = torch.zeros_like(p), torch.zeros_like(p)
    h.fwd_bwd(x, g1)
    h.fwd_bwd(x, g2)
    assert torch.equal(g1, g2)
    runs = []
    for epoch_call in (False, True, False):
        hh, pp = make(n, z, mode, flat)
        m, v = torch.zeros_like(pp), torch.zeros_like(pp)
        acc = torch.zeros(1, dtype=torch.float64).cuda()
        xs = x[:5000]
        if epoch_call:
            hh.train_epoch(xs, 512, pp, m, v, 1, 1e-3, loss_accum=acc)
        else:
            for i, r0 in enumerate(range(0, 5000, 512)):
                hh.train_step(xs[r0:r0 + 512], pp, m, v, 1 + i, 1e-3, loss_accum=acc)
        runs.append((pp.cpu(), m.cpu(), v.cpu(), acc.cpu()))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    for a, b in zip(runs[0], runs[2]):
        assert torch.equal(a, b)


def test_small_batches_match_restatement():
    n, z = 24, 15
    d = fpga_ref.dims(n, z)
    flat = init_flat(n, z, 41)
    xh = kink_free_rows(d, flat, 2048, 42)
    h, p = make(n, z, "fp64", flat)
    x = torch.from_numpy(xh).cuda()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    pr, mr, vr = flat.copy(), np.zeros_like(flat), np.zeros_like(flat)
    step = 0
    for epoch in range(3):
        for r0 in range(0, 2048, 512):
            step += 1
            h.train_step(x[r0:r0 + 512], p, m, v, step, 1e-3)
            _, g = fpga_ref.fwd_bwd(d, pr, xh[r0:r0 + 512])
            fpga_ref.adam_step(pr, g, mr, vr, step, 1e-3)
    assert rel(p.cpu().numpy()[:-1], pr) < 1e-9


def test_bf16_mode_gives_fp32_with_notice(capfd):
    flat = init_flat(24, 15, 51)
    capfd.readouterr()
    h, p = make(24, 15, "bf16", flat)
    err = capfd.readouterr().err
    assert h.compute_mode == native.MODE_F32 and h.path == "fused" and "float32" in err
    h32, _ = make(24, 15, "fp32", flat)
    x = torch.from_numpy(np.random.default_rng(0).random((1000, 24))).cuda()
    assert torch.equal(h.encode(x), h32.encode(x))


@pytest.mark.parametrize("mode", ["fp32", "fp64"])
@pytest.mark.parametrize("forced", [False, True])
def test_swae_latent_gradient(mode, forced, monkeypatch):
    if forced:
        monkeypatch.setenv("BALER_AMD_FORCE_GENERIC", "1")
    n, z = 24, 15
    d = fpga_ref.dims(n, z)
    flat = init_flat(n, z, 61)
    xh = kink_free_rows(d, flat, 700, 62)
    lg = np.random.default_rng(63).standard_normal((700, z)) * 1e-2
    h, p = make(n, z, mode, flat)
    grads = torch.zeros_like(p)
    h.fwd_bwd_latent(torch.from_numpy(xh).cuda(), torch.from_numpy(lg).to(p.dtype).cuda(), grads)
    loss, g_ref = fpga_ref.fwd_bwd(d, flat, xh, latent_grad=lg)
    gh = grads.cpu().numpy().astype(np.float64)
    assert rel(gh[:-1], g_ref) < 10 * TOL[mode]
    assert abs(gh[-1] - loss) < 10 * TOL[mode] * loss


@pytest.mark.parametrize("mode", ["fp32", "fp64"])
def test_dp_world1_epoch_matches_train_epoch(mode):
    n, z = 24, 15
    flat = init_flat(n, z, 71)
    x = torch.from_numpy(np.random.default_rng(72).random((3000, n))).cuda()
    res = []
    for use_comm in (False, True):
        h, p = make(n, z, mode, flat)
        if use_comm:
            h.comm_init(native.comm_unique_id(), 0, 1)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        acc = torch.zeros(1, dtype=torch.float64).cuda()
        if use_comm:
            sizes = [512] * 5 + [3000 - 2560]
            h.train_epoch_dp(x, sizes, p, m, v, 1, 1e-3, loss_accum=acc)
        else:
            h.train_epoch(x, 512, p, m, v, 1, 1e-3, loss_accum=acc)
        torch.cuda.synchronize()
        res.append((p.cpu(), m.cpu(), v.cpu(), acc.cpu()))
        if use_comm:
            h.comm_release()
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("compute_mode", ["fp64", "fp32"])
def test_cli_matches_reference_run(tmp_path, golden, monkeypatch, compute_mode):
    g = golden("g18_fpga_cli.npz")
    from baler_amd.modules import helper
    for k in [k for k in vars(helper.Config) if not k.startswith("__")]:    # (the Config class is mutated in place per project)
        delattr(helper.Config, k)
    ws = tmp_path / "workspaces"
    shutil.copytree(os.path.join(REPO, "workspaces", "CMS_workspace"), ws / "CMS_workspace")
    (ws / "__init__.py").write_text("")
    cfg = ws / "CMS_workspace" / "CMS_project_v1" / "config" / "CMS_project_v1_config.py"
    src = cfg.read_text().replace('c.model_name = "AE"', 'c.model_name = "FPGA_prototype_model"')
    cfg.write_text(src.replace("c.activation_extraction = True", "c.activation_extraction = False"))
    for dd in ("compressed_output", "decompressed_output", "plotting", "training"):
        os.makedirs(ws / "CMS_workspace" / "CMS_project_v1" / "output" / dd, exist_ok=True)
    os.makedirs(ws / "CMS_workspace" / "data", exist_ok=True)
    np.savez(ws / "CMS_workspace" / "data" / "example_CMS_data.npz", data=synth.cms_rows(10000), names=synth.CMS_NAMES)
    monkeypatch.chdir(tmp_path)
    monkeypatch.syspath_prepend(str(tmp_path))
    for k in [k for k in sys.modules if k == "workspaces" or k.startswith("workspaces.")]:
        del sys.modules[k]
    from baler_amd import baler
    from baler_amd.modules import helper, models
    models.set_default_mode(compute_mode)
    try:
        def factory(name):
            cls = getattr(models, name)
            assert cls is models.FPGA_prototype_model
            return lambda n_features, z_dim: cls(n_features, z_dim).load_flat(g["init"])
        monkeypatch.setattr(helper, "model_init", factory)
        for mode_name in ("train", "compress", "decompress"):
            baler.main(["--project", "CMS_workspace", "CMS_project_v1", "--mode", mode_name])
    finally:
        models.set_default_mode("fp32")
    out = ws / "CMS_workspace" / "CMS_project_v1" / "output"
    loss = np.load(out / "training" / "loss_data.npy")
    assert loss.shape == g["loss_data"].shape
    assert np.array_equal(np.load(out / "training" / "normalization_features.npy"), g["normalization_features"])
    sd = torch.load(out / "compressed_output" / "model.pt")
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert all(v.dtype == torch.float64 for v in sd.values())
    final = np.concatenate([v.numpy().ravel() for v in sd.values()])
    comp = np.load(out / "compressed_output" / "compressed.npz")
    dec = np.load(out / "decompressed_output" / "decompressed.npz")
    assert comp["data"].shape == tuple(g["compressed_shape"]) and dec["data"].shape == tuple(g["decompressed_shape"])
    if compute_mode == "fp64":
        assert rel(loss[0], g["loss_data"][0]) < 1e-9
        assert rel(final[g["final_sample_idx"]], g["final_sample"]) < 1e-6
        assert rel(comp["data"][:64], g["compressed_head"]) < 1e-6
        assert rel(dec["data"].sum(axis=0), g["decompressed_colsum"]) < 1e-6
    else:
        assert rel(loss[0][:3], g["loss_data"][0][:3]) < 1e-5
        assert np.all(np.abs(loss[0] - g["loss_data"][0]) <= 0.05 * np.abs(g["loss_data"][0]))


def _ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def test_throughput_floors_vs_layerwise(monkeypatch):
    """fp32 encode at 1M rows, the fp32 training step at the CMS config's 512-row batch and the fp64 fwd_bwd at 1M rows against the
    layer-wise kernels on the same handle (fp32 training batches above 8192 rows are dispatched to the layer-wise kernels)."""
    n, z = 24, 15
    flat = init_flat(n, z, 81)
    t = {}
    for forced in (False, True):
        if forced:
            monkeypatch.setenv("BALER_AMD_FORCE_GENERIC", "1")
        x = torch.rand((1 << 20, n), device="cuda", dtype=torch.float32)
        h, p = make(n, z, "fp32", flat)
        zt = torch.empty((1 << 20, z), device="cuda", dtype=torch.float32)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        enc = _ms(lambda: h.encode(x, out=zt))
        step = _ms(lambda: h.train_step(x[:512], p, m, v, 1, 1e-6))
        h64, p64 = make(n, z, "fp64", flat)
        x64 = x.double()
        g64 = torch.zeros_like(p64)
        fb64 = _ms(lambda: h64.fwd_bwd(x64, g64))
        t[forced] = (enc, step, fb64)
    print(f"fused / layer-wise: encode 1M fp32 {t[False][0]:.3f} / {t[True][0]:.3f} ms, train_step 512 fp32 {t[False][1]:.4f} / "
          f"{t[True][1]:.4f} ms, fwd_bwd 1M fp64 {t[False][2]:.3f} / {t[True][2]:.3f} ms")
    assert t[True][0] >= 1.5 * t[False][0]
    assert t[True][1] >= 1.3 * t[False][1]
    assert t[True][2] >= 3.0 * t[False][2]
