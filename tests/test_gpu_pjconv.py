"""PJ_Conv_AE on MI355X (pjconv.hip, bamd_create_pjconv): against the reference fixture g19 and the float64 restatement
(tests/pjconv_ref.py) at rel() = max(rel-L2, max-norm) <= 1e-5 (Adam: 1e-4), ragged image counts with float32 / float64 inputs,
normalise-on-load and the un-normalise epilogue, a large encode / decode checked on sampled rows, bitwise repeatability, the epoch
calls against step-by-step calls, and the modes a PJ_Conv_AE handle refuses."""
import numpy as np
import pytest
import torch

import pjconv_ref
from pjconv_ref import rel
from baler_amd import native
from baler_amd.modules import models

pytestmark = pytest.mark.gpu

TOL, TOL_ADAM = 1e-5, 1e-4


def seeded_init(z, seed):
    torch.manual_seed(seed)
    return models.pj_conv_init(z).numpy()


def make(z, flat, mode="fp32"):
    h = native.Handle.pj_conv(z, mode)
    p = torch.from_numpy(np.concatenate([flat, [0.0]]).astype(np.float32)).cuda()
    h.load_params(p)
    return h, p


def frames(n, seed):
    return np.random.default_rng(seed).random((n, 784)).astype(np.float32)


def tensor_slices(z):
    return {k: (off, int(np.prod(shape))) for k, off, shape in pjconv_ref.layout(z)[0]}


def check_digest(g, prefix, flat, z, tol, what):
    for k, (off, n) in tensor_slices(z).items():
        a = flat[off:off + n]
        if f"{prefix}{k}" in g.files:
            assert rel(a, g[f"{prefix}{k}"]) <= tol, (what, k, rel(a, g[f"{prefix}{k}"]))
        else:
            idx = g[f"{prefix}{k}.idx"]
            assert rel(a[idx], g[f"{prefix}{k}.sample"]) <= tol, (what, k, rel(a[idx], g[f"{prefix}{k}.sample"]))
            assert abs(np.linalg.norm(a.astype(np.float64)) / g[f"{prefix}{k}.norm"] - 1) <= tol, (what, k)


def test_reference_fixture(golden):
    g = golden("g19_pjconv.npz")
    z, seed = int(g["z_dim"]), int(g["seed"])
    init = seeded_init(z, seed)
    h, p = make(z, init)
    assert h.path == "fused" and h.nparams == 2504541 + 1001 * z and h.compute_mode == native.MODE_F32
    x = g["x"]
    xt = torch.from_numpy(x).cuda()
    code = h.encode(xt).cpu().numpy()
    assert rel(code, g["z"]) <= TOL and rel(code, pjconv_ref.encode(z, init, x)) <= TOL
    recon, loss = h.forward_loss(xt)
    ref_loss = pjconv_ref.loss(z, init, x)
    assert rel(recon.cpu().numpy(), g["recon"]) <= TOL
    assert rel(recon.cpu().numpy(), pjconv_ref.forward(z, init, x)) <= TOL
    assert abs(loss.item() / ref_loss - 1) <= TOL and abs(loss.item() / float(g["loss"]) - 1) <= TOL
    dec = h.decode(torch.from_numpy(g["z"]).cuda()).cpu().numpy()
    assert rel(dec, pjconv_ref.decode(z, init, g["z"])) <= TOL
    grads = torch.empty(h.nparams + 1, dtype=torch.float32, device="cuda")
    h.fwd_bwd(xt, grads)
    gr = grads.cpu().numpy().astype(np.float64)
    l_ref, g_ref = pjconv_ref.fwd_bwd(z, init, x)
    assert abs(gr[-1] / l_ref - 1) <= TOL
    for k, (off, n) in tensor_slices(z).items():      # every tensor on its own scale
        assert rel(gr[off:off + n], g_ref[off:off + n]) <= TOL, (k, rel(gr[off:off + n], g_ref[off:off + n]))
    check_digest(g, "grad.", gr[:-1], z, TOL, "gradient")
    # 3 Adam steps (lr of the fixture) through bamd_train_step
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in (1, 2, 3):
        h.train_step(xt, p, m, v, step, float(g["lr"]))
    check_digest(g, "p3.", p.cpu().numpy()[:-1].astype(np.float64), z, TOL_ADAM, "params after 3 Adam steps")


@pytest.mark.parametrize("n", [1, 3, 17, 63, 64, 65, 511, 512, 513, 4097])
def test_ragged_image_counts(n):
    z = 17
    init = seeded_init(z, 5)
    h, _ = make(z, init)
    x = frames(n, n)
    rng = np.random.default_rng(n + 1)
    mn = rng.uniform(-2, 1, 784)
    rg = rng.uniform(0.5, 3, 784)
    raw = x.astype(np.float64) * rg + mn
    feats = torch.from_numpy(np.stack([mn, rg])).cuda()
    xn = ((raw - mn) / rg).astype(np.float32)           # what normalise-on-load computes (float64, rounded once)
    z_ref = pjconv_ref.encode(z, init, xn)
    for dt in (torch.float32, torch.float64):
        got = h.encode(torch.from_numpy(raw).to(dt).cuda(), features=feats, out_dtype=torch.float64).cpu().numpy()
        if dt == torch.float64:
            assert rel(got, z_ref) <= TOL, (n, rel(got, z_ref))
        else:      # float32 raw values: normalised from the rounded input
            xr = ((raw.astype(np.float32).astype(np.float64) - mn) / rg).astype(np.float32)
            assert rel(got, pjconv_ref.encode(z, init, xr)) <= TOL
    zt = torch.from_numpy(z_ref.astype(np.float32)).cuda()
    d_ref = pjconv_ref.decode(z, init, z_ref.astype(np.float32))
    assert rel(h.decode(zt).cpu().numpy(), d_ref) <= TOL
    ren = h.decode(zt.double(), features=feats, out_dtype=torch.float64).cpu().numpy()
    assert rel(ren, d_ref * rg + mn) <= TOL
    mask = (np.arange(784) % 3 == 0).astype(np.uint8)
    ren_i = h.decode(zt, features=feats, int_mask=torch.from_numpy(mask).cuda(), out_dtype=torch.float64).cpu().numpy()
    np.testing.assert_array_equal(ren_i[:, mask == 1], np.trunc(ren[:, mask == 1]))
    np.testing.assert_array_equal(ren_i[:, mask == 0], ren[:, mask == 0])
    recon, loss = h.forward_loss(torch.from_numpy(raw).cuda(), features=feats)
    f_ref = pjconv_ref.forward(z, init, xn)
    assert rel(recon.cpu().numpy(), f_ref) <= TOL
    assert abs(loss.item() / np.sum((f_ref - xn) ** 2) - 1) <= TOL
    if n in (1, 3, 65, 513, 4097):       # 4097: two groups of the training pass
        grads = torch.empty(h.nparams + 1, dtype=torch.float32, device="cuda")
        h.fwd_bwd(torch.from_numpy(raw).cuda(), grads, features=feats)
        l_ref, g_ref = pjconv_ref.fwd_bwd(z, init, xn)
        gr = grads.cpu().numpy().astype(np.float64)
        assert abs(gr[-1] / l_ref - 1) <= TOL
        for k, (off, cnt) in tensor_slices(z).items():
            assert rel(gr[off:off + cnt], g_ref[off:off + cnt]) <= TOL, (n, k, rel(gr[off:off + cnt], g_ref[off:off + cnt]))


def test_large_batch_sampled_rows():
    z, n = 40, 262_144
    init = seeded_init(z, 7)
    h, _ = make(z, init)
    x = torch.rand((n, 784), generator=torch.Generator().manual_seed(3), dtype=torch.float32)
    code = h.encode(x.cuda())
    dec = h.decode(code)
    rows = np.unique(np.concatenate([[0, 1, 8191, 8192, 8193, 131_071, n - 1], np.random.default_rng(0).integers(0, n, 25)]))
    xs = x[rows].numpy()
    assert rel(code[rows].cpu().numpy(), pjconv_ref.encode(z, init, xs)) <= TOL
    assert rel(dec[rows].cpu().numpy(), pjconv_ref.decode(z, init, code[rows].cpu().numpy())) <= TOL


def test_step_is_bitwise_repeatable():
    z = 40
    init = seeded_init(z, 9)
    x = torch.from_numpy(frames(4200, 1)).cuda()
    outs = []
    for _ in range(2):
        h, p = make(z, init)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        grads = torch.empty_like(p)
        h.train_step(x[:513], p, m, v, 1, 1e-3, grads=grads)
        g2 = torch.empty_like(p)
        h.fwd_bwd(x, g2)
        outs.append((p.cpu().numpy(), grads.cpu().numpy(), g2.cpu().numpy()))
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)


def test_train_epoch_equals_steps_and_dp_world1():
    z = 12
    init = seeded_init(z, 11)
    x = torch.from_numpy(frames(1100, 2)).cuda()
    res = []
    for how in ("steps", "epoch", "epoch_dp"):
        h, p = make(z, init)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        acc = torch.zeros(1, dtype=torch.float64, device="cuda")
        grads = torch.empty_like(p)
        if how == "steps":
            for i, s in enumerate(range(0, 1100, 512)):
                h.train_step(x[s:s + 512], p, m, v, 1 + i, 1e-3, loss_accum=acc, grads=grads)
        elif how == "epoch":
            assert h.train_epoch(x, 512, p, m, v, 1, 1e-3, loss_accum=acc, grads=grads) == 3
        else:
            assert h.train_epoch_dp(x, [512, 512, 76], p, m, v, 1, 1e-3, loss_accum=acc, grads=grads) == 3
        res.append((p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), grads.cpu().numpy(), acc.cpu().numpy()))
    for other in res[1:]:
        for a, b in zip(res[0], other):
            np.testing.assert_array_equal(a, b)


def test_modes_and_refusals(capfd):
    h = native.Handle.pj_conv(10, "bf16")
    assert h.compute_mode == native.MODE_F32 and h.path == "fused"
    assert "computes in float32" in capfd.readouterr().err
    with pytest.raises(native.NativeError, match="status -5"):
        native.Handle.pj_conv(10, "fp64")
    for bad in (0, 2451):
        with pytest.raises(native.NativeError, match="status -1"):
            native.Handle.pj_conv(bad)
    for ok in (1, 2450):
        assert native.Handle.pj_conv(ok).nparams == 2504541 + 1001 * ok
    init = seeded_init(3, 1)
    h, _ = make(3, init)
    x = torch.from_numpy(frames(4, 0)).cuda()
    with pytest.raises(native.NativeError, match="status -5"):
        h.activation_means(x)
    grads = torch.empty(h.nparams + 1, dtype=torch.float32, device="cuda")
    with pytest.raises(native.NativeError, match="status -5"):
        h.fwd_bwd_latent(x, torch.zeros((4, 3), dtype=torch.float32, device="cuda"), grads)
