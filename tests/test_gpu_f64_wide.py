"""The fused fp64 inference class for wide tables (fused64w.hip: AE(n, z) with the reference's hidden widths, 128 <= n <= 4096, z <= 63):
which handles it serves, parity with the scalar fp64 checker at the project's fp64 bar, the persistent loop and repeatability, guard
bands, 16-bit latent codes, fragments that follow the parameters, and its speed against the layer-wise kernels it replaces.

The bar is rel() < 1e-11, the fp64 bar of every other fp64 test here (sums of at most 4096 products in binary64: ~4096 * 2^-53 = 5e-13
per dot product before cancellation).  Row counts 1, 15, 16, 17, 60, 85 and 300 straddle the 16-row tile of a wave and the 64-row group
of a workgroup and, at 300, give a workgroup more than one group once the grid is capped.  The reference of a shape is computed once on
300 rows; a smaller call is compared with its first rows (rows are independent)."""
import functools

import numpy as np
import pytest
import torch

from baler_amd import native
from oracle import c_oracle as orc
from test_gpu_guard_bands import both, forward_loss_raw
from test_gpu_latent16 import assert_same_bits
from test_gpu_parity import rel
from test_gpu_perf_floor import _ms

pytestmark = pytest.mark.gpu

TOL = 1e-11
SERVED = [(128, 8), (129, 7), (625, 7), (900, 9), (200, 63), (2500, 25), (4096, 10)]
PARITY = [(128, 8), (129, 7), (625, 7), (200, 63), (2500, 25), (4096, 10)]
ROWS = (1, 15, 16, 17, 60, 85, 300)
NOTICE = "has fused encode / decode / validation kernels only: training runs layer by layer"


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C", copy=True))      # (a copy: the shared references are read-only)
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def handle(dims, flat, act="leaky_relu"):
    h = native.Handle(dims, "fp64", act=act)
    p = torch.from_numpy(np.concatenate([flat, [0.0]])).cuda()
    h.load_params(p)
    return h, p


@functools.lru_cache(maxsize=None)
def case(F, Z):
    """Inputs and checker results of one shape on 300 rows (read-only for every test)."""
    dims = orc.ae_dims(F, Z)
    flat = orc.formula_params(dims, 50 + F)
    rng = np.random.default_rng(1000 * F + Z)
    raw = rng.uniform(-3.0, 9.0, size=(300, F))
    feats = orc.find_minmax(raw)                               # [min | range]
    xn = (raw - feats[0]) / feats[1]
    xn32 = xn.astype(np.float32)
    raw32 = raw.astype(np.float32)
    c = dict(dims=dims, flat=flat, raw=raw, feats=feats, xn=xn, xn32=xn32, raw32=raw32)
    c["z"] = orc.encode(dims, flat, xn)
    c["z_xn32"] = orc.encode(dims, flat, xn32.astype(np.float64))
    c["z_raw32"] = orc.encode(dims, flat, (raw32.astype(np.float64) - feats[0]) / feats[1])
    c["dec"] = orc.decode(dims, flat, c["z"])
    c["dec_z32"] = orc.decode(dims, flat, c["z"].astype(np.float32).astype(np.float64))
    c["fwd"] = orc.forward(dims, flat, xn)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# ---- 1. path -----------------------------------------------------------------------------------------------------------------------
def test_path_of_served_and_unserved_shapes(monkeypatch, capfd):
    monkeypatch.delenv("BALER_AMD_QUIET", raising=False)
    monkeypatch.delenv("BALER_AMD_F64_WIDE", raising=False)
    for F, Z in SERVED:
        capfd.readouterr()
        h = native.Handle(orc.ae_dims(F, Z), "fp64")
        err = capfd.readouterr().err
        assert h.path == "fused-infer", (F, Z)
        assert err.count(NOTICE) == 1 and "no fused kernel instantiation" not in err, (F, Z, err)      # said once, and true
        h.close()
    monkeypatch.setenv("BALER_AMD_F64_WIDE", "0")
    for F, Z in SERVED:
        h = native.Handle(orc.ae_dims(F, Z), "fp64")
        assert h.path == "generic", (F, Z)
        h.close()
    monkeypatch.delenv("BALER_AMD_F64_WIDE")
    for F, Z in [(4097, 10), (500, 64), (100, 70)]:
        h = native.Handle(orc.ae_dims(F, Z), "fp64")
        assert h.path == "generic", (F, Z)
        h.close()
    h = native.Handle(orc.ae_dims(625, 7), "fp64", act="relu")
    assert h.path == "generic"
    h.close()
    h = native.Handle(orc.ae_dims(127, 16), "fp64")            # the 4-row chain class below the wide one: trains fused, as before
    assert h.path == "fused"
    h.close()
    monkeypatch.setenv("BALER_AMD_QUIET", "1")
    capfd.readouterr()
    h = native.Handle(orc.ae_dims(625, 7), "fp64")
    assert h.path == "fused-infer" and capfd.readouterr().err == ""
    h.close()


# ---- 2. parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", PARITY)
def test_parity_with_the_checker(shape):
    F, Z = shape
    c = case(F, Z)
    h, _ = handle(c["dims"], c["flat"])
    assert h.path == "fused-infer"
    feats = dev(c["feats"])
    mask = np.zeros(F, dtype=np.uint8)
    mask[::3] = 1
    m1 = mask == 1
    dmask = dev(mask)
    pre = orc.renormalize(c["dec"], c["feats"][0], c["feats"][1])
    edge = np.abs(pre - np.round(pre)) < 1e-9 * np.maximum(1.0, np.abs(pre))      # on an integer boundary: the truncation may go either way
    for n in ROWS:
        what = (F, Z, n)
        # encode: float64 and float32 rows, with and without features
        assert rel(h.encode(dev(c["xn"][:n])).cpu().numpy(), c["z"][:n]) < TOL, what
        assert rel(h.encode(dev(c["raw"][:n]), features=feats).cpu().numpy(), c["z"][:n]) < TOL, what
        z = h.encode(dev(c["xn32"][:n]), out_dtype=torch.float64)
        assert z.dtype == torch.float64 and rel(z.cpu().numpy(), c["z_xn32"][:n]) < TOL, what
        assert rel(h.encode(dev(c["raw32"][:n]), features=feats, out_dtype=torch.float64).cpu().numpy(), c["z_raw32"][:n]) < TOL, what
        # decode into float64 with features and an int mask
        out = h.decode(dev(c["z"][:n]), features=feats, int_mask=dmask)
        assert out.dtype == torch.float64
        out = out.cpu().numpy()
        assert rel(out[:, ~m1], pre[:n][:, ~m1]) < TOL, what
        keep = ~edge[:n][:, m1]
        assert np.array_equal(out[:, m1][keep], np.trunc(pre[:n][:, m1])[keep]), what
        assert np.array_equal(out[:, m1], np.trunc(out[:, m1])), what
        # decode without features: into float64 at the bar; into float32 the same values rounded once (bit for bit)
        o64 = h.decode(dev(c["z"][:n]))
        assert o64.dtype == torch.float64 and rel(o64.cpu().numpy(), c["dec"][:n]) < TOL, what
        assert_same_bits(h.decode(dev(c["z"][:n]), out_dtype=torch.float32), o64.to(torch.float32), f"decode into float32 {what}")
        assert rel(h.decode(dev(c["z"][:n], torch.float32), out_dtype=torch.float64).cpu().numpy(), c["dec_z32"][:n]) < TOL, what
        # forward + loss, with and without the reconstruction
        lref = float(((c["fwd"][:n] - c["xn"][:n]) ** 2).sum() / F)
        rec, loss = h.forward_loss(dev(c["xn"][:n]))
        assert rec.dtype == torch.float64 and rel(rec.cpu().numpy(), c["fwd"][:n]) < TOL, what
        assert abs(loss.item() - lref) < TOL * lref, what
        none, loss0 = h.forward_loss(dev(c["xn"][:n]), want_recon=False)
        assert none is None and abs(loss0.item() - lref) < TOL * lref, what
        rec, loss = h.forward_loss(dev(c["raw"][:n]), features=feats)
        assert rel(rec.cpu().numpy(), c["fwd"][:n]) < TOL and abs(loss.item() - lref) < TOL * lref, what
    h.close()


# ---- 3. persistent loop and repeatability -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(129, 7), (625, 7)])
def test_grid_cap_and_repeatability(shape, monkeypatch):
    F, Z = shape
    c = case(F, Z)
    x, z = dev(c["xn"]), dev(c["z"])
    h, _ = handle(c["dims"], c["flat"])
    monkeypatch.setenv("BALER_AMD_F64_WIDE_WGS", "2")          # 300 rows = 5 groups of 64 rows on 2 workgroups: up to 3 groups each
    h2, _ = handle(c["dims"], c["flat"])
    monkeypatch.delenv("BALER_AMD_F64_WIDE_WGS")
    assert h.path == h2.path == "fused-infer"
    e, d = h.encode(x), h.decode(z)
    (r, l) = h.forward_loss(x)
    assert_same_bits(h2.encode(x), e, "encode, 2 workgroups")
    assert_same_bits(h2.decode(z), d, "decode, 2 workgroups")
    r2, l2 = h2.forward_loss(x)
    assert_same_bits(r2, r, "reconstruction, 2 workgroups")
    assert abs(l2.item() - l.item()) <= 1e-12 * abs(l.item())
    assert rel(e.cpu().numpy(), c["z"]) < TOL and rel(r2.cpu().numpy(), c["fwd"]) < TOL
    for hh in (h, h2):                                          # a repeated call: identical bits, loss included
        assert_same_bits(hh.encode(x), e, "encode again")
        assert_same_bits(hh.decode(z), d, "decode again")
    ra, la = h.forward_loss(x)
    assert_same_bits(ra, r, "reconstruction again")
    assert_same_bits(la, l, "loss again")
    h.close()
    h2.close()


# ---- 4. guard bands ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n", [((129, 7), 17), ((625, 7), 60)])
def test_guard_bands(shape, n):
    F, Z = shape
    c = case(F, Z)
    h, _ = handle(c["dims"], c["flat"])
    assert h.path == "fused-infer"
    mask = np.zeros(F, dtype=np.uint8)
    mask[::3] = 1
    for xd in (torch.float64, torch.float32):
        for raw in (False, True):
            ins = {"x": dev(c["raw" if raw else "xn"][:n], xd), "feats": dev(c["feats"]) if raw else None}
            both(f"encode {shape} {xd} features={raw}", lambda i, o: h.encode(i["x"], features=i["feats"], out=o["z"]), ins,
                 {"z": torch.zeros((n, Z), dtype=torch.float64, device="cuda")})
            both(f"forward_loss {shape} {xd} features={raw}", lambda i, o: forward_loss_raw(h, i["x"], i["feats"], o["recon"], o["loss"]), ins,
                 {"recon": torch.zeros((n, F), dtype=xd, device="cuda"), "loss": torch.zeros(1, dtype=torch.float64, device="cuda")})
    both(f"decode {shape} float64, features and int mask",
         lambda i, o: h.decode(i["z"], features=i["feats"], int_mask=i["mask"], out=o["out"]),
         {"z": dev(c["z"][:n]), "feats": dev(c["feats"]), "mask": dev(mask)}, {"out": torch.zeros((n, F), dtype=torch.float64, device="cuda")})
    both(f"decode {shape} float32", lambda i, o: h.decode(i["z"], out=o["out"]), {"z": dev(c["z"][:n], torch.float32)},
         {"out": torch.zeros((n, F), dtype=torch.float32, device="cuda")})
    h.close()


# ---- 5. 16-bit codes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_per_chunk", [None, "64"])
def test_sixteen_bit_codes(rows_per_chunk, monkeypatch):
    F, Z = 625, 7
    c = case(F, Z)
    if rows_per_chunk:
        monkeypatch.setenv("BALER_AMD_LAT32_ROWS", rows_per_chunk)      # 300 rows: five conversion chunks
    h, _ = handle(c["dims"], c["flat"])
    assert h.path == "fused-infer"
    x = dev(c["xn"])
    z64 = h.encode(x)
    for dt in (torch.float16, torch.bfloat16):
        z16 = h.encode(x, out_dtype=dt)
        assert_same_bits(z16, z64.to(torch.float32).to(dt), f"encode into {dt}")
        for od in (torch.float64, torch.float32):
            assert_same_bits(h.decode(z16, out_dtype=od), h.decode(z16.to(torch.float32), out_dtype=od), f"decode of {dt} codes into {od}")
        feats = dev(c["feats"])
        assert_same_bits(h.decode(z16, features=feats, out_dtype=torch.float64), h.decode(z16.to(torch.float32), features=feats, out_dtype=torch.float64),
                         f"decode of {dt} codes, un-normalised")
    h.close()


# ---- 6. fragments follow the parameters --------------------------------------------------------------------------------------------------
def test_fragments_follow_the_parameters(monkeypatch):
    F, Z = 625, 7
    c = case(F, Z)
    x = dev(c["xn"][:60])
    h, p = handle(c["dims"], c["flat"])
    monkeypatch.setenv("BALER_AMD_F64_WIDE", "0")
    hl, pl = handle(c["dims"], c["flat"])
    monkeypatch.delenv("BALER_AMD_F64_WIDE")
    assert h.path == "fused-infer" and hl.path == "generic"
    assert rel(h.encode(x).cpu().numpy(), c["z"][:60]) < TOL                     # fragments of the first parameters exist before the steps
    # training is not re-routed: fwd_bwd and train_step bit for bit those of the layer-wise handle
    g, gl = torch.full_like(p, 3.0), torch.full_like(pl, 3.0)
    h.fwd_bwd(x, g)
    hl.fwd_bwd(x, gl)
    assert_same_bits(g, gl, "fwd_bwd")
    m, v, ml, vl = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    for t in (1, 2):
        h.train_step(x, p, m, v, t, 1e-3)
        hl.train_step(x, pl, ml, vl, t, 1e-3)
    assert_same_bits(p, pl, "parameters after two train_steps")
    assert_same_bits(m, ml, "m")
    assert_same_bits(v, vl, "v")
    own = p.cpu().numpy()[:-1]
    assert rel(own, c["flat"]) > 1e-4                                            # the steps moved them
    assert rel(h.encode(x).cpu().numpy(), orc.encode(c["dims"], own, c["xn"][:60])) < TOL
    rec, _ = h.forward_loss(x)
    assert rel(rec.cpu().numpy(), orc.forward(c["dims"], own, c["xn"][:60])) < TOL
    # fwd_bwd + adam_step (the two-call step) leaves the copy stale as well
    h.fwd_bwd(x, g)
    h.adam_step(p, g, m, v, 3, 1e-3)
    own = p.cpu().numpy()[:-1]
    assert rel(h.decode(dev(c["z"][:60])).cpu().numpy(), orc.decode(c["dims"], own, c["z"][:60])) < TOL
    # a second load_params
    other = orc.formula_params(c["dims"], 7)
    h.load_params(torch.from_numpy(np.concatenate([other, [0.0]])).cuda())
    assert rel(h.encode(x).cpu().numpy(), orc.encode(c["dims"], other, c["xn"][:60])) < TOL
    h.close()
    hl.close()


# ---- 8. speed ------------------------------------------------------------------------------------------------------------------------
def test_faster_than_the_layerwise_kernels(monkeypatch):
    """CFD_dense_AE(2500, 25), 8,192 float64 rows: encode and decode on the fused kernels against the layer-wise kernels a
    BALER_AMD_F64_WIDE=0 handle runs (the code path of this shape before the class existed).  1.3 is noise clearance over the 10-13 %
    run-to-run variation DESIGN.md section 5 documents, not the expectation.  Measured: encode 0.387 ms against 0.593 ms = 1.53x, decode
    0.210 against 0.390 ms = 1.86x (below 2x at this width; DESIGN.md section 4.8 and profiles/f64_wide_infer.txt have every shape)."""
    F, Z, n = 2500, 25, 8192
    dims = orc.ae_dims(F, Z)
    flat = orc.formula_params(dims, 50 + F)
    h, _ = handle(dims, flat)
    monkeypatch.setenv("BALER_AMD_F64_WIDE", "0")
    hl, _ = handle(dims, flat)
    monkeypatch.delenv("BALER_AMD_F64_WIDE")
    assert h.path == "fused-infer" and hl.path == "generic"
    x = torch.rand((n, F), dtype=torch.float64, device="cuda")
    z = h.encode(x)
    zo, oo = torch.empty_like(z), torch.empty_like(x)
    t_enc, t_enc_l = _ms(lambda: h.encode(x, out=zo), 3), _ms(lambda: hl.encode(x, out=zo), 3)
    t_dec, t_dec_l = _ms(lambda: h.decode(z, out=oo), 3), _ms(lambda: hl.decode(z, out=oo), 3)
    print(f"fp64 ({F}, {Z}) x {n} rows: encode {t_enc:.3f} ms fused / {t_enc_l:.3f} ms layer-wise = {t_enc_l / t_enc:.2f}x; "
          f"decode {t_dec:.3f} / {t_dec_l:.3f} ms = {t_dec_l / t_dec:.2f}x")
    assert t_enc_l / t_enc >= 1.3 and t_dec_l / t_dec >= 1.3
    h.close()
    hl.close()
