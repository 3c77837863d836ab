"""The fp16 inference mode (BAMD_MODE_F16) on MI355X: encode / decode / forward + loss of the 24-column AE on
v_mfma_f32_16x16x32_f16, exact fp32 training on the same handle, and the float32 fallback of every other shape.

Tolerance rule -- nothing is fixed in advance.  For every comparison the handle's rel-L2 error against the fp64 oracle must be
  * at most 1.5 x the error of the numpy emulation of the contract (tests/test_f16_host.py: f16_chain) on the same inputs: two
    emulations with different fp32 accumulation orders differ by about 10 % in error (roundings flip at the LeakyReLU kink); the
    1.5 leaves room for that and nothing more;
  * at most 1/4 of the error of a "bf16" handle (existing code) on the same inputs: half of the 2^3 that three more significand
    bits give.
Every measured value is printed."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fpga_ref
import pjconv_ref
from baler_amd import native, synth
from baler_amd.modules import models
from guard_bands import POISON, assert_guards_intact, framed
from oracle import c_oracle as orc
from test_f16_host import c1_model, f16_chain, rel_l2

pytestmark = pytest.mark.gpu

ZS = (15, 12, 10, 8, 6, 5, 4, 3, 2)
NS = (1, 15, 64, 65, 511, 513, 4100)      # pass, wave and workgroup edges: 64 rows per wave pass, 8 waves per workgroup
N_MAX = NS[-1]
N_BIG = 131072 + 77                       # the second round of a full grid (256 workgroups x 512 rows)
TOL32 = 1e-5


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def make_handle(dims, flat, mode, act="leaky_relu"):
    h = native.Handle(dims, mode, act=act)
    p = dev(np.concatenate([flat, [0.0]]), torch.float32)
    h.load_params(p)
    return h, p


def host(t):
    return t.cpu().numpy().astype(np.float64)


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def check_rule(what, got, emu, bf, ref):
    e, ee, eb = rel_l2(got, ref), rel_l2(emu, ref), rel_l2(bf, ref)
    print(f"{what}: fp16 {e:.3e}  emulation {ee:.3e} (x{e / max(ee, 1e-300):.2f})  bf16 {eb:.3e} (1/{eb / max(e, 1e-300):.1f})")
    assert e <= 1.5 * ee, f"{what}: fp16 error {e:.3e} above 1.5 x the emulation's {ee:.3e}"
    assert e <= eb / 4, f"{what}: fp16 error {e:.3e} above 1/4 of the bf16 handle's {eb:.3e}"


@functools.lru_cache(maxsize=None)
def case(z, n=N_MAX):
    """One model per latent size with its rows, the oracle's results and the emulation's -- computed once, read by every test."""
    dims = orc.ae_dims(24, z)
    flat = orc.formula_params(dims, 41 + z)
    x = np.random.default_rng(100 + z).random((n, 24))
    zo = orc.encode(dims, flat, x)
    ro = orc.decode(dims, flat, zo)          # = the oracle's forward(x)
    emu_z = f16_chain(dims, flat, x, 0, 4)
    c = dict(dims=dims, flat=flat, x=x, zo=zo, ro=ro, emu_z=emu_z, emu_d=f16_chain(dims, flat, zo, 4, 8),
             emu_f=f16_chain(dims, flat, emu_z, 4, 8))      # forward: the float32 latent is rounded again by the decoder's loader
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def handles(c):
    return make_handle(c["dims"], c["flat"], "fp16")[0], make_handle(c["dims"], c["flat"], "bf16")[0]


def loss_of(recon, x, dt):
    """The kernel's loss from its own reconstruction: float64 sum of (float32 recon - float32(x))^2 / 24."""
    xf = x.astype(np.float32).astype(np.float64)
    return float(((host(recon.to(torch.float32)) - xf) ** 2).sum() / 24)


def run_all(h, c, n, dt):
    x, zo = dev(c["x"][:n], dt), dev(c["zo"][:n], dt)
    recon, loss = h.forward_loss(x)
    return h.encode(x), h.decode(zo), recon, loss.item()


@pytest.mark.parametrize("z", ZS)
def test_inference_every_latent_size_and_row_edge(z):
    c = case(z)
    h, hb = handles(c)
    assert h.compute_mode == native.MODE_F16 and h.path == "f16" and h.param_dtype == torch.float32
    assert hb.path == "bf16"
    for dt in (torch.float32, torch.float64):
        for n in NS:
            ze, de, re_, loss = run_all(h, c, n, dt)
            zb, db, rb, _ = run_all(hb, c, n, dt)
            assert ze.dtype == dt and de.dtype == dt and re_.dtype == dt and ze.shape == (n, z) and de.shape == (n, 24)
            tag = f"z={z} n={n} {str(dt)[6:]}"
            check_rule(f"encode {tag}", host(ze), c["emu_z"][:n], host(zb), c["zo"][:n])
            check_rule(f"decode {tag}", host(de), c["emu_d"][:n], host(db), c["ro"][:n])
            check_rule(f"forward {tag}", host(re_), c["emu_f"][:n], host(rb), c["ro"][:n])
            if dt == torch.float32:      # (a float64 reconstruction is the widened float32 one)
                want = loss_of(re_, c["x"][:n], dt)
                assert abs(loss - want) <= 1e-9 * want, f"loss {tag}: {loss} vs {want} from the reconstruction"
            _, loss2 = h.forward_loss(dev(c["x"][:n], dt), want_recon=False)
            assert loss2.item() == loss
    assert h.encode(dev(c["x"][:0])).shape == (0, z)


def test_second_grid_round_every_row_against_the_oracle():
    c = case(15, N_BIG)
    h, hb = handles(c)
    ze, de, re_, loss = run_all(h, c, N_BIG, torch.float64)
    zb, db, rb, _ = run_all(hb, c, N_BIG, torch.float64)
    check_rule("encode", host(ze), c["emu_z"], host(zb), c["zo"])
    check_rule("decode", host(de), c["emu_d"], host(db), c["ro"])
    check_rule("forward", host(re_), c["emu_f"], host(rb), c["ro"])
    # every row, not the aggregate alone: the worst row of the second round is no worse than the worst row of the first
    row_err = np.linalg.norm(host(ze) - c["zo"], axis=1) / np.linalg.norm(c["zo"], axis=1)
    emu_err = np.linalg.norm(c["emu_z"] - c["zo"], axis=1) / np.linalg.norm(c["zo"], axis=1)
    print(f"worst row: fp16 {row_err.max():.3e} (row {row_err.argmax()}), emulation {emu_err.max():.3e}")
    assert row_err.max() <= 1.5 * emu_err.max()
    assert np.isfinite(host(de)).all() and np.isfinite(host(re_)).all()


def test_trained_model_normalise_on_load_and_renormalise_with_int_mask():
    """The C1 fixture on its own kind of data: raw rows normalised inside the encode, the decode un-normalised and truncated."""
    dims, flat = c1_model()
    h, hb = make_handle(dims, flat, "fp16")[0], make_handle(dims, flat, "bf16")[0]
    raw = synth.cms_rows(3001)
    feats = orc.find_minmax(raw)
    xn = orc.normalize(raw)
    zo = orc.encode(dims, flat, xn)
    ro = orc.decode(dims, flat, zo)
    emu_z, emu_d = f16_chain(dims, flat, xn, 0, 4), f16_chain(dims, flat, zo, 4, 8)
    for dt in (torch.float64, torch.float32):
        x = dev(raw, dt)
        rawd = host(x)                      # float32 rows: the kernel normalises the float32 values (in float64)
        xnd = (rawd - feats[0]) / feats[1]
        ref = zo if dt == torch.float64 else orc.encode(dims, flat, xnd)
        emu = emu_z if dt == torch.float64 else f16_chain(dims, flat, xnd, 0, 4)
        check_rule(f"encode + normalise {str(dt)[6:]}", host(h.encode(x, features=dev(feats))), emu,
                   host(hb.encode(x, features=dev(feats))), ref)
    check_rule("encode (normalised rows)", host(h.encode(dev(xn))), emu_z, host(hb.encode(dev(xn))), zo)
    check_rule("decode", host(h.decode(dev(zo))), emu_d, host(hb.decode(dev(zo))), ro)
    mask = np.array([t == "int" for t in synth.CMS_TYPE_LIST], dtype=np.uint8)
    md = torch.from_numpy(mask).cuda()
    out = host(h.decode(dev(zo), features=dev(feats), int_mask=md))
    outb = host(hb.decode(dev(zo), features=dev(feats), int_mask=md))
    want = orc.renormalize(ro, feats[0], feats[1])
    emu_out = emu_d.astype(np.float64) * feats[1] + feats[0]
    fl = mask == 0
    check_rule("decode + un-normalise (float columns)", out[:, fl], emu_out[:, fl], outb[:, fl], want[:, fl])
    assert np.array_equal(out[:, ~fl], np.trunc(out[:, ~fl]))
    # the int columns: what the kernel's own float32 reconstruction truncates to
    plain = host(h.decode(dev(zo, torch.float32)))
    assert np.array_equal(out[:, ~fl], np.trunc(plain * feats[1] + feats[0])[:, ~fl])


def test_not_a_fallback_and_repeatable():
    c = case(15)
    h, _ = handles(c)
    h32 = make_handle(c["dims"], c["flat"], "fp32")[0]
    x = dev(c["x"])
    z16, z32 = h.encode(x), h32.encode(x)
    assert not torch.equal(z16, z32)                                   # binary16 operands: not the float32 kernels
    assert rel_l2(host(z32), c["zo"]) < TOL32 < rel_l2(host(z16), c["zo"])
    zo = dev(c["zo"])
    d, (r, l) = h.decode(zo), h.forward_loss(x)
    for _ in range(3):
        assert same_bits(h.encode(x), z16) and same_bits(h.decode(zo), d)
        r2, l2 = h.forward_loss(x)
        assert same_bits(r2, r) and l2.item() == l.item()


@pytest.mark.parametrize("z", [15, 8])      # latent 8: the aligned 16-byte code load
def test_sixteen_bit_codes(z):
    c = case(z)
    h, _ = handles(c)
    feats = dev(np.stack([np.linspace(-3, 3, 24), np.linspace(0.5, 40, 24)]))
    mask = torch.from_numpy((np.arange(24) % 3 == 0).astype(np.uint8)).cuda()
    for n in (513, 4100):
        x = dev(c["x"][:n], torch.float32)
        z32 = h.encode(x, out_dtype=torch.float32)
        for h16 in (torch.float16, torch.bfloat16):
            z16 = h.encode(x, out_dtype=h16)
            assert z16.dtype == h16 and same_bits(z16, z32.to(h16)), f"encode {h16} n={n}"
            wide = z16.to(torch.float32)
            assert same_bits(h.decode(z16), h.decode(wide)), f"decode {h16} n={n}"
            assert same_bits(h.decode(z16, out_dtype=torch.float64), h.decode(wide, out_dtype=torch.float64))
            assert same_bits(h.decode(z16, features=feats, int_mask=mask, out_dtype=torch.float64),
                             h.decode(wide, features=feats, int_mask=mask, out_dtype=torch.float64))
        # float16 codes enter the chain without a rounding: decoding them is decoding the emulation's input exactly
        z16 = h.encode(x, out_dtype=torch.float16)
        emu = f16_chain(c["dims"], c["flat"], host(z16), 4, 8)
        ref = orc.decode(c["dims"], c["flat"], host(z16))
        assert rel_l2(host(h.decode(z16)), ref) <= 1.5 * rel_l2(emu, ref)


@pytest.mark.parametrize("z", [15, 8])
def test_guard_bands(z):
    """Encode and decode at ragged row counts into poisoned arenas, out of NaN-framed inputs: nothing outside the block is written,
    and nothing outside it is read into a result."""
    c = case(z)
    h, _ = handles(c)
    for n, lead in ((1, 3), (65, 1), (513, 7), (4099, 2)):
        for dt, zdt in ((torch.float32, torch.float32), (torch.float64, torch.float64), (torch.float32, torch.float16)):
            x, zc = dev(c["x"][:n], dt), dev(c["zo"][:n], dt).to(zdt)
            want_z, want_d = h.encode(x, out_dtype=zdt), h.decode(zc, out_dtype=dt)
            xv, _ = framed(x, lead, fill="nan")
            zv, _ = framed(zc, lead, fill="nan")
            zout, zarena = framed(torch.zeros((n, z), dtype=zdt, device="cuda"), lead, fill=POISON)
            dout, darena = framed(torch.zeros((n, 24), dtype=dt, device="cuda"), lead, fill=POISON)
            h.encode(xv, out=zout)
            h.decode(zv, out=dout)
            what = f"z={z} n={n} {dt} codes {zdt}"
            assert_guards_intact(zarena, lead, n, "encode " + what)
            assert_guards_intact(darena, lead, n, "decode " + what)
            assert same_bits(zout, want_z) and same_bits(dout, want_d), what


def test_overflow_stays_in_its_row():
    """Defined behaviour, not a fault: 1e6 in one column of row 37 rounds to +inf as a binary16 layer input whatever the weights
    are; every output of that row is non-finite and every other row is what it is without it."""
    c = case(15)
    h, _ = handles(c)
    x = dev(c["x"][:130], torch.float32)
    clean = x.clone()
    clean[37] = 0.0
    x[37, 5] = 1e6
    for name, fn in (("encode", h.encode), ("forward", lambda t: h.forward_loss(t)[0])):
        got, ref = fn(x), fn(clean)
        assert not torch.isfinite(got[37]).any(), f"{name}: row 37 has finite outputs"
        keep = torch.arange(130, device="cuda") != 37
        assert same_bits(got[keep], ref[keep]), f"{name}: another row changed"
        assert torch.isfinite(got[keep]).all()
    zc = dev(c["zo"][:130], torch.float32)
    zclean = zc.clone()
    zclean[37] = 0.0
    zc[37, 2] = 1e6
    got, ref = h.decode(zc), h.decode(zclean)
    keep = torch.arange(130, device="cuda") != 37
    assert not torch.isfinite(got[37]).any() and same_bits(got[keep], ref[keep])


@pytest.mark.parametrize("n", [512, 20000])
def test_training_is_the_fp32_handles_bit_for_bit(n):
    c = case(15)
    x = dev(np.random.default_rng(9).random((3 * n, 24)), torch.float32)
    state = {}
    for mode in ("fp16", "fp32"):
        h, p = make_handle(c["dims"], c["flat"], mode)
        g1 = torch.zeros_like(p)
        h.fwd_bwd(x[:n], g1)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        z_before = h.encode(x[:n])
        h.train_step(x[:n], p, m, v, 1, 1e-3)
        after_step = (p.clone(), m.clone(), v.clone())
        z_step = h.encode(x[:n])
        g2 = torch.zeros_like(p)
        steps = h.train_epoch(x, n, p, m, v, 2, 1e-3, grads=g2)
        assert steps == 3
        h.adam_step(p, g2, m, v, 5, 1e-3)
        state[mode] = dict(h=h, g1=g1, after_step=after_step, g2=g2, p=p.clone(), m=m.clone(), v=v.clone(), z_before=z_before,
                           z_step=z_step, z_end=h.encode(x[:n]))
    a, b = state["fp16"], state["fp32"]
    assert same_bits(a["g1"], b["g1"]), "fwd_bwd"
    for k in range(3):
        assert same_bits(a["after_step"][k], b["after_step"][k]), f"train_step tensor {k}"
    assert same_bits(a["g2"], b["g2"]), "train_epoch gradients"
    for k in ("p", "m", "v"):
        assert same_bits(a[k], b[k]), f"train_epoch + adam_step {k}"
    # the steps reached the binary16 fragments (lazily re-rounded), and inference at the new parameters meets the rule
    assert not torch.equal(a["z_before"], a["z_step"]) and not torch.equal(a["z_step"], a["z_end"])
    hb = make_handle(c["dims"], c["flat"], "bf16")[0]
    xs = host(x[:n])
    for tag, params, got in (("after train_step", a["after_step"][0], a["z_step"]), ("after the epoch", a["p"], a["z_end"])):
        flat_new = host(params)[:-1]
        hb.load_params(params)
        ref = orc.encode(c["dims"], flat_new, xs)
        check_rule(f"encode {tag} n={n}", host(got), f16_chain(c["dims"], flat_new, xs, 0, 4), host(hb.encode(x[:n])), ref)
    # load_params reaches the fragments too
    h = a["h"]
    h.load_params(dev(np.concatenate([c["flat"], [0.0]]), torch.float32))
    assert same_bits(h.encode(x[:n]), a["z_before"])


def test_activation_means_are_the_fp32_handles():
    c = case(15)
    x = dev(c["x"][:700], torch.float32)
    a = make_handle(c["dims"], c["flat"], "fp16")[0].activation_means(x)
    b = make_handle(c["dims"], c["flat"], "fp32")[0].activation_means(x)
    assert same_bits(a, b)


NOTICE = "BAMD_MODE_F16 has kernels for the 24-column AE"


@pytest.mark.parametrize("shape", ["ae-30-8", "ae-2500-25", "relu", "pjconv"])
def test_fallback_shapes_are_float32_handles_with_a_notice(shape, capfd, monkeypatch):
    monkeypatch.delenv("BALER_AMD_QUIET", raising=False)
    rng = np.random.default_rng(3)
    if shape == "pjconv":
        z = 10
        flat = models.pj_conv_init(z).numpy().astype(np.float64)
        h = native.Handle.pj_conv(z, "fp16")
        h.load_params(dev(np.concatenate([flat, [0.0]]), torch.float32))
        x = rng.random((5, 784))
        ref = pjconv_ref.encode(z, flat, x)
    elif shape == "relu":
        dims = fpga_ref.dims(16, 4)
        flat = orc.formula_params(dims, 5)
        h, _ = make_handle(dims, flat, "fp16", act="relu")
        x = rng.random((300, 16))
        ref = fpga_ref.encode(dims, flat, x)
    else:
        F, Z = (30, 8) if shape == "ae-30-8" else (2500, 25)
        dims = orc.ae_dims(F, Z)
        flat = orc.formula_params(dims, 5)
        h, _ = make_handle(dims, flat, "fp16")
        x = rng.random((300 if F == 30 else 40, F))
        ref = orc.encode(dims, flat, x)
    err = capfd.readouterr().err
    assert NOTICE in err and "computes in float32" in err and err.count(NOTICE) == 1, err
    assert h.mode == native.MODE_F16 and h.compute_mode == native.MODE_F32 and h.path != "f16"
    assert int(native.lib().bamd_mode_of(h._h)) == native.MODE_F32
    got = host(h.encode(dev(x, torch.float32)))
    e = max(rel_l2(got, ref), float(np.abs(got - ref).max() / np.abs(ref).max()))
    print(f"{shape}: encode error {e:.3e}")
    assert e < TOL32
    # silent under BALER_AMD_QUIET=1
    monkeypatch.setenv("BALER_AMD_QUIET", "1")
    if shape == "pjconv":
        native.Handle.pj_conv(10, "fp16")
    else:
        native.Handle(h.dims, "fp16", act=h.act)
    assert NOTICE not in capfd.readouterr().err


def test_create_through_the_c_abi():
    L = native.lib()
    h = ctypes.c_void_p()
    dims = (ctypes.c_int * 9)(*orc.ae_dims(24, 15))
    assert L.bamd_create(dims, 8, native.MODE_F16, 0, ctypes.byref(h)) == 0
    assert L.bamd_mode_of(h) == 3 and L.bamd_path_of(h) == 4
    L.bamd_destroy(h)
    assert L.bamd_create(dims, 8, 4, 0, ctypes.byref(h)) == -1 and b"unknown mode" in L.bamd_last_error()
    assert L.bamd_abi_version() == 1


def _ms(fn, reps, warm_ms=30.0, samples=5):
    """The timing method of tests/test_gpu_perf_floor.py."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    for _ in range(min(200, int(warm_ms / max(e0.elapsed_time(e1), 1e-3)))):
        fn()
    got = []
    for _ in range(samples):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        got.append(e0.elapsed_time(e1) / reps)
    return sorted(got)[len(got) // 2]


def test_speed_is_the_bf16_modes():
    """Same MFMA count, same bytes, no more VALU instructions than the bf16 kernels: at most 1.10 x their time (the 10 % is the
    clock-ramp variation DESIGN.md section 5 documents).  The two handles are timed alternately in one process."""
    c = case(15)
    h, hb = handles(c)
    n = 1_000_000
    x = torch.rand((n, 24), dtype=torch.float64, device="cuda")
    z = h.encode(x)
    zout, dout = torch.empty_like(z), torch.empty_like(x)
    t = {"fp16": [[], []], "bf16": [[], []]}
    for _ in range(3):
        for name, hh in (("bf16", hb), ("fp16", h)):
            t[name][0].append(_ms(lambda: hh.encode(x, out=zout), 5))
            t[name][1].append(_ms(lambda: hh.decode(z, out=dout), 5))
    med = {k: [sorted(s)[1] for s in v] for k, v in t.items()}
    print(f"1M float64 rows: encode fp16 {med['fp16'][0]:.4f} ms  bf16 {med['bf16'][0]:.4f} ms;  "
          f"decode fp16 {med['fp16'][1]:.4f} ms  bf16 {med['bf16'][1]:.4f} ms")
    assert med["fp16"][0] <= 1.10 * med["bf16"][0], "encode"
    assert med["fp16"][1] <= 1.10 * med["bf16"][1], "decode"
