"""The fp16x3 inference mode (BAMD_MODE_F16X3) on MI355X: encode / decode / forward + loss of the 24-column AE at fp32 accuracy on
v_mfma_f32_16x16x32_f16 (three binary16 products per tile), exact fp32 training on the same handle, and the float32 fallback of
every other shape.

Tolerances.
  * The hard bar is the project's fp32 bar: rel() = max(rel-L2, max-norm) over the whole tensor below 1e-5 against the fp64 oracle.
  * Against a "fp32" handle on the same inputs: the ratio (rel-L2 error of fp16x3) / (rel-L2 error of fp32) is printed for every
    case, with the worst one seen so far.  WORST_RATIO is the largest one measured on an MI355X over every case of this file: 1.22
    (encode, z = 2, ONE float32 row, where a single rounding decides); every case asserts 1.5 x that, the 1.5 being the project's
    allowance for accumulation-order variation.  On 64 rows and more the measured ratio is 0.40 - 0.66: the MFMA's fp32 sum of exact
    binary16 products is closer to the oracle than the fp32 kernels' chain of rounded fp32 products.  The NumPy emulation
    (tests/f16x3_ref.py, float32 sums) gives 1.02 - 1.11 on 4,096 rows.
Kernel geometry: 32 rows per wave pass (kMB = 2), 8 waves = 256 rows per workgroup, at most 256 workgroups per launch."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import f16x3_ref as ref
import fpga_ref
import pjconv_ref
from baler_amd import native, synth
from baler_amd.modules import models
from guard_bands import POISON, assert_guards_intact, framed
from oracle import c_oracle as orc
from test_f16x3_host import c1_model

pytestmark = pytest.mark.gpu

ZS = (15, 12, 10, 8, 6, 5, 4, 3, 2)
# one row, a ragged tile, the 64-row pass of the other 16-bit modes and some hundreds and thousands of rows, each +-1; and the pass
# (32 rows) and workgroup (256 rows) edges of this mode's kMB = 2
NS = (1, 15, 31, 32, 33, 64, 65, 255, 256, 257, 511, 513, 4100)
N_MAX = NS[-1]
N_BIG = 131072 + 77                       # past a full grid (256 workgroups x 256 rows): second and third rounds
TOL32 = 1e-5
WORST_RATIO = 1.22                        # measured on an MI355X: see the module docstring and DESIGN.md section 15
seen = {"ratio": 0.0, "what": ""}


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


def check_rule(what, got, got32, want):
    """got: the fp16x3 handle's result, got32: the fp32 handle's on the same inputs, want: the fp64 oracle's."""
    e, e32, em = ref.rel_l2(got, want), ref.rel_l2(got32, want), ref.rel(got, want)
    ratio = e / max(e32, 1e-300)
    if ratio > seen["ratio"]:
        seen.update(ratio=ratio, what=what)
    print(f"{what}: fp16x3 {e:.3e} (rel() {em:.3e})  fp32 handle {e32:.3e}  ratio {ratio:.2f}   [worst so far {seen['ratio']:.2f}: {seen['what']}]")
    assert em < TOL32, f"{what}: rel() {em:.3e} misses the fp32 bar"
    assert e <= 1.5 * WORST_RATIO * e32, f"{what}: error {e:.3e} above {1.5 * WORST_RATIO} x the fp32 handle's {e32:.3e}"


@functools.lru_cache(maxsize=None)
def case(z, n=N_MAX):
    """One model per latent size with its rows and the oracle's results -- computed once, read by every test."""
    dims = orc.ae_dims(24, z)
    flat = orc.formula_params(dims, 41 + z)
    x = np.random.default_rng(100 + z).random((n, 24))
    zo = orc.encode(dims, flat, x)
    c = dict(dims=dims, flat=flat, x=x, zo=zo, ro=orc.decode(dims, flat, zo))      # ro = the oracle's forward(x)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def handles(c):
    return make_handle(c["dims"], c["flat"], "fp16x3")[0], make_handle(c["dims"], c["flat"], "fp32")[0]


def run_all(h, c, n, dt):
    x, zo = dev(c["x"][:n], dt), dev(c["zo"][:n], dt)
    recon, loss = h.forward_loss(x)
    return h.encode(x), h.decode(zo), recon, loss.item()


@pytest.mark.parametrize("z", ZS)
def test_inference_every_latent_size_and_row_edge(z):
    c = case(z)
    h, h32 = handles(c)
    assert h.compute_mode == native.MODE_F16X3 == 5 and h.path == "f16x3" and h.param_dtype == torch.float32
    assert h32.path == "fused"
    for dt in (torch.float32, torch.float64):
        for n in NS:
            ze, de, re_, loss = run_all(h, c, n, dt)
            z32, d32, r32, _ = run_all(h32, c, n, dt)
            assert ze.dtype == dt and de.dtype == dt and re_.dtype == dt and ze.shape == (n, z) and de.shape == (n, 24)
            tag = f"z={z} n={n} {str(dt)[6:]}"
            check_rule(f"encode {tag}", host(ze), host(z32), c["zo"][:n])
            check_rule(f"decode {tag}", host(de), host(d32), c["ro"][:n])
            check_rule(f"forward {tag}", host(re_), host(r32), c["ro"][:n])
            # the loss is taken between the float32 reconstruction and the row as the kernel saw it: rounded once to float32
            xf = c["x"][:n].astype(np.float32).astype(np.float64)
            want = float(((host(re_) - xf) ** 2).sum() / 24)
            assert abs(loss - want) <= 1e-9 * want, f"loss {tag}: {loss} vs {want} from the reconstruction"
            _, loss2 = h.forward_loss(dev(c["x"][:n], dt), want_recon=False)
            assert loss2.item() == loss
    assert h.encode(dev(c["x"][:0])).shape == (0, z) and h.decode(dev(c["zo"][:0])).shape == (0, 24)


def test_later_grid_rounds_every_row_against_the_oracle():
    """More than one pass per wave (over 65,536 rows).  Both row dtypes: the float32 rows' prefetch of the next pass sits elsewhere in
    the encoder than the float64 rows'; and the 16-bit codes' decode, which has a loader of its own."""
    c = case(15, N_BIG)
    h, h32 = handles(c)
    xf = c["x"].astype(np.float32).astype(np.float64)
    for dt in (torch.float32, torch.float64):
        ze, de, re_, loss = run_all(h, c, N_BIG, dt)
        z32, d32, r32, _ = run_all(h32, c, N_BIG, dt)
        tag = str(dt)[6:]
        check_rule(f"encode {tag}", host(ze), host(z32), c["zo"])
        check_rule(f"decode {tag}", host(de), host(d32), c["ro"])
        check_rule(f"forward {tag}", host(re_), host(r32), c["ro"])
        want = float(((host(re_) - xf) ** 2).sum() / 24)
        assert abs(loss - want) <= 1e-9 * want, f"loss {tag}: {loss} vs {want} from the reconstruction"
        assert h.forward_loss(dev(c["x"], dt), want_recon=False)[1].item() == loss
    for h16 in (torch.float16, torch.bfloat16):
        z16 = dev(c["zo"], torch.float32).to(h16)
        # the float32 codes' decode is held to the oracle on every row above; the 16-bit loader must give its bits on the widened codes
        assert same_bits(h.decode(z16), h.decode(z16.to(torch.float32))), f"decode {h16}"
    # every row, not the aggregate alone: the worst row of the whole table is no worse than 1.5 x WORST_RATIO x the fp32 handle's worst
    norm = np.linalg.norm(c["ro"], axis=1)
    row_err = np.linalg.norm(host(de) - c["ro"], axis=1) / norm
    row32 = np.linalg.norm(host(d32) - c["ro"], axis=1) / norm
    print(f"worst decoded row: fp16x3 {row_err.max():.3e} (row {row_err.argmax()}), fp32 handle {row32.max():.3e}")
    assert row_err.max() <= 1.5 * WORST_RATIO * row32.max() and row_err.max() < TOL32


def test_trained_model_normalise_on_load_and_renormalise_with_int_mask():
    """The C1 fixture on its own kind of data: raw rows normalised (in float64) inside the encode; the un-normalise + int-mask
    epilogue of the decode is NumPy's arithmetic applied to the handle's own float32 decode, bit for bit."""
    dims, flat = c1_model()
    h, h32 = make_handle(dims, flat, "fp16x3")[0], make_handle(dims, flat, "fp32")[0]
    raw = synth.cms_rows(3001)
    feats = orc.find_minmax(raw)
    xn = orc.normalize(raw)
    zo = orc.encode(dims, flat, xn)
    ro = orc.decode(dims, flat, zo)
    for dt in (torch.float64, torch.float32):
        x = dev(raw, dt)
        xnd = (host(x) - feats[0]) / feats[1]      # float32 rows: the kernel normalises the float32 values (in float64)
        want = zo if dt == torch.float64 else orc.encode(dims, flat, xnd)
        check_rule(f"encode + normalise {str(dt)[6:]}", host(h.encode(x, features=dev(feats))), host(h32.encode(x, features=dev(feats))), want)
        recon, loss = h.forward_loss(x, features=dev(feats))
        recon32, _ = h32.forward_loss(x, features=dev(feats))
        check_rule(f"forward + normalise {str(dt)[6:]}", host(recon), host(recon32), ro if dt == torch.float64 else orc.forward(dims, flat, xnd))
        # the loss: against the row normalised in float64 and rounded once to float32, as the encoder read it
        want_loss = float(((host(recon) - xnd.astype(np.float32).astype(np.float64)) ** 2).sum() / 24)
        assert abs(loss.item() - want_loss) <= 1e-9 * want_loss, f"loss + normalise {dt}: {loss.item()} vs {want_loss}"
        assert h.forward_loss(x, features=dev(feats), want_recon=False)[1].item() == loss.item()
    check_rule("decode", host(h.decode(dev(zo))), host(h32.decode(dev(zo))), ro)
    mask = np.array([t == "int" for t in synth.CMS_TYPE_LIST], dtype=np.uint8)
    md = torch.from_numpy(mask).cuda()
    plain = host(h.decode(dev(zo, torch.float32)))
    want = plain * feats[1] + feats[0]
    want[:, mask == 1] = np.trunc(want[:, mask == 1])
    for zdt in (torch.float32, torch.float64):      # (float64 codes are rounded to float32 first: the same decode)
        out = host(h.decode(dev(zo, torch.float32).to(zdt), features=dev(feats), int_mask=md, out_dtype=torch.float64))
        assert np.array_equal(out, want), f"epilogue, codes {zdt}"
    assert np.array_equal(host(h.decode(dev(zo, torch.float32), features=dev(feats), out_dtype=torch.float64)), plain * feats[1] + feats[0])


def test_not_a_fallback_and_repeatable():
    c = case(15)
    h, h32 = handles(c)
    x, zo = dev(c["x"]), dev(c["zo"])
    z3, z32 = h.encode(x), h32.encode(x)
    assert not torch.equal(z3, z32)                                    # another summation: not the float32 kernels
    d, (r, l) = h.decode(zo), h.forward_loss(x)
    for _ in range(3):
        assert same_bits(h.encode(x), z3) and same_bits(h.decode(zo), d)
        r2, l2 = h.forward_loss(x)
        assert same_bits(r2, r) and l2.item() == l.item()
    # a second handle with the same parameters: the same bits (nothing depends on allocation or launch history)
    h2, _ = make_handle(c["dims"], c["flat"], "fp16x3")
    assert same_bits(h2.encode(x), z3) and same_bits(h2.decode(zo), d)


@pytest.mark.parametrize("z", [15, 8])      # latent 8: the aligned 16-byte code load
def test_sixteen_bit_codes(z):
    c = case(z)
    h, _ = handles(c)
    feats = dev(np.stack([np.linspace(-3, 3, 24), np.linspace(0.5, 40, 24)]))
    mask = torch.from_numpy((np.arange(24) % 3 == 0).astype(np.uint8)).cuda()
    for n in (33, 513, 4100):
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
            # the codes are the decoder's exact input: decoding them meets the fp32 bar against the oracle's decode of THEM
            assert ref.rel(host(h.decode(z16)), orc.decode(c["dims"], c["flat"], host(wide))) < TOL32


@pytest.mark.parametrize("z", [15, 2])
def test_guard_bands(z):
    """Encode and decode at ragged row counts into poisoned arenas, out of NaN-framed inputs: nothing outside the block is written,
    and nothing outside it is read into a result."""
    c = case(z)
    h, _ = handles(c)
    for n, lead in ((1, 3), (33, 1), (257, 7), (4099, 2)):
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
    """Defined behaviour, not a fault.  A weight of 1e5 has no binary16 image itself (its hi part is +inf, which meets every row); what
    CAN single out a row is a large weight in range meeting a large value of one row: en1's weight (0, 5) = 1e4 takes row 37, whose
    column 5 holds 10, to an activation of 1e5 -- beyond 65504, so its hi part is +inf at the next split -- and leaves every other row
    (column 5 below 1) in range.  Every output of row 37 is non-finite; every other row is what it is without that row, bit for bit.
    The same for a value beyond the range in a row or in a latent code."""
    c = case(15)
    flat = c["flat"].copy()
    flat[0 * 24 + 5] = 1e4
    h, _ = make_handle(c["dims"], flat, "fp16x3")
    x = dev(c["x"][:130], torch.float32)
    clean = x.clone()
    clean[37] = 0.0
    keep = torch.arange(130, device="cuda") != 37
    for value in (10.0, 1e6):
        x[37, 5] = value
        for name, fn in (("encode", h.encode), ("forward", lambda t: h.forward_loss(t)[0])):
            got, want = fn(x), fn(clean)
            assert not torch.isfinite(got[37]).any(), f"{name}: row 37 has finite outputs"
            assert same_bits(got[keep], want[keep]), f"{name}: another row changed"
            assert torch.isfinite(got[keep]).all()
    # a WEIGHT beyond the range is another matter: the hi part of 1e5 is +inf, and every row meets it
    flat[0 * 24 + 5] = 1e5
    hw, _ = make_handle(c["dims"], flat, "fp16x3")
    for got in (hw.encode(clean), hw.forward_loss(clean)[0]):
        assert not torch.isfinite(got).any(), "a weight of 1e5 left an output finite"
    zc = dev(c["zo"][:130], torch.float32)
    zclean = zc.clone()
    zclean[37] = 0.0
    zc[37, 2] = 1e6
    got, want = h.decode(zc), h.decode(zclean)
    assert not torch.isfinite(got[37]).any() and same_bits(got[keep], want[keep]) and torch.isfinite(got[keep]).all()


def test_range_check_of_compress_and_decompress_covers_the_mode():
    """compress / decompress count the rows with finite input and non-finite output on the device and refuse before writing."""
    from baler_amd.modules import helper
    c = case(15)
    h, h32 = handles(c)
    x = dev(c["x"][:64], torch.float32)
    x[5, 3] = 1e6
    out = h.encode(x)
    with pytest.raises(ValueError, match="BALER_AMD_MODE=fp16x3: 1 rows"):
        helper._check_fp16_mode_range(h, x, out, 1, "encoded")
    helper._check_fp16_mode_range(h, x[:5], out[:5], 1, "encoded")           # rows in range pass
    helper._check_fp16_mode_range(h32, x, h32.encode(x), 1, "encoded")       # a float32 handle is not checked (and has nothing to report)


@pytest.mark.parametrize("n", [512, 20000])
def test_training_is_the_fp32_handles_bit_for_bit(n):
    c = case(15)
    x = dev(np.random.default_rng(9).random((3 * n, 24)), torch.float32)
    state = {}
    for mode in ("fp16x3", "fp32"):
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
    a, b = state["fp16x3"], state["fp32"]
    assert same_bits(a["g1"], b["g1"]), "fwd_bwd"
    for k in range(3):
        assert same_bits(a["after_step"][k], b["after_step"][k]), f"train_step tensor {k}"
    assert same_bits(a["g2"], b["g2"]), "train_epoch gradients"
    for k in ("p", "m", "v"):
        assert same_bits(a[k], b[k]), f"train_epoch + adam_step {k}"
    # the steps reached the split fragments (re-made lazily): encode after a step is encode on a fresh handle with the stepped parameters
    assert not torch.equal(a["z_before"], a["z_step"]) and not torch.equal(a["z_step"], a["z_end"])
    for tag, params, got in (("after train_step", a["after_step"][0], a["z_step"]), ("after the epoch", a["p"], a["z_end"])):
        fresh = native.Handle(c["dims"], "fp16x3")
        fresh.load_params(params)
        assert same_bits(fresh.encode(x[:n]), got), tag
        check_rule(f"encode {tag} n={n}", host(got), host(b["z_step"] if tag == "after train_step" else b["z_end"]),
                   orc.encode(c["dims"], host(params)[:-1], host(x[:n])))
    # load_params reaches the fragments too
    h = a["h"]
    h.load_params(dev(np.concatenate([c["flat"], [0.0]]), torch.float32))
    assert same_bits(h.encode(x[:n]), a["z_before"])


def test_activation_means_are_the_fp32_handles():
    c = case(15)
    x = dev(c["x"][:700], torch.float32)
    a = make_handle(c["dims"], c["flat"], "fp16x3")[0].activation_means(x)
    b = make_handle(c["dims"], c["flat"], "fp32")[0].activation_means(x)
    assert same_bits(a, b)


NOTICE = "BAMD_MODE_F16X3 has kernels for the 24-column AE"


@pytest.mark.parametrize("shape", ["ae-30-8", "ae-2500-25", "relu", "pjconv"])
def test_fallback_shapes_are_float32_handles_with_a_notice(shape, capfd, monkeypatch):
    monkeypatch.delenv("BALER_AMD_QUIET", raising=False)
    rng = np.random.default_rng(3)
    if shape == "pjconv":
        z = 10
        flat = models.pj_conv_init(z).numpy().astype(np.float64)
        h = native.Handle.pj_conv(z, "fp16x3")
        h.load_params(dev(np.concatenate([flat, [0.0]]), torch.float32))
        x = rng.random((5, 784))
        want = pjconv_ref.encode(z, flat, x)
    elif shape == "relu":
        dims = fpga_ref.dims(16, 4)
        flat = orc.formula_params(dims, 5)
        h, _ = make_handle(dims, flat, "fp16x3", act="relu")
        x = rng.random((300, 16))
        want = fpga_ref.encode(dims, flat, x)
    else:
        F, Z = (30, 8) if shape == "ae-30-8" else (2500, 25)
        dims = orc.ae_dims(F, Z)
        flat = orc.formula_params(dims, 5)
        h, _ = make_handle(dims, flat, "fp16x3")
        x = rng.random((300 if F == 30 else 40, F))
        want = orc.encode(dims, flat, x)
    err = capfd.readouterr().err
    assert NOTICE in err and "computes in float32" in err and err.count(NOTICE) == 1, err
    assert h.mode == native.MODE_F16X3 and h.compute_mode == native.MODE_F32 and h.path != "f16x3"
    assert int(native.lib().bamd_mode_of(h._h)) == native.MODE_F32
    e = ref.rel(host(h.encode(dev(x, torch.float32))), want)
    print(f"{shape}: encode error {e:.3e}")
    assert e < TOL32
    # silent under BALER_AMD_QUIET=1
    monkeypatch.setenv("BALER_AMD_QUIET", "1")
    if shape == "pjconv":
        native.Handle.pj_conv(10, "fp16x3")
    else:
        native.Handle(h.dims, "fp16x3", act=h.act)
    assert NOTICE not in capfd.readouterr().err


def test_create_through_the_c_abi():
    L = native.lib()
    h = ctypes.c_void_p()
    dims = (ctypes.c_int * 9)(*orc.ae_dims(24, 15))
    assert L.bamd_create(dims, 8, 5, 0, ctypes.byref(h)) == 0
    assert L.bamd_mode_of(h) == 5 and L.bamd_path_of(h) == 5
    L.bamd_destroy(h)
    assert L.bamd_create(dims, 8, 4, 0, ctypes.byref(h)) == -1 and b"unknown mode" in L.bamd_last_error()      # 4 is no mode
    assert L.bamd_create(dims, 8, 6, 0, ctypes.byref(h)) == -1 and b"unknown mode" in L.bamd_last_error()
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


def test_faster_than_the_fp32_handle():
    """The mode exists to beat the fp32 kernels at their accuracy: 1M float64 rows, encode and decode, the two handles timed
    alternately in one process; the ratio is printed."""
    c = case(15)
    h, h32 = handles(c)
    n = 1_000_000
    x = torch.rand((n, 24), dtype=torch.float64, device="cuda")
    z = h32.encode(x)
    zout, dout = torch.empty_like(z), torch.empty_like(x)
    t = {"fp16x3": [[], []], "fp32": [[], []]}
    for _ in range(3):
        for name, hh in (("fp32", h32), ("fp16x3", h)):
            t[name][0].append(_ms(lambda: hh.encode(x, out=zout), 5))
            t[name][1].append(_ms(lambda: hh.decode(z, out=dout), 5))
    med = {k: [sorted(s)[1] for s in v] for k, v in t.items()}
    print(f"1M float64 rows: encode fp16x3 {med['fp16x3'][0]:.4f} ms  fp32 {med['fp32'][0]:.4f} ms (x{med['fp32'][0] / med['fp16x3'][0]:.2f});  "
          f"decode fp16x3 {med['fp16x3'][1]:.4f} ms  fp32 {med['fp32'][1]:.4f} ms (x{med['fp32'][1] / med['fp16x3'][1]:.2f})")
    assert med["fp16x3"][0] < med["fp32"][0], "encode"
    assert med["fp16x3"][1] < med["fp32"][1], "decode"
