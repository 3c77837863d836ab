"""bamd_frame_stats and bamd_pixel_moments (native.frame_stats / native.pixel_moments_raw) against numpy restatements written here:
d = before - after in the table's dtype, extrema with np.nanmin / np.nanmax, sums with np.sum of float64.  Extrema, NaN counts and the
difference image bit for bit; sums within 1e-11 * sum |term| (the bar DESIGN section 11 sets for the report's statistics: the
restatement's pairwise float64 sum and the kernels' fixed-order float64 sums both err by far less).  The frame-independence rule bit
for bit, the fixture recorded from the reference's plot_2D, special values, the refusals of the ABI, guard bands and a gated side stream.

Shapes: the frame lengths at which bamd_frame_stats changes path (a wave takes a segment of 4096 elements, a lane keeps two 16-byte
vector pairs in flight: 128 float64 / 256 float32 elements per wave and round; frames above a segment are split and finished by a
second launch, above 64 segments a lane of that launch folds several), one below, at and above each, odd lengths (float32 frames at
odd offsets: the scalar-load route); bamd_pixel_moments: frames narrower than, equal to and wider than a workgroup's 256 pixels, one and many ranges."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import guard_bands as gb
import stream_gate as sg
from baler_amd import native

pytestmark = pytest.mark.gpu

TOL = 1e-11
SEG = 4096
FRAME_ELEMS = [1, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2500, 4095, 4096, 4097, 2 * 4096 + 5, 65535, 65536, 65537,
               2 * 65536 + 5, 64 * 4096 + 1]
N_FRAMES = [1, 2, 7, 300]
MAX_ELEMS = 2_100_000


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def tables(n, f, dtype, seed, specials=True):
    """Both signs, another scale in every frame; where the frame is long enough a NaN in `before` only, one in `after` only, +-inf and
    -0 / +0 are put in (never a frame without a finite value)."""
    rng = np.random.default_rng(seed)
    before = rng.normal(0.0, 1.0, (n, f)) * (1.0 + np.arange(n))[:, None]
    after = before + rng.normal(0.0, 0.05, (n, f))
    before, after = before.astype(dtype), after.astype(dtype)
    if specials and f >= 63:
        for k in range(n):
            if k % 3 == 1:
                before[k, (7 * k) % f] = np.nan
            if k % 4 == 2:
                after[k, (11 * k + 5) % f] = np.nan
            if k % 5 == 3:
                before[k, (13 * k + 1) % f] = np.inf
                after[k, (17 * k + 2) % f] = -np.inf
            before[k, f - 1], after[k, f - 1] = -0.0, 0.0
    return before, after


def np_frame_stats(before, after):
    """-> ((10, n) float64 restatement, (10, n) bars for the sums (rows 6..8), d)."""
    with np.errstate(all="ignore"):
        d = np.subtract(before, after)
        b64, a64, d64 = before.astype(np.float64), after.astype(np.float64), d.astype(np.float64)
        rows = [np.nanmin(b64, axis=1), np.nanmax(b64, axis=1), np.nanmin(a64, axis=1), np.nanmax(a64, axis=1),
                np.nanmin(d64, axis=1), np.nanmax(d64, axis=1),
                np.sum(d64, axis=1), np.sum(d64 * d64, axis=1), np.sum(b64 * b64, axis=1),
                np.sum(np.isnan(before) | np.isnan(after), axis=1).astype(np.float64)]
        bars = [np.sum(np.abs(d64), axis=1), np.sum(d64 * d64, axis=1), np.sum(b64 * b64, axis=1)]
    return np.stack(rows), np.stack(bars), d


def assert_bits(got, want, what):
    """The same bits, -0 against +0 included; a NaN stands where a NaN stands (IEEE 754 leaves the sign and payload of a NaN result
    open: x - NaN keeps the operand's sign on the host and may carry the negated one on the device)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    nan = np.isnan(want)
    bad = (np.isnan(got) != nan) | (~nan & (got.view(u) != want.view(u)))
    assert not bad.any(), f"{what}: {int(bad.sum())} element(s) differ, first at {tuple(int(i) for i in np.argwhere(bad)[0])}: " \
                          f"{got[bad][0]!r} ({got.view(u)[bad][0]:#x}) against {want[bad][0]!r} ({want.view(u)[bad][0]:#x})"


def assert_values(got, want, what):
    """Equal values, NaN in the same places; -0 and +0 compare equal (an extremum over both zeros is either, in numpy too)."""
    np.testing.assert_array_equal(got, want, err_msg=what)


def assert_sums(got, want, bar, what):
    fin = np.isfinite(want) & np.isfinite(bar)
    np.testing.assert_array_equal(got[~fin], want[~fin], err_msg=what)
    err = np.abs(got[fin] - want[fin])
    worst = float((err / np.maximum(bar[fin], 1e-300)).max()) if err.size else 0.0
    print(f"{what}: worst error {worst:.3e} of sum |term|")
    assert (err <= TOL * bar[fin]).all(), what


def check_frames(before, after, what):
    n, f = before.shape
    bd, ad = dev(before), dev(after)
    diff = torch.full_like(bd, 7.0)
    raw = native.frame_stats(bd, ad, diff)
    assert tuple(raw.shape) == (10, n) and raw.dtype == torch.float64
    got = raw.cpu().numpy()
    want, bars, d = np_frame_stats(before, after)
    assert_bits(diff.cpu().numpy(), d, what + " diff")
    assert_values(got[:6], want[:6], what + " extrema")
    np.testing.assert_array_equal(got[9], want[9], err_msg=what + " NaN count")
    for k in range(3):
        assert_sums(got[6 + k], want[6 + k], bars[k], f"{what} row {6 + k}")
    again = native.frame_stats(bd, ad)                                # without diff, and a second call: the same bits
    assert torch.equal(raw.view(torch.int64), again.view(torch.int64)), what + " repeat"
    return raw


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("f", FRAME_ELEMS)
def test_frame_stats_against_numpy(f, dtype):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        ran = 0
        for n in N_FRAMES:
            if n * f > MAX_ELEMS:
                continue
            before, after = tables(n, f, dtype, 1000 * n + f)
            check_frames(before, after, f"n={n} F={f}")
            ran += 1
        assert ran >= 1


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("f", [3, 63, 257, 1025, 2500, SEG + 1, 2 * SEG + 5, 65537, 2 * 65536 + 5])
def test_a_frame_is_a_function_of_its_values_alone(f, dtype):
    """The same frame alone, at index 5 of 9, in a table whose base is one element off (a slice of a larger tensor: no base is
    16-byte aligned, the scalar-load route) and in chunks: the same ten values bit for bit, and the same difference image."""
    before, after = tables(9, f, dtype, 77 + f)
    bd, ad = dev(before), dev(after)
    bits = lambda t: t.contiguous().view(torch.int64)                  # noqa: E731
    whole = native.frame_stats(bd, ad)
    alone = native.frame_stats(bd[5:6].clone(), ad[5:6].clone())
    assert torch.equal(bits(alone[:, 0]), bits(whole[:, 5])), "index"
    # one element off: both tables and the difference image
    big_b, big_a = torch.zeros(9 * f + 1, dtype=bd.dtype, device="cuda"), torch.zeros(9 * f + 1, dtype=bd.dtype, device="cuda")
    big_d = torch.zeros(9 * f + 1, dtype=bd.dtype, device="cuda")
    ob, oa, od = big_b[1:].view(9, f), big_a[1:].view(9, f), big_d[1:].view(9, f)
    ob.copy_(bd)
    oa.copy_(ad)
    assert ob.data_ptr() % 16 and oa.data_ptr() % 16 and ob.is_contiguous()
    aligned_d = torch.empty_like(bd)
    native.frame_stats(bd, ad, aligned_d)
    off = native.frame_stats(ob, oa, od)
    assert torch.equal(bits(off), bits(whole)), "offset base"
    assert_bits(od.cpu().numpy(), aligned_d.cpu().numpy(), "offset diff")
    assert float(big_d[0]) == 0.0
    # only one of the two tables off: still the same bits
    assert torch.equal(bits(native.frame_stats(ob, ad)), bits(whole)), "one table off"
    # chunked against whole: uneven chunks (odd frame counts put odd-length float32 frames at odd offsets)
    parts = [native.frame_stats(bd[a:e], ad[a:e]) for a, e in ((0, 1), (1, 4), (4, 9))]
    assert torch.equal(bits(torch.cat(parts, dim=1)), bits(whole)), "chunks"


@pytest.mark.parametrize("run", ["f64", "f32", "blocks"])
def test_fixture_of_the_reference_is_reproduced(golden, run):
    """tests/golden/g23_plot2d.npz: what the reference's plot_2D handed to imshow -- vmin, vmax and the difference image of every frame."""
    g = golden("g23_plot2d.npz")
    before, after = g[f"{run}_before"], g[f"{run}_after"]
    bd = dev(before)
    ad = dev(after).reshape(bd.shape)                                  # the flat decompressed array of the block run, viewed as frames
    diff = torch.empty_like(bd)
    raw = native.frame_stats(bd, ad, diff)
    s = native.frame_summary(raw, 12 * 9, before.dtype)
    assert s["vmin"].dtype == before.dtype
    assert_bits(s["vmin"], g[f"{run}_vmin"], "vmin")
    assert_bits(s["vmax"], g[f"{run}_vmax"], "vmax")
    assert_bits(diff.cpu().numpy(), g[f"{run}_diff"], "difference image")
    assert (s["nan_count"] == 0).all() and np.isfinite(s["psnr"]).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("f", [5, 300, 2500])
def test_special_values(f, dtype):
    before = np.full((8, f), 1.5, dtype)
    after = np.full((8, f), 0.25, dtype)
    before[0, 1] = np.nan                                              # a NaN in before only
    after[1, f - 2] = np.nan                                           # in after only
    before[2, 0], after[2, 2] = np.inf, np.inf                         # +inf - x, x - inf
    before[3, 3], after[3, 3] = -np.inf, -np.inf                       # -inf - -inf = NaN in d alone: not counted
    before[4], after[4] = -0.0, 0.0                                    # d = -0 - 0 = -0 everywhere
    before[5, ::2] = -0.0
    before[5, 1::2] = 0.0                                              # both zeros in one frame
    after[5] = 0.0
    before[6], after[6] = np.nan, np.nan                               # nothing but NaN
    # frame 7: one repeated value
    raw = native.frame_stats(dev(before), dev(after)).cpu().numpy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        want, bars, d = np_frame_stats(before, after)
    np.testing.assert_array_equal(raw[9], [1, 1, 0, 0, 0, 0, f, 0])
    keep = [0, 1, 2, 3, 4, 5, 7]
    assert_values(raw[:6, keep], want[:6, keep], "extrema")
    assert raw[0, 6] == np.inf and raw[1, 6] == -np.inf and raw[4, 6] == np.inf and raw[5, 6] == -np.inf      # no value: the neutral elements
    assert np.isnan(raw[6:9, 6]).all() and np.isnan(raw[6, 0]) and np.isnan(raw[6, 1]) and np.isnan(raw[8, 0]) and not np.isnan(raw[8, 1])
    assert raw[1, 2] == np.inf and raw[5, 2] == np.inf and raw[4, 2] == -np.inf and raw[0, 3] == -np.inf and np.isnan(raw[6, 3])
    # a frame of -0 alone keeps the sign in every extremum (a sum over ranks would lose it); d = -0 - (+0) = -0
    assert_bits(raw[0:2, 4], np.array([-0.0, -0.0]), "min / max of -0")
    assert_bits(raw[4:6, 4], np.array([-0.0, -0.0]), "min / max of d = -0")
    assert_bits(raw[2:4, 4], np.array([0.0, 0.0]), "min / max of +0")
    assert (raw[0:6, 5] == 0.0).all()                                  # both zeros: a zero
    assert_bits(raw[0:6, 7], np.array([1.5, 1.5, 0.25, 0.25, 1.25, 1.25]), "a repeated value")
    for k in range(3):
        assert_sums(raw[6 + k, [4, 5, 7]], want[6 + k, [4, 5, 7]], bars[k][[4, 5, 7]], f"row {6 + k}")


# ---- bamd_pixel_moments ---------------------------------------------------------------------------------------------------------
def np_pixel_moments(before, after):
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        d64 = np.subtract(before, after).astype(np.float64)
        rows = [np.sum(d64, axis=0), np.sum(d64 * d64, axis=0), np.nanmin(d64, axis=0), np.nanmax(d64, axis=0),
                np.sum(np.isnan(before) | np.isnan(after), axis=0).astype(np.float64)]
        bars = [np.sum(np.abs(d64), axis=0), np.sum(d64 * d64, axis=0)]
    return np.stack(rows), np.stack(bars)


def check_pixels(got, before, after, what):
    want, bars = np_pixel_moments(before, after)
    got = got.cpu().numpy()
    assert got.shape == want.shape, what
    assert_values(got[2:4], want[2:4], what + " extrema")
    np.testing.assert_array_equal(got[4], want[4], err_msg=what + " NaN count")
    assert_sums(got[0], want[0], bars[0], what + " sum")
    assert_sums(got[1], want[1], bars[1], what + " sum of squares")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n, f", [(1, 1), (5000, 1), (5000, 3), (1, 2500), (7, 63), (300, 100), (300, 255), (300, 256), (300, 257),
                                  (300, 2500), (1, 2 * 65536 + 5), (40, 4097)])
def test_pixel_moments_against_numpy(n, f, dtype):
    before, after = tables(n, f, dtype, 31 * n + f, specials=f >= 63 and n >= 7)
    if n >= 7 and f >= 63:
        before[:, 2] = np.nan                                          # a pixel that is NaN in every frame: no extremum
    bd, ad = dev(before), dev(after)
    raw = native.pixel_moments_raw(bd, ad)
    assert tuple(raw.shape) == (5, f)
    if n >= 7 and f >= 63:
        g = raw.cpu().numpy()
        assert g[2, 2] == np.inf and g[3, 2] == -np.inf and g[4, 2] == n
        keep = np.arange(f) != 2
        check_pixels(raw[:, torch.as_tensor(keep).cuda()], before[:, keep], after[:, keep], f"n={n} F={f}")
    else:
        check_pixels(raw, before, after, f"n={n} F={f}")
    again = native.pixel_moments_raw(bd, ad)
    assert torch.equal(raw.view(torch.int64), again.view(torch.int64)), "repeat"
    s = native.pixel_summary(raw, n)
    assert s["pixel_diff_rms"].shape == (f,)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("f", [3, 100, 2500])
def test_pixel_accumulate_over_uneven_chunks(f, dtype):
    n = 301
    before, after = tables(n, f, dtype, 5 + f, specials=f >= 63)
    bd, ad = dev(before), dev(after)
    whole = native.pixel_moments_raw(bd, ad)
    check_pixels(whole, before, after, f"whole F={f}")
    acc = None
    for a, e in ((0, 1), (1, 98), (98, 301)):                          # the float32 chunks of odd frames begin off a 16-byte boundary
        acc = native.pixel_moments_raw(bd[a:e], ad[a:e], out=acc)
    assert torch.equal(acc[2:].view(torch.int64), whole[2:].view(torch.int64)), "extrema and counts"
    check_pixels(acc, before, after, f"three chunks F={f}")
    # an empty chunk adds nothing, and alone gives the neutral elements
    same = native.pixel_moments_raw(bd[:0], ad[:0], out=acc.clone())
    assert torch.equal(same.view(torch.int64), acc.view(torch.int64))
    neutral = native.pixel_moments_raw(bd[:0], ad[:0]).cpu().numpy()
    np.testing.assert_array_equal(neutral, np.array([[0.0], [0.0], [np.inf], [-np.inf], [0.0]]) * np.ones((1, f)))


def test_binding_refusals():
    x = torch.ones((4, 3, 5), dtype=torch.float32, device="cuda")
    assert tuple(native.frame_stats(x, x).shape) == (10, 4) and tuple(native.pixel_moments_raw(x, x).shape) == (5, 15)     # N-D frames
    assert tuple(native.frame_stats(x[:0], x[:0]).shape) == (10, 0)
    for fn in (native.frame_stats, native.pixel_moments_raw):
        with pytest.raises(native.NativeError):
            fn(x, x.double())
        with pytest.raises(native.NativeError):
            fn(x, x[:3])
        with pytest.raises(native.NativeError):
            fn(x[:, 0, 0], x[:, 0, 0])                                 # 1-D: no frames
        with pytest.raises(native.NativeError):
            fn(x.cpu(), x.cpu())
    with pytest.raises(native.NativeError):
        native.frame_stats(x, x, diff=torch.empty((4, 3, 4), dtype=torch.float32, device="cuda"))
    with pytest.raises(native.NativeError):
        native.pixel_moments_raw(x, x, out=torch.empty((5, 14), dtype=torch.float64, device="cuda"))


def test_abi_refusals_and_no_frames():
    L = native.lib()
    INVALID = -1
    x = torch.ones((8, 6), dtype=torch.float64, device="cuda")
    y = torch.zeros((8, 6), dtype=torch.float64, device="cuda")
    fo = torch.full((10, 8), 5.0, dtype=torch.float64, device="cuda")
    po = torch.full((5, 6), 5.0, dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    null = ctypes.c_void_p(0)

    def frames(b=x, a=y, dtype=1, n=8, f=6, out=fo):
        return L.bamd_frame_stats(p(b) if b is not None else null, p(a) if a is not None else null, dtype, n, f,
                                  p(out) if out is not None else null, null, null)

    def pixels(b=x, a=y, dtype=1, n=8, f=6, out=po, acc=0):
        return L.bamd_pixel_moments(p(b) if b is not None else null, p(a) if a is not None else null, dtype, n, f,
                                    p(out) if out is not None else null, acc, null)

    for call, name in ((frames, b"bamd_frame_stats"), (pixels, b"bamd_pixel_moments")):
        for kw, word in (({"dtype": 2}, b"dtype must be BAMD_F32 or BAMD_F64"), ({"dtype": 3}, b"dtype"), ({"dtype": 8}, b"dtype"),
                         ({"dtype": -1}, b"dtype"), ({"f": 0}, b"frame_elems"), ({"f": -3}, b"frame_elems"), ({"n": -1}, b"n_frames"),
                         ({"out": None}, b"null output"), ({"out": None, "n": 0}, b"null output"), ({"b": None}, b"null table"),
                         ({"a": None}, b"null table")):
            assert call(**kw) == INVALID, kw
            assert name in L.bamd_last_error() and word in L.bamd_last_error(), (kw, L.bamd_last_error())
    torch.cuda.synchronize()
    assert (fo == 5).all() and (po == 5).all()                         # a refusal writes nothing
    assert frames(n=0) == 0 and frames(b=None, a=None, n=0) == 0 and pixels(n=0, acc=1) == 0
    torch.cuda.synchronize()
    assert (fo == 5).all() and (po == 5).all()
    assert pixels(b=None, a=None, n=0) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(po.cpu().numpy(), np.array([[0.0], [0.0], [np.inf], [-np.inf], [0.0]]) * np.ones((1, 6)))
    assert frames() == 0 and pixels() == 0 and pixels(acc=1) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(fo.cpu().numpy(), np.array([1, 1, 0, 0, 1, 1, 6, 6, 6, 0.0])[:, None] * np.ones((1, 8)))
    np.testing.assert_array_equal(po.cpu().numpy(), np.array([16, 16, 1, 1, 0.0])[:, None] * np.ones((1, 6)))


# ---- guard bands and streams ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n, f", [(5, 257), (3, 2 * SEG + 3)], ids=["one-segment", "segments"])
def test_frame_stats_inside_guard_bands(n, f, dtype):
    before, after = tables(n, f, dtype, 3, specials=False)
    bd, ad = dev(before), dev(after)
    plain_d = torch.empty_like(bd)
    plain = native.frame_stats(bd, ad, plain_d)
    for lead in (0, 1, 3):
        (bv, ba), (av, aa) = gb.framed(bd, lead, fill=gb.NAN), gb.framed(ad, lead, fill=gb.NAN)
        snaps = [t.clone() for t in (ba, aa)]
        dv, da = gb.framed(torch.zeros_like(bd), lead)
        got = native.frame_stats(bv, av, dv)
        torch.cuda.synchronize()
        gb.assert_guards_intact(da, lead, n, f"diff lead={lead}")
        for arena, snap, what in zip((ba, aa), snaps, ("before", "after")):
            gb.assert_inputs_untouched(arena, snap, what)
        assert torch.equal(got.view(torch.int64), plain.view(torch.int64)) and torch.equal(dv, plain_d)
    # the (10, n) output inside a poisoned arena, through the C ABI
    ov, oa = gb.framed(torch.zeros_like(plain), 2)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    rc = native.lib().bamd_frame_stats(P(bd), P(ad), 1 if dtype == np.float64 else 0, n, f, P(ov), None,
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, native.lib().bamd_last_error()
    torch.cuda.synchronize()
    gb.assert_guards_intact(oa, 2, 10, "out")
    assert torch.equal(ov.view(torch.int64), plain.view(torch.int64))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n, f", [(300, 100), (300, 257), (3, 2500)], ids=["narrow", "ranges", "one-range"])
def test_pixel_moments_inside_guard_bands(n, f, dtype):
    before, after = tables(n, f, dtype, 4, specials=False)
    bd, ad = dev(before), dev(after)
    plain = native.pixel_moments_raw(bd, ad)
    for lead in (0, 1, 3):
        (bv, ba), (av, aa) = gb.framed(bd, lead, fill=gb.NAN), gb.framed(ad, lead, fill=gb.NAN)
        snaps = [t.clone() for t in (ba, aa)]
        ov, oa = gb.framed(torch.zeros_like(plain), lead)
        P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
        for acc in (0, 1):
            rc = native.lib().bamd_pixel_moments(P(bv), P(av), 1 if dtype == np.float64 else 0, n, f, P(ov), acc,
                                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, native.lib().bamd_last_error()
        torch.cuda.synchronize()
        gb.assert_guards_intact(oa, lead, 5, f"out lead={lead}")
        for arena, snap, what in zip((ba, aa), snaps, ("before", "after")):
            gb.assert_inputs_untouched(arena, snap, what)
        twice = native.pixel_moments_raw(bd, ad, out=plain.clone())
        assert torch.equal(ov.view(torch.int64), twice.view(torch.int64))


def _same_bits(got, want, what):
    assert sg.same_bits(got, want), what


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_frame_stats_on_a_gated_side_stream(dtype):
    n, f = 3, SEG + 1                                                  # two segments: the scratch partials and the finishing launch too
    before, after = tables(n, f, dtype, 6, specials=False)
    plain_d = torch.empty((n, f), dtype=dev(before).dtype, device="cuda")
    plain = native.frame_stats(dev(before), dev(after), plain_d)
    code = 1 if dtype == np.float64 else 0

    def seq(t):
        o = {"stats": sg.out((10, n), torch.float64), "diff": sg.out((n, f), t["x"].dtype), "short": sg.out((10, n), torch.float64)}
        L = native.lib()
        P = lambda x: ctypes.c_void_p(x.data_ptr())      # noqa: E731
        S = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.bamd_frame_stats(P(t["x"]), P(t["r"]), code, n, f, P(o["stats"]), P(o["diff"]), S) == 0, L.bamd_last_error()
        assert L.bamd_frame_stats(P(t["x"]), P(t["r"]), code, n, 300, P(o["short"]), None, S) == 0, L.bamd_last_error()
        return o

    res = sg.run_gated(seq, {"x": dev(before), "r": dev(after)}, same={None: _same_bits}, what="frame stats")
    assert sg.same_bits(res["outs"]["stats"], plain) and sg.same_bits(res["outs"]["diff"], plain_d)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_pixel_moments_on_a_gated_side_stream(dtype):
    n, f = 300, 2500                                                   # many ranges: the scratch partials and the finishing launch
    before, after = tables(n, f, dtype, 8, specials=False)
    plain = native.pixel_moments_raw(dev(before), dev(after))
    code = 1 if dtype == np.float64 else 0

    def seq(t):
        o = {"once": sg.out((5, f), torch.float64), "twice": sg.out((5, f), torch.float64)}
        L = native.lib()
        P = lambda x: ctypes.c_void_p(x.data_ptr())      # noqa: E731
        S = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for name, acc in (("once", 0), ("twice", 0), ("twice", 1)):
            assert L.bamd_pixel_moments(P(t["x"]), P(t["r"]), code, n, f, P(o[name]), acc, S) == 0, L.bamd_last_error()
        return o

    res = sg.run_gated(seq, {"x": dev(before), "r": dev(after)}, same={None: _same_bits}, what="pixel moments")
    assert sg.same_bits(res["outs"]["once"], plain)
    assert sg.same_bits(res["outs"]["twice"], native.pixel_moments_raw(dev(before), dev(after), out=plain.clone()))
