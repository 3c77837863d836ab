"""The report mode for 2-D data without a GPU: the frame-statistics header and symbols, the host summaries on hand-made raw arrays, the
opt-in dispatch of the CLI mode and its refusals, and the fixture recorded from the reference's plot_2D."""
import os
import re
import types

import numpy as np
import pytest

from baler_amd import native
from baler_amd.modules import helper

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_frame_statistics():
    with open(os.path.join(REPO, "include", "baler_amd_frames.h")) as f:
        src = f.read()
    declared = re.findall(r"^int (bamd_[a-z_0-9]+)\(", src, flags=re.M)
    assert declared == ["bamd_frame_stats", "bamd_pixel_moments"] == list(native.FRAME_SYMBOLS)
    decl = " ".join(src[src.index("int bamd_frame_stats("):].split(";")[0].split())
    assert decl == ("int bamd_frame_stats(const void *before, const void *after, int dtype, int64_t n_frames, int64_t frame_elems, "
                    "double *out, void *diff, void *stream)")
    decl = " ".join(src[src.index("int bamd_pixel_moments("):].split(";")[0].split())
    assert decl == ("int bamd_pixel_moments(const void *before, const void *after, int dtype, int64_t n_frames, int64_t frame_elems, "
                    "double *out, int accumulate, void *stream)")
    with open(os.path.join(REPO, "include", "baler_amd.h")) as f:
        assert '#include "baler_amd_frames.h"' in f.read()
    assert not set(native.FRAME_SYMBOLS) & set(native.SYMBOLS)
    lib = native.lib()
    for name in native.FRAME_SYMBOLS:
        assert hasattr(lib, name), name
    with open(os.path.join(REPO, "baler_amd", "csrc", "framestats.hip")) as f:
        hip = f.read()
    assert re.findall(r"^int (bamd_\w+)\(", hip[hip.index('extern "C"'):], flags=re.M) == list(native.FRAME_SYMBOLS)
    assert "atomic" not in hip.replace("no float atomics", "")          # fixed-order sums only
    assert len(native.FRAME_ROWS) == 10 and len(native.PIXEL_ROWS) == 5
    assert sorted(native.PIXEL_SUM_ROWS + native.PIXEL_MIN_ROWS + native.PIXEL_MAX_ROWS) == list(range(5))
    with open(os.path.join(REPO, "README.md")) as f:
        readme = f.read()
    assert "40 in all" in readme and "framestats.hip" in readme and "report_frames" in readme


def _raw(n):
    r = np.zeros((10, n))
    r[0], r[1], r[2], r[3] = -1.0, 3.0, -2.0, 2.5
    r[4], r[5] = -0.5, 0.25
    return r


def test_frame_summary():
    F = 4
    r = _raw(4)
    r[6], r[7], r[8] = 2.0, 16.0, 64.0
    r[9, 1] = 2                                                      # frame 1 holds NaNs: the reference's amin / amax give NaN
    r[7, 2] = 0.0                                                    # frame 2: a perfect reconstruction
    r[6, 2] = 0.0
    r[8, 3], r[0, 3], r[1, 3] = 0.0, 0.0, 0.0                        # frame 3: before is all zero
    s = native.frame_summary(r, F, np.float32)
    assert set(s) == {"vmin", "vmax", "diff_min", "diff_max", "diff_mean", "diff_rms", "rel_l2", "psnr", "nan_count"}
    assert s["vmin"].dtype == np.float32 and s["vmax"].dtype == np.float32 and s["nan_count"].dtype == np.int64
    np.testing.assert_array_equal(s["vmin"], np.array([-2.0, np.nan, -2.0, -2.0], np.float32))
    np.testing.assert_array_equal(s["vmax"], np.array([3.0, np.nan, 3.0, 2.5], np.float32))
    np.testing.assert_array_equal(s["nan_count"], [0, 2, 0, 0])
    np.testing.assert_array_equal(s["diff_min"], [-0.5] * 4)
    np.testing.assert_array_equal(s["diff_max"], [0.25] * 4)
    np.testing.assert_array_equal(s["diff_mean"], [0.5, 0.5, 0.0, 0.5])
    np.testing.assert_array_equal(s["diff_rms"], [2.0, 2.0, 0.0, 2.0])
    np.testing.assert_array_equal(s["rel_l2"], [0.5, 0.5, 0.0, np.inf])              # sqrt(16 / 64); 16 / 0
    np.testing.assert_array_equal(s["psnr"], [20 * np.log10(4.0 / 2.0), 20 * np.log10(4.0 / 2.0), np.inf, -np.inf])
    assert native.frame_summary(r, F)["vmin"].dtype == np.float64
    z = np.zeros((10, 1))                                                            # 0 / 0: NaN, no warning raised
    with np.errstate(all="raise"):
        s = native.frame_summary(z, F)
    assert np.isnan(s["rel_l2"][0]) and np.isnan(s["psnr"][0])
    assert native.frame_summary(np.zeros((10, 0)), F)["diff_rms"].shape == (0,)


def test_pixel_summary():
    r = np.zeros((5, 3))
    r[0], r[1] = (6.0, -3.0, np.nan), (36.0, 27.0, np.nan)
    r[2], r[3] = (-1.0, -2.0, np.inf), (4.0, 0.0, -np.inf)
    r[4] = (0, 1, 4)                                                 # pixel 2 is NaN in all four frames
    with np.errstate(all="raise"):
        s = native.pixel_summary(r, 4)
    assert set(s) == {"pixel_diff_mean", "pixel_diff_rms", "pixel_diff_min", "pixel_diff_max", "pixel_nan_count"}
    np.testing.assert_array_equal(s["pixel_diff_mean"], [1.5, -1.0, np.nan])
    np.testing.assert_array_equal(s["pixel_diff_rms"], [3.0, 3.0, np.nan])
    np.testing.assert_array_equal(s["pixel_diff_min"], [-1.0, -2.0, np.inf])
    np.testing.assert_array_equal(s["pixel_nan_count"], [0, 1, 4])
    assert s["pixel_nan_count"].dtype == np.int64


def _project(tmp_path, data_dimension, before_shape=(6, 4, 5), after_shape=None, **keys):
    rng = np.random.default_rng(3)
    before = rng.normal(size=before_shape)
    after = before.reshape(after_shape or before_shape) if after_shape is None or np.prod(after_shape) == before.size \
        else rng.normal(size=after_shape)
    np.savez(str(tmp_path / "d.npz"), data=before, names=np.array(["a"]))
    os.makedirs(tmp_path / "decompressed_output", exist_ok=True)
    np.savez(str(tmp_path / "decompressed_output" / "decompressed.npz"), data=after, names=np.array(["a"]))
    return types.SimpleNamespace(input_path=str(tmp_path / "d.npz"), data_dimension=data_dimension, **keys)


def _no_gpu():
    raise native.NativeError("no MI355X (gfx950) device visible: the baler_amd hot path has no CPU fallback")


def test_report_of_frames_without_gpu_fails_loudly(tmp_path, monkeypatch):
    """The opt-in reaches the GPU path: NativeError, not the NotImplementedError of a 2-D config without the key."""
    monkeypatch.setattr(native, "require_gpu", _no_gpu)
    from baler_amd import baler
    with pytest.raises(native.NativeError):
        baler.perform_report(str(tmp_path), _project(tmp_path, 2, report_frames=True), False)
    assert not os.path.exists(tmp_path / "plotting")


def test_without_the_key_the_refusal_stands(tmp_path, monkeypatch):
    monkeypatch.setattr(native, "require_gpu", lambda: pytest.fail("GPU touched before the refusal"))
    from baler_amd import baler
    for keys in ({}, {"report_frames": False}):
        c = _project(tmp_path, 2, **keys)
        with pytest.raises(NotImplementedError, match="plot_2D") as e:
            baler.perform_report(str(tmp_path), c, False)
        assert "report_frames" in str(e.value)
        with pytest.raises(NotImplementedError, match="plot_2D"):
            helper.check_report(c)
    assert not helper.report_frames_on(types.SimpleNamespace(data_dimension=1, report_frames=True))


@pytest.mark.parametrize("after_shape", [(6, 20), (6, 1, 4, 5), (6, 2, 10)], ids=["flat", "4d", "blocks"])
def test_matching_after_shapes_are_accepted(tmp_path, monkeypatch, after_shape):
    """Accepted: the shape checks pass and the next thing the report does is ask for the GPU."""
    monkeypatch.setattr(native, "require_gpu", _no_gpu)
    c = _project(tmp_path, 2, after_shape=after_shape, report_frames=True)
    before, after = helper._frame_tables(c, str(tmp_path))
    assert before.shape == after.shape == (6, 4, 5)
    np.testing.assert_array_equal(before, after)
    with pytest.raises(native.NativeError):
        helper.frame_report(c, str(tmp_path))


@pytest.mark.parametrize("before_shape, after_shape", [((6, 4, 5), (5, 4, 5)), ((6, 4, 5), (6, 4, 4)), ((6, 4, 5), (120,)), ((6,), (6,)),
                                                       ((6, 4, 5), (3, 40))],
                         ids=["frames", "elems", "1d-after", "1d-before", "same-size-other-frames"])
def test_mismatched_shapes_are_refused_before_gpu_work(tmp_path, monkeypatch, before_shape, after_shape):
    monkeypatch.setattr(native, "require_gpu", lambda: pytest.fail("GPU touched before the refusal"))
    c = _project(tmp_path, 2, before_shape=before_shape, after_shape=after_shape, report_frames=True)
    with pytest.raises(ValueError) as e:
        helper.frame_report(c, str(tmp_path))
    assert str(before_shape) in str(e.value) and str(after_shape) in str(e.value)


def test_frame_report_refuses_1d(tmp_path, monkeypatch):
    monkeypatch.setattr(native, "require_gpu", lambda: pytest.fail("GPU touched before the refusal"))
    with pytest.raises(ValueError, match="data_dimension"):
        helper.frame_report(_project(tmp_path, 1, report_frames=True), str(tmp_path))


def test_default_config_names_the_key():
    text = helper.create_default_config("w", "p")
    assert "report_frames" in text and "report_diff" in text
    ns = {}
    exec(text, ns)                                                   # still a config module: the notes are comments
    c = types.SimpleNamespace()
    ns["set_config"](c)
    assert c.data_dimension == 1 and not hasattr(c, "report_frames")


def test_chunk_holds_at_least_one_frame():
    from baler_amd import hostio
    assert helper.report_chunk_rows(types.SimpleNamespace(), 2 * 2500 * 4) == hostio.CHUNK_BYTES // 20000
    assert helper.report_chunk_rows(types.SimpleNamespace(), 4 * hostio.CHUNK_BYTES) == 1
    assert helper.report_chunk_rows(types.SimpleNamespace(report_chunk_rows=5), 20000) == 5


def test_fixture_holds_what_the_reference_drew(golden):
    g = golden("g23_plot2d.npz")
    assert str(g["source"]) == "reference plot_2D, unmodified" and list(g["runs"]) == ["f64", "f32", "blocks"]
    for run, dt in (("f64", np.float64), ("f32", np.float32), ("blocks", np.float64)):
        before, after = g[f"{run}_before"], g[f"{run}_after"]
        assert before.shape == (7, 12, 9) and before.dtype == dt and after.dtype == dt
        assert after.shape == ((7, 108) if run == "blocks" else (7, 12, 9))
        assert (before < 0).any() and (before > 0).any() and np.isfinite(before).all() and np.isfinite(after).all()
        after = after.reshape(before.shape)
        assert g[f"{run}_diff"].dtype == dt and g[f"{run}_vmin"].dtype == dt
        np.testing.assert_array_equal(g[f"{run}_diff"], before - after)          # the sign: opposite to plot_1D's residual
        np.testing.assert_array_equal(g[f"{run}_vmin"], np.minimum(before.min(axis=(1, 2)), after.min(axis=(1, 2))))
        np.testing.assert_array_equal(g[f"{run}_vmax"], np.maximum(before.max(axis=(1, 2)), after.max(axis=(1, 2))))
