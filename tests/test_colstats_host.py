"""The report mode without a GPU: the C header and the symbol list, the host-built bin edges against the reference's expressions,
the row-cut selection, and the refusals of the CLI mode."""
import os
import types

import numpy as np
import pytest

from baler_amd import native
from baler_amd.modules import helper

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_column_statistics():
    with open(os.path.join(REPO, "include", "baler_amd.h")) as f:
        src = f.read()
    assert "int bamd_column_moments(const void *before, const void *after, int dtype, int64_t n_rows, int n_cols, int cut_col" in src
    assert "int bamd_column_hist(const void *before, const void *after, int dtype, int64_t n_rows, int n_cols, int cut_col" in src
    assert "#define BAMD_ABI_VERSION 1" in src
    assert "bamd_column_moments" in native.SYMBOLS and "bamd_column_hist" in native.SYMBOLS
    assert len(native.SYMBOLS) == 38 == len(set(native.SYMBOLS))
    assert len(native.MOMENT_ROWS) == 13
    assert sorted(native.MOMENT_SUM_ROWS + native.MOMENT_MIN_ROWS + native.MOMENT_MAX_ROWS) == list(range(13))


def test_readme_counts_the_exported_functions():
    with open(os.path.join(REPO, "README.md")) as f:
        assert "38 exported functions" in f.read()


def test_edges_equal_the_reference_expressions_bit_for_bit():
    # plotting.py:194, 217, 146-153
    np.testing.assert_array_equal(helper.report_response_edges(), np.arange(-20, 20, 0.1))
    np.testing.assert_array_equal(helper.report_residual_edges(), np.arange(-1, 1, 0.01))
    assert len(helper.report_response_edges()) == 400 and len(helper.report_residual_edges()) == 200
    rng = np.random.default_rng(5)
    for dt in (np.float64, np.float32):
        before = rng.normal(3.0, 10.0, 500).astype(dt)
        after = (before + rng.normal(0.0, 0.1, 500)).astype(dt)
        x_min, x_max = min(before + after), max(before + after)
        x_diff = abs(x_max - x_min)
        want = np.linspace(x_min - 0.1 * x_diff, x_max + 0.1 * x_diff, 200)
        got = helper.report_value_edges(dt((before + after).min()), dt((before + after).max()))
        assert got.dtype == want.dtype and len(got) == 200
        np.testing.assert_array_equal(got, want)


def test_cut_selection():
    cfg = types.SimpleNamespace()
    assert helper.REPORT_CUT == (3, 1e-6)
    for c in (1, 2, 3):
        assert helper.report_cut(cfg, c) is None          # the reference's column 3 does not exist
    assert helper.report_cut(cfg, 4) == (3, 1e-6) and helper.report_cut(cfg, 24) == (3, 1e-6)
    assert helper.report_cut(types.SimpleNamespace(report_cut=None), 24) is None
    assert helper.report_cut(types.SimpleNamespace(report_cut=(1, 0.5)), 3) == (1, 0.5)
    with pytest.raises(ValueError):
        helper.report_cut(types.SimpleNamespace(report_cut=(3, 0.5)), 3)


def test_chunk_rows_default_is_the_staging_size():
    from baler_amd import hostio
    assert helper.report_chunk_rows(types.SimpleNamespace(), 2 * 24 * 8) == hostio.CHUNK_BYTES // (2 * 24 * 8)
    assert helper.report_chunk_rows(types.SimpleNamespace(report_chunk_rows=1000), 384) == 1000


def test_moments_summary():
    raw = np.zeros((13, 2))
    raw[0] = 4
    raw[1], raw[2] = (2.0, -4.0), (16.0, 36.0)
    raw[5], raw[6] = (np.inf, 8.0), (np.inf, 64.0)
    raw[3:5] = [[-1.0, -2.0], [3.0, 0.5]]
    s = native.moments_summary(raw)
    np.testing.assert_array_equal(s["count"], [4, 4])
    np.testing.assert_array_equal(s["resid_mean"], [0.5, -1.0])
    np.testing.assert_array_equal(s["resid_rms"], [2.0, 3.0])
    np.testing.assert_array_equal(s["resp_mean"], [np.inf, 2.0])
    np.testing.assert_array_equal(s["resp_rms"], [np.inf, 4.0])
    np.testing.assert_array_equal(s["resid_min"], [-1.0, -2.0])
    assert set(s) == {"count", "resid_mean", "resid_rms", "resid_min", "resid_max", "resp_mean", "resp_rms", "before_min",
                      "before_max", "after_min", "after_max", "sum_min", "sum_max"}


def _project(tmp_path, data_dimension):
    np.savez(str(tmp_path / "d.npz"), data=np.ones((8, 5)), names=np.array([f"c{k}" for k in range(5)]))
    os.makedirs(tmp_path / "decompressed_output")
    np.savez(str(tmp_path / "decompressed_output" / "decompressed.npz"), data=np.ones((8, 5)),
             names=np.array([f"c{k}" for k in range(5)]))
    return types.SimpleNamespace(input_path=str(tmp_path / "d.npz"), data_dimension=data_dimension)


def test_report_refuses_2d_before_gpu_work(tmp_path, monkeypatch):
    monkeypatch.setattr(native, "require_gpu", lambda: pytest.fail("GPU touched before the refusal"))
    from baler_amd import baler
    c = _project(tmp_path, 2)
    with pytest.raises(NotImplementedError, match="plot_2D"):
        baler.perform_report(str(tmp_path), c, False)
    with pytest.raises(NotImplementedError, match="plot_2D"):
        helper.column_report(c, str(tmp_path))


def test_report_without_gpu_fails_loudly(tmp_path, monkeypatch):
    def no_gpu():
        raise native.NativeError("no MI355X (gfx950) device visible: the baler_amd hot path has no CPU fallback")
    monkeypatch.setattr(native, "require_gpu", no_gpu)
    from baler_amd import baler
    with pytest.raises(native.NativeError):
        baler.perform_report(str(tmp_path), _project(tmp_path, 1), False)
    assert not os.path.exists(tmp_path / "plotting" / "column_stats.npz")


def test_plot_mode_still_raises_and_points_at_report(monkeypatch):
    from baler_amd import baler
    monkeypatch.setattr(helper, "get_arguments", lambda argv=None: (None, "plot", "w", "p", False))
    with pytest.raises(NameError, match="consumes artefacts only") as e:
        baler.main([])
    assert "--mode report" in str(e.value)


def test_fixture_holds_what_the_reference_drew(golden):
    g = golden("g21_colstats.npz")
    assert str(g["source"]) == "reference plot_1D, unmodified"
    assert g["before"].shape == g["after"].shape == (2000, 6) and g["before"].dtype == np.float64
    np.testing.assert_array_equal(g["edges_response"], np.tile(np.arange(-20, 20, 0.1), (6, 1)))
    np.testing.assert_array_equal(g["edges_residual"], np.tile(np.arange(-1, 1, 0.01), (6, 1)))
    keep = ~(g["before"][:, 3] < 1e-6)
    assert 0 < (~keep).sum() < 200 and (g["before"][:, 1] == 0).sum() >= 3
    s = g["before"][keep] + g["after"][keep]
    for k in range(6):      # the value bins follow from the before + after extrema through the helper's expression
        np.testing.assert_array_equal(helper.report_value_edges(s[:, k].min(), s[:, k].max()), g["edges_before"][k])
    with np.errstate(all="ignore"):
        resp = (g["after"][keep] - g["before"][keep]) / g["before"][keep] * 100
    assert np.isinf(resp[:, 1]).any() and np.isnan(resp[:, 1]).any()
