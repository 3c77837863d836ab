"""colbox.box_stats over native.column_hist on the GPU against matplotlib.cbook.boxplot_stats, bit for bit: the fixture g22 (float64 and
float32), the seeded cases of the CPU test, row chunks against one call, and helper.column_report with the chunks resident on the device
against streamed again every round."""
import os
import types

import numpy as np
import pytest
import torch

import colbox_cases as cc
from baler_amd import colbox, native
from baler_amd.modules import helper

pytestmark = pytest.mark.gpu


def gpu_hist(before, after, cut, chunk=None, calls=None):
    bd, ad = torch.as_tensor(before).cuda(), torch.as_tensor(after).cuda()
    n = len(before)
    chunk = chunk or max(n, 1)

    def hist(edges):
        e = torch.as_tensor(np.ascontiguousarray(edges)).cuda()
        got = native.column_hist(bd[:0], ad[:0], edges_resid=e, cut=cut)
        for lo in range(0, n, chunk):
            native.column_hist(bd[lo:lo + chunk], ad[lo:lo + chunk], edges_resid=e, cut=cut, out=got)
        if calls is not None:
            calls.append(edges.shape)
        return got["resid"].cpu().numpy()
    return hist


def gpu_box(before, after, cut, dtype, chunk=None):
    cut = helper.report_kernel_cut(cut, dtype)            # numpy's float32 comparison in the ABI's float64 terms
    s = native.column_moments(torch.as_tensor(before).cuda(), torch.as_tensor(after).cuda(), cut)
    calls = []
    got, info = colbox.box_stats(s["count"], s["resid_min"], s["resid_max"], gpu_hist(before, after, cut, chunk, calls), dtype)
    assert info["rounds"] == len(calls) and all(k <= 1025 for _, k in calls)
    return got, info


@pytest.mark.parametrize("tag, dtype", [("f64", np.float64), ("f32", np.float32)])
def test_g22(golden, tag, dtype):
    g = golden("g22_boxplot.npz")
    b, a = g[f"before_{tag}"], g[f"after_{tag}"]
    got, info = gpu_box(b, a, (3, 1e-6), dtype)
    np.testing.assert_array_equal(np.stack([got[k] for k in colbox.BOX_KEYS[:5]], axis=1), g[f"stats_{tag}"])
    edge = got["box_edge"]
    np.testing.assert_array_equal(np.array([-edge - edge * 0.1, edge + edge * 0.1]), g[f"xlim_{tag}"])
    chunked, info2 = gpu_box(b, a, (3, 1e-6), dtype, chunk=333)
    for k in colbox.BOX_KEYS:
        np.testing.assert_array_equal(chunked[k], got[k])
    assert info2 == info
    print(f"g22 {tag}: {info}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_seeded_cases(dtype):
    for name, (b, a) in cc.seeded_cases(dtype).items():
        cut = cc.cut_of(b.shape[1])
        got, info = gpu_box(b, a, cut, dtype, chunk=1001 if len(b) > 1001 else None)
        cc.check_box(got, cc.residual(b, a, cut), f"{name} {np.dtype(dtype).name}")
        assert info["quartile_rounds"] <= colbox.round_bound(dtype, 6), name
        assert info["whisker_rounds"] <= colbox.round_bound(dtype, 2, shared_first=False), name


@pytest.mark.parametrize("tag, dtype", [("f64", np.float64), ("f32", np.float32)])
def test_report_resident_equals_streamed(golden, tmp_path, capsys, tag, dtype):
    g = golden("g22_boxplot.npz")
    b, a = g[f"before_{tag}"], g[f"after_{tag}"]
    os.makedirs(tmp_path / "out" / "decompressed_output")
    np.savez(tmp_path / "in.npz", data=b, names=g["names"])
    np.savez(tmp_path / "out" / "decompressed_output" / "decompressed.npz", data=a, names=g["names"])

    def report(**kw):
        cfg = types.SimpleNamespace(data_dimension=1, input_path=str(tmp_path / "in.npz"), **kw)
        r = helper.column_report(cfg, str(tmp_path / "out"))
        return r, dict(np.load(tmp_path / "out" / "plotting" / "column_stats.npz")), capsys.readouterr().out

    res, on_disk, text = report()
    assert "=== Box and whisker ===" in text and "resident" in text and text.count("residual mean") == b.shape[1]
    np.testing.assert_array_equal(np.stack([res[k] for k in colbox.BOX_KEYS[:5]], axis=1), g[f"stats_{tag}"])
    streamed, on_disk2, text2 = report(report_box_resident_mb=0, report_chunk_rows=700)
    assert "streamed" in text2
    for k in colbox.BOX_KEYS:
        np.testing.assert_array_equal(streamed[k], res[k])
        np.testing.assert_array_equal(on_disk[k], res[k])
        np.testing.assert_array_equal(on_disk2[k], res[k])
    off, on_disk3, text3 = report(report_box=False)
    assert "Box and whisker" not in text3 and not set(colbox.BOX_KEYS) & set(off) and not set(colbox.BOX_KEYS) & set(on_disk3)
    assert set(on_disk3) | set(colbox.BOX_KEYS) == set(on_disk)
    for k in on_disk3:
        np.testing.assert_array_equal(on_disk3[k], on_disk[k])
