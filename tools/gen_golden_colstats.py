#!/usr/bin/env python3
"""Generate tests/golden/g21_colstats.npz by RUNNING the reference's plotting.plot_1D (authoring machine only).

Run:  python tools/gen_golden_colstats.py <reference checkout>

Writes data only: a small synthetic (before, after) table pair, the column names, and what plot_1D handed to matplotlib for it.
plot_1D (plotting.py:101-239) draws every histogram as ``hist(bins[:-1], bins, weights=counts)``, marks the means with ``axvline``
and puts the rounded RMS / Max / Min into the labels of empty ``plot`` calls, so wrapping ``matplotlib.axes.Axes.hist``, ``axvline``
and ``plot`` for the duration of the run records the exact edges and counts of all four histograms per column, the means and the
label texts.  The reference runs unmodified (Agg backend); the pages it draws are thrown away.
"""
import os
import re
import sys
import tempfile
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")

import matplotlib  # noqa: E402

matplotlib.use("Agg")
import numpy as np  # noqa: E402
from matplotlib.axes import Axes  # noqa: E402

N_ROWS, N_COLS = 2000, 6
NAMES = np.array([f"recoPFJets_ak5PFJets__RECO.obj.col{k}_" for k in range(N_COLS)])


def tables():
    """before: six columns of different scales; column 3 (the reference's cut column) has rows below 1e-6, column 1 a few exact
    zeros (its response then holds +-inf and NaN).  after: before with a perturbation that puts residuals and responses on both
    sides of several bin edges of np.arange(-1, 1, 0.01) / np.arange(-20, 20, 0.1), some of them outside the binned range."""
    rng = np.random.default_rng(2110)
    before = np.empty((N_ROWS, N_COLS))
    before[:, 0] = rng.normal(50.0, 20.0, N_ROWS)
    before[:, 1] = rng.normal(0.0, 1.0, N_ROWS)
    before[:, 2] = rng.uniform(-3.0, 3.0, N_ROWS)
    before[:, 3] = np.abs(rng.normal(0.0, 1.0, N_ROWS))
    before[:, 4] = rng.exponential(5.0, N_ROWS)
    before[:, 5] = np.trunc(rng.uniform(0.0, 40.0, N_ROWS))
    before[rng.choice(N_ROWS, 60, replace=False), 3] = rng.uniform(0.0, 9e-7, 60)       # rows the cut removes
    before[7, 3] = 1e-6                                                                 # on the threshold: kept
    zeros = rng.choice(N_ROWS, 8, replace=False)
    before[zeros, 1] = 0.0
    after = before + rng.normal(0.0, 0.05, before.shape) * np.array([1.0, 0.2, 0.5, 0.1, 4.0, 8.0])
    after[zeros[:3], 1] = 0.0                                                           # 0 / 0 -> NaN; the others -> +-inf
    # residuals exactly on, just below and just above edges of np.arange(-1, 1, 0.01)
    e = np.arange(-1, 1, 0.01)
    for i, k in enumerate((0, 37, 100, 150, 199)):
        for j, v in enumerate((np.nextafter(e[k], -np.inf), e[k], np.nextafter(e[k], np.inf))):
            r = 100 + 3 * i + j
            after[r, 2] = before[r, 2] + v
    return before, after


def main(ref):
    scratch = tempfile.mkdtemp(prefix="baler_golden_colstats_")
    os.makedirs(os.path.join(scratch, "out", "decompressed_output"))
    os.makedirs(os.path.join(scratch, "out", "plotting"))
    before, after = tables()
    np.savez(os.path.join(scratch, "in.npz"), data=before, names=NAMES)
    np.savez(os.path.join(scratch, "out", "decompressed_output", "decompressed.npz"), data=after, names=NAMES)

    sys.path.insert(0, ref)
    from baler.modules import plotting as ref_plotting

    hists, vlines, labels = [], [], []
    orig = Axes.hist, Axes.axvline, Axes.plot

    def hist(self, x, bins=None, **kw):
        if "weights" in kw:
            hists.append((np.array(bins, copy=True), np.array(kw["weights"], copy=True)))
        return orig[0](self, x, bins, **kw)

    def axvline(self, x=0, *a, **kw):
        vlines.append(float(x))
        return orig[1](self, x, *a, **kw)

    def plot(self, *a, **kw):
        if str(kw.get("label", "")).startswith(("RMS:", "Max:", "Min:")):       # (the box plot's lines carry labels too)
            labels.append(str(kw["label"]))
        return orig[2](self, *a, **kw)

    Axes.hist, Axes.axvline, Axes.plot = hist, axvline, plot
    try:
        with np.errstate(all="ignore"):
            ref_plotting.plot_1D(os.path.join(scratch, "out"), types.SimpleNamespace(input_path=os.path.join(scratch, "in.npz")))
    finally:
        Axes.hist, Axes.axvline, Axes.plot = orig

    assert len(hists) == 4 * N_COLS and len(vlines) == 2 * N_COLS and len(labels) == 4 * N_COLS, (len(hists), len(vlines), len(labels))
    order = ("before", "after", "response", "residual")             # the order plot_1D draws a column's histograms in
    rec = {}
    for i, name in enumerate(order):
        rec[f"edges_{name}"] = np.stack([hists[4 * k + i][0] for k in range(N_COLS)]).astype(np.float64)
        rec[f"counts_{name}"] = np.stack([hists[4 * k + i][1] for k in range(N_COLS)]).astype(np.int64)
    assert rec["edges_before"].shape[1] == 200 and rec["edges_response"].shape[1] == 400 and rec["edges_residual"].shape[1] == 200
    assert np.array_equal(rec["edges_before"], rec["edges_after"])
    num = lambda s: float(re.search(r":\s*(\S+)", s).group(1))      # noqa: E731  "RMS: 0.1234 %" -> 0.1234
    rec["resp_mean"] = np.array(vlines[0::2])
    rec["resid_mean"] = np.array(vlines[1::2])
    rec["resp_rms_rounded"] = np.array([num(labels[4 * k]) for k in range(N_COLS)])            # round(rms, 4)
    rec["resid_rms_rounded"] = np.array([num(labels[4 * k + 1]) for k in range(N_COLS)])       # round(.., 6)
    rec["resid_max_rounded"] = np.array([num(labels[4 * k + 2]) for k in range(N_COLS)])
    rec["resid_min_rounded"] = np.array([num(labels[4 * k + 3]) for k in range(N_COLS)])

    # the recorded residual counts are np.histogram of the rows that pass the cut (a check of the recording, not of the reference)
    keep = ~(before[:, 3] < 1e-6)
    for k in range(N_COLS):
        want = np.histogram((after - before)[keep, k], bins=np.arange(-1, 1, 0.01))[0]
        assert np.array_equal(rec["counts_residual"][k], want), k
    path = os.path.join(OUT, "g21_colstats.npz")
    np.savez_compressed(path, before=before, after=after, names=NAMES, source=np.array("reference plot_1D, unmodified"), **rec)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; {len(hists)} hist calls, {int((~keep).sum())} rows cut")


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
