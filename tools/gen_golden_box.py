#!/usr/bin/env python3
"""Generate tests/golden/g22_boxplot.npz by RUNNING the reference's plotting.plot_1D (authoring machine only).

Run:  python tools/gen_golden_box.py <reference checkout>

Writes data only.  The tables are those of g21 (tools/gen_golden_colstats.tables()), once as float64 and once cast to float32.
plot_1D's first page is plot_box_and_whisker (plotting.py:76-98): ``Axes.boxplot`` computes matplotlib's boxplot_stats per column and
hands them to ``Axes.bxp``, then the page's x axis is set with ``Axes.set_xlim``.  Wrapping ``bxp`` and ``set_xlim`` for the duration
of the run records the five statistics per column as matplotlib computed them and the x limits the reference chose.  The reference runs
unmodified (Agg backend); the pages it draws are thrown away.
"""
import os
import sys
import tempfile
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, os.path.join(REPO, "tools"))

import matplotlib  # noqa: E402

matplotlib.use("Agg")
import numpy as np  # noqa: E402
from matplotlib.axes import Axes  # noqa: E402

import gen_golden_colstats as g21  # noqa: E402

KEYS = ("q1", "med", "q3", "whislo", "whishi")


def record(ref_plotting, before, after):
    scratch = tempfile.mkdtemp(prefix="baler_golden_box_")
    os.makedirs(os.path.join(scratch, "out", "decompressed_output"))
    os.makedirs(os.path.join(scratch, "out", "plotting"))
    np.savez(os.path.join(scratch, "in.npz"), data=before, names=g21.NAMES)
    np.savez(os.path.join(scratch, "out", "decompressed_output", "decompressed.npz"), data=after, names=g21.NAMES)
    boxes, xlims = [], []
    orig = Axes.bxp, Axes.set_xlim

    def bxp(self, bxpstats, *a, **kw):
        boxes.append([{k: float(s[k]) for k in KEYS} for s in bxpstats])
        return orig[0](self, bxpstats, *a, **kw)

    def set_xlim(self, *a, **kw):
        if len(boxes) == 1 and not xlims and len(a) == 2:  # the first (left, right) call after the box page's bxp: plotting.py:97
            xlims.append((float(a[0]), float(a[1])))
        return orig[1](self, *a, **kw)

    Axes.bxp, Axes.set_xlim = bxp, set_xlim
    try:
        with np.errstate(all="ignore"):
            ref_plotting.plot_1D(os.path.join(scratch, "out"), types.SimpleNamespace(input_path=os.path.join(scratch, "in.npz")))
    finally:
        Axes.bxp, Axes.set_xlim = orig
    assert len(boxes) == 1 and len(boxes[0]) == g21.N_COLS and len(xlims) == 1, (len(boxes), len(xlims))
    stats = np.array([[s[k] for k in KEYS] for s in boxes[0]], dtype=np.float64)          # (columns, 5)
    return stats, np.array(xlims[0], dtype=np.float64)


def main(ref):
    sys.path.insert(0, ref)
    from baler.modules import plotting as ref_plotting

    before, after = g21.tables()
    rec = {}
    for tag, dt in (("f64", np.float64), ("f32", np.float32)):
        b, a = before.astype(dt), after.astype(dt)
        stats, xlim = record(ref_plotting, b, a)
        rec[f"before_{tag}"], rec[f"after_{tag}"] = b, a
        rec[f"stats_{tag}"], rec[f"xlim_{tag}"] = stats, xlim
    path = os.path.join(OUT, "g22_boxplot.npz")
    np.savez_compressed(path, names=g21.NAMES, stat_names=np.array(KEYS), cut=np.array([3.0, 1e-6]),
                        source=np.array("reference plot_box_and_whisker, unmodified"), **rec)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    for tag in ("f64", "f32"):
        print(tag, rec[f"stats_{tag}"][0], rec[f"xlim_{tag}"])


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
