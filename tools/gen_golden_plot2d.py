#!/usr/bin/env python3
"""Generate tests/golden/g23_plot2d.npz by RUNNING the reference's plotting.plot_2D (authoring machine only).

Run:  python tools/gen_golden_plot2d.py <reference checkout>

Writes data only: small synthetic (before, after) frame tables and what plot_2D handed to matplotlib for them.  plot_2D
(plotting.py:370-437) draws three ``imshow(..., vmin=min_value, vmax=max_value)`` panels per frame -- original, reconstructed,
difference -- so wrapping ``matplotlib.axes.Axes.imshow`` for the duration of the run records, per frame, the colour scale and the
difference image.  ``Figure.savefig`` is a no-op meanwhile: the pages are not wanted.  The reference runs unmodified (Agg backend).

Three runs on seeded (7, 12, 9) tables with both signs and finite values: float64 ("f64"), float32 ("f32"), and float64 with
convert_to_blocks set and the decompressed array stored flat per frame, (7, 108) ("blocks"; plot_2D reshapes it,
plotting.py:388-391).
"""
import os
import sys
import tempfile
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")

import matplotlib  # noqa: E402

matplotlib.use("Agg")
import numpy as np  # noqa: E402
from matplotlib.axes import Axes  # noqa: E402
from matplotlib.figure import Figure  # noqa: E402

SHAPE = (7, 12, 9)
RUNS = (("f64", np.float64, False), ("f32", np.float32, False), ("blocks", np.float64, True))


def tables(seed, dtype):
    """before: smooth fields of both signs, another scale in every frame; after: before with a perturbation of a few per cent."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(-1.0, 1.0, SHAPE[1]), np.linspace(-1.0, 1.0, SHAPE[2]), indexing="ij")
    before = np.stack([(k + 1.0) * np.sin(3.0 * x + k) * np.cos(2.0 * y - k) + rng.normal(0.0, 0.1, SHAPE[1:]) for k in range(SHAPE[0])])
    after = before + rng.normal(0.0, 0.03, SHAPE) * (1.0 + np.arange(SHAPE[0]))[:, None, None]
    return before.astype(dtype), after.astype(dtype)


def run_reference(ref_plotting, before, after, blocks):
    scratch = tempfile.mkdtemp(prefix="baler_golden_plot2d_")
    os.makedirs(os.path.join(scratch, "out", "decompressed_output"))
    os.makedirs(os.path.join(scratch, "out", "plotting"))
    np.savez(os.path.join(scratch, "in.npz"), data=before)
    stored = after.reshape(after.shape[0], -1) if blocks else after
    np.savez(os.path.join(scratch, "out", "decompressed_output", "decompressed.npz"), data=stored)

    panels = []
    orig_imshow, orig_savefig = Axes.imshow, Figure.savefig

    def imshow(self, X, *a, **kw):
        panels.append((np.array(X, copy=True), kw["vmin"], kw["vmax"]))
        return orig_imshow(self, X, *a, **kw)

    Axes.imshow, Figure.savefig = imshow, lambda self, *a, **kw: None
    try:
        ref_plotting.plot_2D(os.path.join(scratch, "out"),
                             types.SimpleNamespace(input_path=os.path.join(scratch, "in.npz"), convert_to_blocks=blocks))
    finally:
        Axes.imshow, Figure.savefig = orig_imshow, orig_savefig
        matplotlib.pyplot.close("all")
    n = before.shape[0]
    assert len(panels) == 3 * n, len(panels)
    for k in range(n):          # a check of the recording, not of the reference: the first two panels are the two tiles
        assert np.array_equal(panels[3 * k][0], before[k]) and np.array_equal(panels[3 * k + 1][0], after[k])
        assert panels[3 * k][1:] == panels[3 * k + 1][1:] == panels[3 * k + 2][1:]
    vmin = np.array([panels[3 * k + 2][1] for k in range(n)])
    vmax = np.array([panels[3 * k + 2][2] for k in range(n)])
    diff = np.stack([panels[3 * k + 2][0] for k in range(n)])
    return stored, vmin, vmax, diff


def main(ref):
    sys.path.insert(0, ref)
    import matplotlib.pyplot  # noqa: F401
    from baler.modules import plotting as ref_plotting

    rec = {}
    for i, (name, dtype, blocks) in enumerate(RUNS):
        before, after = tables(2300 + i, dtype)
        stored, vmin, vmax, diff = run_reference(ref_plotting, before, after, blocks)
        assert vmin.dtype == dtype and vmax.dtype == dtype and diff.dtype == dtype and diff.shape == SHAPE, (vmin.dtype, diff.dtype)
        assert (before < 0).any() and (before > 0).any() and np.isfinite(before).all() and np.isfinite(after).all()
        rec.update({f"{name}_before": before, f"{name}_after": stored, f"{name}_vmin": vmin, f"{name}_vmax": vmax, f"{name}_diff": diff})
    path = os.path.join(OUT, "g23_plot2d.npz")
    np.savez_compressed(path, source=np.array("reference plot_2D, unmodified"), runs=np.array([r[0] for r in RUNS]), **rec)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; {len(RUNS)} runs of {SHAPE[0]} frames")


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
