#!/usr/bin/env python3
"""Generate tests/golden/g22_emd_wide.npz by IMPORTING the reference (authoring machine only; needs scipy, as the reference does).

Run:  python tools/gen_golden_emd_wide.py <reference checkout>

Writes data only: the case names, (columns, rows, seed) per case and the reference's utils.mse_loss_emd_l1(validate=True) of each table
(the summed per-row scipy.stats.wasserstein_distance, utils.py:112-120) on float64 CPU tensors.  The tables themselves are rebuilt from
the seeds by tests/emd_wide_cases.py, here and in the tests, so the file stays at a few hundred bytes.  While generating, oracle/c_oracle's
emd_rows is checked against the reference at 1e-12 (the bar of tests/test_oracle_golden.py::test_g10_emd) and the script aborts if they
disagree.  Same ReduceLROnPlateau(verbose=...) shim as tools/gen_golden.py (utils.py imports the scheduler at module level).
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")

import numpy as np  # noqa: E402
import torch  # noqa: E402

_RLROP = torch.optim.lr_scheduler.ReduceLROnPlateau


class _RLROPShim(_RLROP):
    def __init__(self, *a, verbose=None, **k):
        super().__init__(*a, **k)


torch.optim.lr_scheduler.ReduceLROnPlateau = _RLROPShim


def main(ref):
    sys.path.insert(0, ref)
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from baler.modules import utils as ref_utils

    import emd_wide_cases as cases
    from oracle import c_oracle as orc

    names, meta, sums = [], [], []
    for name, (cols, rows, seed) in cases.CASES.items():
        x, recon = cases.table(name, cols, rows, seed)
        want = float(ref_utils.mse_loss_emd_l1(None, torch.tensor(x), torch.tensor(recon), 0.0, True))
        got = orc.emd_rows(x, recon)
        err = abs(got - want) / abs(want)
        print(f"  {name}: {rows} x {cols}, reference {want:.17g}, oracle rel {err:.3e} (tol 1e-12)")
        if not err <= 1e-12:
            raise SystemExit(f"oracle.emd_rows disagrees with the reference: {name}")
        names.append(name)
        meta.append([cols, rows, seed])
        sums.append(want)
    path = os.path.join(OUT, "g22_emd_wide.npz")
    np.savez(path, names=np.array(names), shapes_seeds=np.array(meta, dtype=np.int64), emd=np.array(sums, dtype=np.float64))
    print("wrote g22_emd_wide.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(os.path.abspath(sys.argv[1]))
