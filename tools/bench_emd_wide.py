#!/usr/bin/env python3
"""Times bamd_emd_rows against the same quantity from torch.sort: 8192 rows of 100 / 256 / 625 / 2500 / 4096 columns, float32 and float64.

Run on the GPU:  python tools/bench_emd_wide.py [out.json]      (profiles/emd_wide.json was made with it)

Per shape: the call time of native.emd_rows (both launches) and of the torch expression, timed as tests/test_gpu_perf_floor.py times
(_ms: 30 ms of the same call, then the median of five event-timed samples of three calls), the bytes of both tables read once and
the rate that gives, and the relative difference of the two results."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402

from baler_amd import native  # noqa: E402
from test_gpu_perf_floor import _ms  # noqa: E402

ROWS = 8192


def main(out):
    native.require_gpu()
    res = []
    for dtype in (torch.float32, torch.float64):
        for c in (100, 256, 625, 2500, 4096):
            g = torch.Generator(device="cuda").manual_seed(c)
            x = torch.rand((ROWS, c), dtype=dtype, device="cuda", generator=g)
            r = (x * (1.0 + 0.05 * torch.randn(x.shape, dtype=dtype, device="cuda", generator=g))).contiguous()

            def with_torch():
                return (torch.sort(x, 1)[0].double() - torch.sort(r, 1)[0].double()).abs().mean(1).sum()
            a, b = native.emd_rows(x, r).item(), with_torch().item()
            tk, tt = _ms(lambda: native.emd_rows(x, r), 3), _ms(with_torch, 3)
            nbytes = 2 * ROWS * c * x.element_size()
            row = {"rows": ROWS, "cols": c, "dtype": str(dtype).replace("torch.", ""), "kernel_ms": round(tk, 4), "torch_ms": round(tt, 4),
                   "speedup": round(tt / tk, 2), "read_bytes": nbytes, "read_TBps": round(nbytes / tk / 1e9, 3),
                   "share_of_8TBps_HBM": round(nbytes / tk / 1e9 / 8.0, 3), "rel_diff_vs_torch": abs(a - b) / abs(b)}
            print(row, flush=True)
            res.append(row)
    if out:
        with open(out, "w") as f:
            json.dump({"rows": res}, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
