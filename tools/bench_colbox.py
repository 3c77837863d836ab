#!/usr/bin/env python3
"""Time the box-and-whisker statistics of the report mode (colbox.box_stats over bamd_column_hist with per-column edges) beside the
two sweeps the report had before, and beside single-threaded numpy on the same residuals.

Run:  python tools/bench_colbox.py [--out profiles/colbox_bench.json]

Per table (1M x 24 float64, 1M x 24 float32, 12.5M x 24 float64), wall-clock milliseconds with a device synchronise at both ends, one
warm-up run first, then the MEDIAN of five samples:
  report_sweeps_ms    bamd_column_moments + bamd_column_hist with the reference's bins: the report without c.report_box
  box_resident_ms     box_stats, every round one call over the table held on the device (what the report adds when the rank's
                      slices fit in c.report_box_resident_mb)
  box_streamed_ms     box_stats, every round copies the two tables from pinned host memory in chunks of hostio.CHUNK_BYTES and counts chunk by
                      chunk (what the report adds otherwise; the file reads of the real report are not in it)
  rounds              the hist calls box_stats made, by phase
  numpy_ms            np.percentile([25, 50, 75]) plus the fences and whiskers, column by column, one thread, timed once
The results of the three ways are checked equal before anything is timed."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from baler_amd import colbox, hostio, native  # noqa: E402
from baler_amd.modules import helper  # noqa: E402

CUT = (3, 1e-6)


def wall_ms(fn, samples=5):
    fn()
    got = []
    for _ in range(samples):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        got.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(got))


def tables(n, c, dtype):
    g = torch.Generator(device="cuda").manual_seed(1)
    before = torch.randn((n, c), generator=g, device="cuda", dtype=dtype) * 2 + 5
    before[:, 3] = before[:, 3].abs()
    after = before + 0.05 * torch.randn((n, c), generator=g, device="cuda", dtype=dtype)
    return before, after


def numpy_box(resid):
    out = []
    for k in range(resid.shape[1]):
        x = resid[:, k]
        q1, med, q3 = np.percentile(x, [25, 50, 75])
        iqr = q3 - q1
        lo, hi = q1 - 1.5 * iqr, q3 + 1.5 * iqr
        wl, wh = x[x >= lo], x[x <= hi]
        out.append([q1, med, q3, wl.min() if len(wl) and wl.min() <= q1 else q1, wh.max() if len(wh) and wh.max() >= q3 else q3])
    return np.array(out, dtype=np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "colbox_bench.json"))
    args = ap.parse_args()
    native.require_gpu()
    torch.set_num_threads(1)
    res = {"device": torch.cuda.get_device_name(0), "cut": list(CUT), "bins": colbox.BINS, "chunk_bytes": hostio.CHUNK_BYTES, "entries": []}
    e_resp = torch.as_tensor(helper.report_response_edges()).cuda()
    e_resid = torch.as_tensor(helper.report_residual_edges()).cuda()
    for n, c, dtype in ((1_000_000, 24, torch.float64), (1_000_000, 24, torch.float32), (12_500_000, 24, torch.float64)):
        before, after = tables(n, c, dtype)
        npdt = np.float64 if dtype == torch.float64 else np.float32
        raw = native.column_moments_raw(before, after, CUT)
        s = native.moments_summary(raw)
        e_val = torch.as_tensor(np.stack([np.asarray(helper.report_value_edges(lo, hi), np.float64)
                                          for lo, hi in zip(s["sum_min"], s["sum_max"])])).cuda()
        counts = native.column_hist(before, after, e_resp, e_resid, e_val, CUT)

        def sweeps():
            native.column_moments_raw(before, after, CUT, out=raw)
            native.column_hist(before, after, e_resp, e_resid, e_val, CUT, out=counts)

        hb, ha = before.cpu().pin_memory(), after.cpu().pin_memory()
        rows = max(1, hostio.CHUNK_BYTES // (2 * c * before.element_size()))

        def hist_resident(edges):
            return native.column_hist(before, after, edges_resid=torch.as_tensor(edges).cuda(), cut=CUT)["resid"].cpu().numpy()

        def hist_streamed(edges):
            e = torch.as_tensor(edges).cuda()
            got = native.column_hist(before[:0], after[:0], edges_resid=e, cut=CUT)
            for lo in range(0, n, rows):
                native.column_hist(hb[lo:lo + rows].cuda(non_blocking=True), ha[lo:lo + rows].cuda(non_blocking=True), edges_resid=e, cut=CUT,
                                   out=got)
            return got["resid"].cpu().numpy()

        box = lambda hist: colbox.box_stats(s["count"], s["resid_min"], s["resid_max"], hist, npdt)      # noqa: E731
        got_r, info = box(hist_resident)
        got_s, info_s = box(hist_streamed)
        keep = ~(hb[:, 3].numpy() < 1e-6)
        resid = np.subtract(ha.numpy()[keep], hb.numpy()[keep])
        t0 = time.perf_counter()
        want = numpy_box(resid)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        have = np.stack([got_r[k] for k in colbox.BOX_KEYS[:5]], axis=1)
        assert np.array_equal(have, want) and info == info_s and all(np.array_equal(got_r[k], got_s[k]) for k in colbox.BOX_KEYS)
        del resid
        entry = {"rows": n, "cols": c, "dtype": str(dtype).split(".")[-1], "report_sweeps_ms": round(wall_ms(sweeps), 3),
                 "box_resident_ms": round(wall_ms(lambda: box(hist_resident)), 3),
                 "box_streamed_ms": round(wall_ms(lambda: box(hist_streamed)), 3), "rounds": info, "numpy_ms": round(numpy_ms, 1)}
        res["entries"].append(entry)
        print(entry, flush=True)
        del before, after, hb, ha
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
