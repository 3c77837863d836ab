#!/usr/bin/env python3
"""Time bamd_column_moments (pass A) and bamd_column_hist (pass B) and the numpy restatement of the same statistics.

Run:  python tools/bench_colstats.py [--out profiles/colstats_bench.json] [--no-numpy]

Timing as tests/test_gpu_perf_floor.py::_ms: ~30 ms of the same call first, then the MEDIAN of five event-timed samples.  Every
entry carries bytes read / time next to the plain-load HBM streaming rate of the chip (6.0-6.3 TB/s measured for 16-byte loads).
The numpy restatement (single-threaded, as the reference runs it; statistics only, no loading or drawing) is timed once at
1M x 24 float64."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from baler_amd import native  # noqa: E402
from baler_amd.modules import helper  # noqa: E402

HBM_STREAM_TBS = 6.0      # plain 16-byte loads sweeping a table that does not fit the Infinity Cache
CUT = (3, 1e-6)


def _ms(fn, reps, warm_ms=30.0, samples=5):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    for _ in range(min(200, int(warm_ms / max(e0.elapsed_time(e1), 1e-3)))):
        fn()
    got = []
    for _ in range(samples):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        got.append(e0.elapsed_time(e1) / reps)
    return float(np.median(got))


def tables(n, c, dtype):
    g = torch.Generator(device="cuda").manual_seed(1)
    before = torch.randn((n, c), generator=g, device="cuda", dtype=dtype) * 2 + 5
    before[:, 3] = before[:, 3].abs()
    after = before + 0.05 * torch.randn((n, c), generator=g, device="cuda", dtype=dtype)
    return before, after


def numpy_stats(before, after):
    """plot_1D's statistics (plotting.py:118-234) on (columns, rows) arrays, as the reference holds them."""
    cut = np.argwhere(before[3] < 1e-6).flatten()
    before, after = np.delete(before, cut, axis=1), np.delete(after, cut, axis=1)
    response = np.divide(np.subtract(after, before), before) * 100
    residual = np.subtract(after, before)
    for k in range(before.shape[0]):
        np.sqrt(np.mean(np.square(response[k])))
        np.sqrt(np.mean(np.square(residual[k])))
        s = before[k] + after[k]
        x_min, x_max = s.min(), s.max()
        d = abs(x_max - x_min)
        bins = np.linspace(x_min - 0.1 * d, x_max + 0.1 * d, 200)
        np.histogram(before[k], bins=bins)
        np.histogram(after[k], bins=bins)
        np.histogram(response[k], bins=np.arange(-20, 20, 0.1))
        np.mean(response[k])
        np.histogram(residual[k], bins=np.arange(-1, 1, 0.01))
        np.mean(residual[k]), residual[k].max(), residual[k].min()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "colstats_bench.json"))
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()
    native.require_gpu()
    res = {"device": torch.cuda.get_device_name(0), "hbm_stream_tbs": HBM_STREAM_TBS, "cut": list(CUT), "entries": []}
    e_resp = torch.as_tensor(helper.report_response_edges()).cuda()
    e_resid = torch.as_tensor(helper.report_residual_edges()).cuda()
    for n, c, dtype in ((1_000_000, 24, torch.float64), (1_000_000, 24, torch.float32), (12_500_000, 24, torch.float64)):
        before, after = tables(n, c, dtype)
        raw = native.column_moments_raw(before, after, CUT)
        s = native.moments_summary(raw)
        e_val = torch.as_tensor(np.stack([np.asarray(helper.report_value_edges(lo, hi), np.float64)
                                          for lo, hi in zip(s["sum_min"], s["sum_max"])])).cuda()
        counts = native.column_hist(before, after, e_resp, e_resid, e_val, CUT)
        reps = 20 if n <= 1_000_000 else 3
        ms_a = _ms(lambda: native.column_moments_raw(before, after, CUT, out=raw), reps)
        ms_b = _ms(lambda: native.column_hist(before, after, e_resp, e_resid, e_val, CUT, out=counts), reps)
        nbytes = 2 * before.numel() * before.element_size()
        for name, ms in (("moments", ms_a), ("hist", ms_b)):
            tbs = nbytes / (ms * 1e-3) / 1e12
            res["entries"].append({"pass": name, "rows": n, "cols": c, "dtype": str(dtype).split(".")[-1], "ms": round(ms, 4),
                                   "bytes_read": nbytes, "tb_per_s": round(tbs, 3), "fraction_of_hbm_stream": round(tbs / HBM_STREAM_TBS, 3)})
            print(res["entries"][-1], flush=True)
        if n == 1_000_000 and dtype == torch.float64 and not args.no_numpy:
            torch.set_num_threads(1)
            hb, ha = np.ascontiguousarray(before.cpu().numpy().T), np.ascontiguousarray(after.cpu().numpy().T)
            with np.errstate(all="ignore"):
                t0 = time.perf_counter()
                numpy_stats(hb, ha)
                t_np = time.perf_counter() - t0
            res["numpy_1m_x24_f64_s"] = round(t_np, 3)
            res["numpy_over_gpu_1m_x24_f64"] = round(t_np * 1e3 / (ms_a + ms_b), 1)
            print(f"numpy restatement {t_np:.3f} s = {res['numpy_over_gpu_1m_x24_f64']} x (pass A + pass B)", flush=True)
        del before, after
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
