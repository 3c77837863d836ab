#!/usr/bin/env python3
"""Time bamd_frame_stats (with and without the difference image) and bamd_pixel_moments, and the numpy restatement of the same numbers.

Run:  python tools/bench_framestats.py [--out profiles/framestats_bench.json] [--no-numpy]

Timing as tools/bench_colstats.py: ~30 ms of the same call first, then the MEDIAN of five event-timed samples.  Every entry carries
bytes read / time next to the plain-load HBM streaming rate of the chip (6.0-6.3 TB/s measured for 16-byte loads).  Tables:
  262,144 x 2,500 float32   the project's full-size C4 table (50 x 50 frames)
       60 x 2,500 float32   the shipped size
        1 x 4,194,304 float64   one huge frame: the segment path of bamd_frame_stats
The numpy restatement (single-threaded; plot_2D's per-frame amax / amin / subtraction plus the error sums, frame by frame as the
reference loops, then the per-pixel map) runs on the whole table for the two small ones and on the first 4,096 frames of the large
one, scaled by the frame count (it is linear in the frames)."""
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

HBM_STREAM_TBS = 6.0      # plain 16-byte loads sweeping a table that does not fit the Infinity Cache
NUMPY_FRAMES = 4096


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


def tables(n, f, dtype):
    g = torch.Generator(device="cuda").manual_seed(1)
    before = torch.randn((n, f), generator=g, device="cuda", dtype=dtype) * 0.02 + 0.0185
    after = before + 0.001 * torch.randn((n, f), generator=g, device="cuda", dtype=dtype)
    return before, after


def numpy_stats(before, after):
    """plot_2D's numbers (plotting.py:412-418) frame by frame, the per-frame error sums, then the per-pixel map."""
    for k in range(before.shape[0]):
        tile, tile_dec = before[k], after[k]
        diff = tile - tile_dec
        np.amax([np.amax(tile), np.amax(tile_dec)])
        np.amin([np.amin(tile), np.amin(tile_dec)])
        d = diff.astype(np.float64)
        d.min(), d.max(), d.sum(), np.dot(d, d)
        b = tile.astype(np.float64)
        np.dot(b, b)
    d = (before - after).astype(np.float64)
    d.sum(axis=0), np.square(d).sum(axis=0), d.min(axis=0), d.max(axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "framestats_bench.json"))
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()
    native.require_gpu()
    res = {"device": torch.cuda.get_device_name(0), "hbm_stream_tbs": HBM_STREAM_TBS, "entries": []}
    for n, f, dtype in ((262_144, 2_500, torch.float32), (60, 2_500, torch.float32), (1, 4_194_304, torch.float64)):
        before, after = tables(n, f, dtype)
        diff = torch.empty_like(before)
        acc = native.pixel_moments_raw(before, after)
        reps = 3 if n > 100_000 else 50
        nbytes = 2 * before.numel() * before.element_size()
        runs = (("frame_stats", lambda: native.frame_stats(before, after), 0),
                ("frame_stats+diff", lambda: native.frame_stats(before, after, diff), nbytes // 2),
                ("pixel_moments", lambda: native.pixel_moments_raw(before, after, out=acc), 0))
        gpu_ms = {}
        for name, fn, written in runs:
            ms = _ms(fn, reps)
            gpu_ms[name] = ms
            tbs = nbytes / (ms * 1e-3) / 1e12
            res["entries"].append({"pass": name, "frames": n, "frame_elems": f, "dtype": str(dtype).split(".")[-1], "ms": round(ms, 4),
                                   "bytes_read": nbytes, "bytes_written": written, "read_tb_per_s": round(tbs, 3),
                                   "fraction_of_hbm_stream": round(tbs / HBM_STREAM_TBS, 3)})
            print(res["entries"][-1], flush=True)
        if not args.no_numpy:
            torch.set_num_threads(1)
            m = min(n, NUMPY_FRAMES)
            hb, ha = before[:m].cpu().numpy(), after[:m].cpu().numpy()
            t0 = time.perf_counter()
            numpy_stats(hb, ha)
            t_np = (time.perf_counter() - t0) * n / m
            both = gpu_ms["frame_stats+diff"] + gpu_ms["pixel_moments"]
            res["entries"].append({"pass": "numpy", "frames": n, "frame_elems": f, "dtype": str(dtype).split(".")[-1],
                                   "s": round(t_np, 4), "frames_timed": m, "over_gpu_frame_stats_diff_plus_pixel_moments": round(t_np * 1e3 / both, 1)})
            print(res["entries"][-1], flush=True)
        del before, after, diff, acc
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
