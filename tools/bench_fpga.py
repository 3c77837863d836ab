#!/usr/bin/env python3
"""FPGA_prototype_model(24, 15) throughput: rows/s of encode, decode and train_step at 512 to 1M rows, fp32 and fp64,
fused (fpga.hip) and layer-wise (BALER_AMD_FORCE_GENERIC=1), one JSON line per configuration.  Each line also gives the fraction
of the byte roofline at 6.3 TB/s: the bytes a call must move (rows in, rows out; a training step reads its rows only) over the
time.  Timing: a warm-up call, then the median of five event-timed samples of `reps` back-to-back calls on the launch stream.

Run:  python tools/bench_fpga.py [--rows 512,4096,8192,16384,32768,1048576]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from baler_amd import native  # noqa: E402

HBM = 6.3e12
N, Z = 24, 15


def dims():
    return [N, 20, 10, Z, 10, 20, N]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        samples.append(e0.elapsed_time(e1) / 1e3 / reps)
    return float(np.median(samples))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="512,4096,8192,16384,32768,1048576")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    d = dims()
    flat = np.concatenate([rng.uniform(-0.2, 0.2, d[l + 1] * d[l] + d[l + 1]) for l in range(6)])
    for forced in (False, True):
        if forced:
            os.environ["BALER_AMD_FORCE_GENERIC"] = "1"
        for mode in ("fp32", "fp64"):
            dt = torch.float64 if mode == "fp64" else torch.float32
            h = native.Handle(d, mode, act="relu")
            p = torch.from_numpy(np.concatenate([flat, [0.0]])).to(dt).cuda()
            h.load_params(p)
            m, v = torch.zeros_like(p), torch.zeros_like(p)
            for rows in (int(r) for r in args.rows.split(",")):
                x = torch.rand((rows, N), device="cuda", dtype=dt)
                z = torch.empty((rows, Z), device="cuda", dtype=dt)
                out = torch.empty((rows, N), device="cuda", dtype=dt)
                reps = max(1, min(200, (1 << 22) // rows))
                es = x.element_size()
                t_enc = timed(lambda: h.encode(x, out=z), reps)
                t_dec = timed(lambda: h.decode(z, out=out), reps)
                step = [1]

                def train():
                    h.train_step(x, p, m, v, step[0], 1e-4)
                    step[0] += 1
                t_tr = timed(train, reps)
                line = {"model": "FPGA_prototype_model(24,15)", "path": h.path, "mode": mode, "rows": rows,
                        "encode_rows_per_s": rows / t_enc, "decode_rows_per_s": rows / t_dec,
                        "train_step_rows_per_s": rows / t_tr,
                        "encode_roofline": rows * (N + Z) * es / t_enc / HBM,
                        "decode_roofline": rows * (N + Z) * es / t_dec / HBM,
                        "train_step_roofline": rows * N * es / t_tr / HBM,
                        "encode_us": t_enc * 1e6, "decode_us": t_dec * 1e6, "train_step_us": t_tr * 1e6}
                print(json.dumps(line), flush=True)
            h.close()


if __name__ == "__main__":
    main()
