#!/usr/bin/env python3
"""PJ_Conv_AE (z = 40) throughput on one MI355X: encode / decode of 1M frames (float32 in and out, with and without normalise-on-load),
a 512-frame and a 65,536-frame training step (bamd_train_step), and as a yardstick the same model restated in eager PyTorch fp32 on
the same GPU (torch's own convolutions and GEMMs; forward / backward by autograd, torch.optim.Adam).  FLOPs per frame are counted
exactly (multiply-adds of taps that land inside the image, x 2); the fraction is of the fp32 MFMA peak, 157.3 TFLOP/s.
Timing: a warm-up call, then the median of five event-timed samples of `reps` back-to-back calls.

Run:  python tools/bench_pjconv.py [--out profiles/pjconv_bench.json] [--no-torch] [--profile-step]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from baler_amd import native  # noqa: E402
from baler_amd.modules import models  # noqa: E402

PEAK = 157.3e12
Z = 40


def conv_macs(hin, hout, cin, cout, transposed):
    """multiply-adds of a k5 / stride 2 / pad 2 (transposed: + output_padding 1) convolution, taps inside the image only"""
    if not transposed:
        valid = sum(1 for o in range(hout) for k in range(5) if 0 <= 2 * o - 2 + k < hin)
    else:
        valid = sum(1 for i in range(hin) for k in range(5) if 0 <= 2 * i - 2 + k < hout)
    return valid * valid * cin * cout


def flops_per_frame(z):
    c0 = conv_macs(28, 14, 1, 20, False)
    c2 = conv_macs(14, 7, 20, 50, False)
    d4 = conv_macs(7, 14, 50, 20, True)
    d5 = conv_macs(14, 28, 20, 1, True)
    lin = 2450 * 500 + 500 * z + z * 500 + 500 * 2450
    fwd = 2 * (c0 + c2 + d4 + d5 + lin)
    enc = 2 * (c0 + c2 + 2450 * 500 + 500 * z)
    # training: forward + input gradients of every layer but encoder.0 + weight gradients of every layer
    train = fwd + 2 * (c2 + d4 + d5 + lin) + 2 * (c0 + c2 + d4 + d5 + lin)
    return {"encode": enc, "decode": fwd - enc, "forward": fwd, "train": train,
            "convs_fwd": 2 * (c0 + c2 + d4 + d5), "linear_fwd": 2 * lin}


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


def torch_model(flat, z):
    ps = []
    for _, off, shape in models.pj_conv_layout(z)[0]:
        ps.append(flat[off:off + int(np.prod(shape))].view(*shape).clone().requires_grad_(True))

    def fwd(x):
        h = F.leaky_relu(F.conv2d(x.view(-1, 1, 28, 28), ps[0], ps[1], stride=2, padding=2), 0.2)
        h = F.conv2d(h, ps[2], ps[3], stride=2, padding=2).reshape(-1, 2450)
        code = F.linear(F.linear(h, ps[4], ps[5]), ps[6], ps[7])
        return code

    def dec(code):
        h = F.linear(F.leaky_relu(F.linear(code, ps[8], ps[9]), 0.2), ps[10], ps[11]).view(-1, 50, 7, 7)
        h = F.conv_transpose2d(h, ps[12], ps[13], stride=2, padding=2, output_padding=1)
        return F.leaky_relu(F.conv_transpose2d(h, ps[14], ps[15], stride=2, padding=2, output_padding=1), 0.2).view(-1, 784)

    return ps, fwd, dec


def line(name, rows, sec, flops, **extra):
    rec = {"name": name, "rows": rows, "us": round(sec * 1e6, 1), "frames_per_s": round(rows / sec),
           "tflops": round(rows * flops / sec / 1e12, 2), "fraction_of_fp32_mfma_peak": round(rows * flops / sec / PEAK, 3)}
    rec.update(extra)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--infer-rows", type=int, default=1 << 20)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--profile-step", action="store_true", help="only 20 512-frame training steps (for a rocprofv3 kernel trace)")
    a = ap.parse_args()
    if a.profile_step:
        torch.manual_seed(0)
        p = torch.cat([models.pj_conv_init(Z), torch.zeros(1)]).cuda()
        h = native.Handle.pj_conv(Z)
        h.load_params(p)
        x = torch.rand((512, 784), device="cuda")
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        for step in range(1, 21):
            h.train_step(x, p, m, v, step, 1e-3)
        torch.cuda.synchronize()
        return
    fl = flops_per_frame(Z)
    out = {"model": f"PJ_Conv_AE(z={Z})", "flops_per_frame": fl, "peak_fp32_mfma_tflops": PEAK / 1e12, "results": []}
    print(json.dumps({"flops_per_frame": fl}), flush=True)
    torch.manual_seed(0)
    flat = models.pj_conv_init(Z).cuda()
    p = torch.cat([flat, torch.zeros(1, device="cuda")])
    h = native.Handle.pj_conv(Z)
    h.load_params(p)
    n = a.infer_rows
    x = torch.rand((n, 784), device="cuda")
    feats = torch.stack([torch.full((784,), -1.0, dtype=torch.float64), torch.full((784,), 2.0, dtype=torch.float64)]).cuda()
    code = torch.empty((n, Z), device="cuda")
    recon = torch.empty((n, 784), device="cuda")
    R = out["results"]
    R.append(line("encode", n, timed(lambda: h.encode(x, out=code), 1), fl["encode"], impl="hip"))
    R.append(line("encode_norm_on_load", n, timed(lambda: h.encode(x, features=feats, out=code), 1), fl["encode"], impl="hip"))
    R.append(line("decode", n, timed(lambda: h.decode(code, out=recon), 1), fl["decode"], impl="hip"))
    for rows, reps in ((512, 20), (65536, 1)):
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        xs = x[:rows]
        R.append(line("train_step", rows, timed(lambda: h.train_step(xs, p, m, v, 1, 1e-3), reps), fl["train"], impl="hip"))
    if not a.no_torch:
        try:
            ps, enc, dec = torch_model(flat, Z)
            opt = torch.optim.Adam(ps, lr=1e-3)
            with torch.no_grad():
                R.append(line("encode", n, timed(lambda: [enc(x[s:s + 65536]) for s in range(0, n, 65536)], 1), fl["encode"],
                              impl="torch_eager_fp32", chunk=65536))
                R.append(line("decode", n, timed(lambda: [dec(code[s:s + 65536]) for s in range(0, n, 65536)], 1), fl["decode"],
                              impl="torch_eager_fp32", chunk=65536))

            def step(xs):
                opt.zero_grad()
                ((dec(enc(xs)) - xs) ** 2).sum().backward()
                opt.step()
            for rows, reps in ((512, 20), (65536, 1)):
                xs = x[:rows]
                R.append(line("train_step", rows, timed(lambda: step(xs), reps), fl["train"], impl="torch_eager_fp32"))
        except Exception as e:  # noqa: BLE001 -- the yardstick is optional: say why it is missing
            out["torch_eager_error"] = f"{type(e).__name__}: {e}"
            print(json.dumps({"torch_eager_error": out["torch_eager_error"]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
