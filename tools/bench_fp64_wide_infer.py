#!/usr/bin/env python3
"""fp64 encode / decode of wide tables (128 .. 4096 columns): the fused launch (fused64w.hip) against the layer-wise kernels
(BALER_AMD_F64_WIDE=0, read at bamd_create: both handles live in one process).  About 30 ms of warm-up, then the median of five
event-timed samples per call; the fraction of the 78.6 TFLOP/s fp64 matrix peak counts the model's own products only.
python tools/bench_fp64_wide_infer.py [--out profiles/f64_wide_infer.txt] [--append] [--label TEXT]
On a commit without the fused class both handles report "generic" and the two columns time the same kernels: that is the
"before" half of profiles/f64_wide_infer.txt (--label says which commit a block comes from, --append keeps the blocks already there)."""
import argparse, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np, torch
from baler_amd import native
from oracle import c_oracle as orc

PEAK = 78.6e12
SHAPES = ((625, 7), (900, 9), (2500, 25), (512, 6))
ROWS = (8192, 32768)


def ms(fn, warm_ms=30.0, samples=5, reps=3):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
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
    return sorted(got)[len(got) // 2]


def handle(dims, wide):
    if wide:
        os.environ.pop("BALER_AMD_F64_WIDE", None)
    else:
        os.environ["BALER_AMD_F64_WIDE"] = "0"
    h = native.Handle(dims, "fp64")
    os.environ.pop("BALER_AMD_F64_WIDE", None)
    h.load_params(torch.from_numpy(np.concatenate([orc.formula_params(dims, 1), [0.0]])).cuda())
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R, "profiles", "f64_wide_infer.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--label", default="this commit")
    a = ap.parse_args()
    os.environ["BALER_AMD_QUIET"] = "1"
    lines = [f"== {a.label}: fp64 encode / decode of wide tables, float64 rows, ms per call (median of 5), "
             f"fraction of the {PEAK / 1e12:.1f} TFLOP/s fp64 peak =="]
    for F, Z in SHAPES:
        dims = orc.ae_dims(F, Z)
        hf, hl = handle(dims, True), handle(dims, False)
        half = 2.0 * (F * 200 + 200 * 100 + 100 * 50 + 50 * Z)      # FLOP per row of either half of the model
        for n in ROWS:
            x = torch.rand((n, F), dtype=torch.float64, device="cuda")
            z = hf.encode(x)
            y = torch.empty_like(x)
            row = [f"AE({F}, {Z}) x {n} rows [{hf.path} | {hl.path}]:"]
            for tag, call in (("encode", lambda h: h.encode(x, out=z)), ("decode", lambda h: h.decode(z, out=y))):
                tf, tl = ms(lambda: call(hf)), ms(lambda: call(hl))
                row.append(f"{tag} {tf:.3f} ({half * n / (tf * 1e-3) / PEAK:.2f} of peak) | {tl:.3f} ({half * n / (tl * 1e-3) / PEAK:.2f}) = {tl / tf:.2f}x")
            lines.append("  ".join(row))
            print(lines[-1], flush=True)
        hf.close()
        hl.close()
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
