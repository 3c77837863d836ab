"""A/B run of the fp32 training pair's schedules in ONE process: bamd_fwd_bwd on AE(24, 15), 1,000,000 resident float64 rows, 300
warm-up calls, then 12 interleaved rounds, each the mean of 5 calls between two HIP events (the method of
profiles/r7_f32_train_roles_ab.txt).

    python tools/train_roles_ab.py [ROLES ...]      values of BALER_AMD_TRAIN_ROLES to interleave (default: 0 1)

Prints the per-round table, median / min / max / spread per value, the gain of every value against the first one and three times
the larger of the two spreads (the bar a gain has to clear), and whether [grads | loss] at 1M rows is bit-identical across values."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from baler_amd import native, synth                               # noqa: E402
from baler_amd.modules import models                              # noqa: E402

ROUNDS, CALLS, WARM = 12, 5, 300


def main():
    vals = sys.argv[1:] or ["0", "1"]
    dev = torch.device("cuda", 0)
    n = 1_000_000
    raw = torch.as_tensor(synth.cms_rows(n)).to(dev)
    x = native.normalize(raw, native.minmax(raw), torch.float64)
    torch.manual_seed(0)
    model = models.AE(24, 15, mode="fp32").to(dev)
    h = model.handle()
    grads = torch.zeros_like(model.flat)

    def call(v):
        os.environ["BALER_AMD_TRAIN_ROLES"] = v
        h.fwd_bwd(x, grads)

    outs = []
    for v in vals:
        call(v)
        torch.cuda.synchronize()
        outs.append(grads.clone())
    same = all(torch.equal(outs[0], o) for o in outs[1:])
    for i in range(WARM):
        call(vals[i % len(vals)])
    torch.cuda.synchronize()
    ms = {v: [] for v in vals}
    for _ in range(ROUNDS):
        for v in vals:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                call(v)
            e1.record()
            e1.synchronize()
            ms[v].append(e0.elapsed_time(e1) / CALLS)
    print(f"bamd_fwd_bwd on AE(24,15), {n:,} resident float64 rows; {WARM} warm-up calls, then {ROUNDS} interleaved rounds, "
          f"each the mean of {CALLS} calls (HIP events).")
    print(f"[grads | loss] at 1M rows across BALER_AMD_TRAIN_ROLES = {', '.join(vals)}: {'bit-identical' if same else 'DIFFERENT'}\n")
    print("round " + "".join(f"{'ROLES=' + v + ' ms':>16s}" for v in vals))
    for r in range(ROUNDS):
        print(f"{r:5d} " + "".join(f"{ms[v][r]:16.4f}" for v in vals))
    print()
    med = {v: float(np.median(ms[v])) for v in vals}
    spread = {v: max(ms[v]) - min(ms[v]) for v in vals}
    for v in vals:
        print(f"ROLES={v}  median {med[v]:.4f}  min {min(ms[v]):.4f}  max {max(ms[v]):.4f}  (spread {spread[v]:.4f} ms)")
    for v in vals[1:]:
        bar = 3 * max(spread[vals[0]], spread[v])
        gain = med[vals[0]] - med[v]
        print(f"ROLES={v} against ROLES={vals[0]}: gain of the medians {gain:+.4f} ms = {100 * gain / med[vals[0]]:+.2f} %; "
              f"three times the larger spread = {bar:.4f} ms: {'clears the bar' if gain > bar else 'does NOT clear the bar'}")


if __name__ == "__main__":
    main()
