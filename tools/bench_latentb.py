#!/usr/bin/env python3
"""Time bamd_encode / bamd_decode of 1M rows of AE(24, 15) in fp32 and bf16 mode with float32, uint8, packed 5-bit and packed 1-bit
codes.

Run:  python tools/bench_latentb.py [--out profiles/latentb_bench.json] [--repeat 3]

The yardstick is the uint8 route of the same library in the same session: the packed route reads the same float32 workspace and
writes fewer bytes.  uint8 is therefore timed TWICE inside every repeat ("uint8" and "uint8 again"); the difference between those
two medians is the margin a packed time is held against.  Every code type runs on parameters folded for its own number of levels
(baler_amd.latent8.fold_flat on the min / max of the float32 latent of the timed rows), so the codes span their range as they do in
compress; float32 codes run on the 8-bit fold.  Timing as tools/bench_latent8.py: ~30 ms of the same call first, then the MEDIAN of
five event-timed samples of 20 calls; the whole measurement is repeated --repeat times with the code types ALTERNATING inside every
repeat.  A call is the whole entry point: the encode / decode kernel through the float32 workspace plus the row-conversion launch."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from baler_amd import latent8, native  # noqa: E402
from baler_amd.modules import models  # noqa: E402
from oracle import c_oracle as orc  # noqa: E402

N_ROWS = 1_000_000
# name -> (torch dtype of the buffer, code_bits or None, bits the parameters are folded for)
CODES = {"float32": (torch.float32, None, 8), "uint8": (torch.uint8, None, 8), "uint5": (torch.uint8, 5, 5), "uint1": (torch.uint8, 1, 1),
         "uint8 again": (torch.uint8, None, 8)}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "latentb_bench.json"))
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    native.require_gpu()
    res = {"device": torch.cuda.get_device_name(0), "rows": N_ROWS,
           "timing": "ms per call (whole entry point); median over --repeat alternating repeats of the median of 5 event-timed samples of 20 calls",
           "entries": []}
    g = torch.Generator(device="cuda").manual_seed(1)
    F, Z = 24, 15
    dims = orc.ae_dims(F, Z)
    layout = models.tensor_layout(dims)[0]
    for mode in ("fp32", "bf16"):
        flat = orc.formula_params(dims, 1)
        x = torch.rand((N_ROWS, F), generator=g, device="cuda", dtype=torch.float32)
        h = native.Handle(dims, mode)
        h.load_params(torch.from_numpy(np.concatenate([flat, [0.0]]).astype(np.float32)).cuda())
        z32 = h.encode(x).double()
        lo, hi = z32.min(dim=0).values.cpu().numpy(), z32.max(dim=0).values.cpu().numpy()
        params = {b: torch.from_numpy(np.concatenate([latent8.fold_flat(flat, layout, lo, hi - lo, latent8.levels(b)), [0.0]]).astype(np.float32)).cuda()
                  for b in (8, 5, 1)}
        z = {name: torch.empty((N_ROWS, Z if cb is None else native.packed_row_bytes(Z, cb)), dtype=dt, device="cuda")
             for name, (dt, cb, _) in CODES.items()}
        out = torch.empty((N_ROWS, F), dtype=torch.float32, device="cuda")
        for name, (dt, cb, fb) in CODES.items():      # fill every buffer with its codes and check the packed ones against NumPy
            h.load_params(params[fb])
            h.encode(x, out=z[name], code_bits=cb)
            if cb is not None:
                z32f = h.encode(x[:4096], out_dtype=torch.float32).cpu().numpy()
                assert np.array_equal(z[name][:4096].cpu().numpy(), latent8.pack_rows(latent8.qb(z32f, cb), cb))
        t = {name: ([], []) for name in CODES}
        for _ in range(args.repeat):              # alternately: clock ramps and neighbours hit every code type alike
            for name, (dt, cb, fb) in CODES.items():
                h.load_params(params[fb])
                t[name][0].append(_ms(lambda: h.encode(x, out=z[name], code_bits=cb), 20))
                t[name][1].append(_ms(lambda: h.decode(z[name], out=out, code_bits=cb), 20))
        for name in CODES:
            entry = {"model": f"AE({F}, {Z})", "mode": mode, "path": h.path, "codes": name, "latent_bytes": z[name].numel() * z[name].element_size()}
            for what, v in (("encode", t[name][0]), ("decode", t[name][1])):
                entry[what + "_ms"] = round(float(np.median(v)), 4)
                entry[what + "_repeats_ms"] = [round(u, 4) for u in v]
                entry[what + "_spread"] = round((max(v) - min(v)) / min(v), 4)
            res["entries"].append(entry)
            print(entry, flush=True)
        by = {e["codes"]: e for e in res["entries"] if e["mode"] == mode}
        margin = {w: round(abs(by["uint8"][w + "_ms"] - by["uint8 again"][w + "_ms"]), 4) for w in ("encode", "decode")}
        res.setdefault("uint8_margin_ms", {})[mode] = margin
        for name in ("uint5", "uint1"):
            for w in ("encode", "decode"):
                by[name][w + "_minus_uint8_ms"] = round(by[name][w + "_ms"] - min(by["uint8"][w + "_ms"], by["uint8 again"][w + "_ms"]), 4)
        print(mode, "margin between the two uint8 measurements:", margin, flush=True)
        h.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
