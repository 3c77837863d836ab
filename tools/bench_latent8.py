#!/usr/bin/env python3
"""Time bamd_encode / bamd_decode of 1M rows of AE(24, 15) in fp32 and bf16 mode with float32, float16 and uint8 codes.

Run:  python tools/bench_latent8.py [--out profiles/latent8_bench.json] [--repeat 3]
      BALER_AMD_LIB=/path/to/parent/libbaler_amd.so python tools/bench_latent8.py --out ...   (the yardstick: the parent build)

The parameters carry a latent scale folded in (baler_amd.latent8.fold_flat, calibrated on the min / max of the float32 latent of
the timed rows), so the uint8 codes span the byte as they do in compress; the float32 and float16 codes of the same handle are timed
on the same parameters.  Timing as tools/bench_latent16.py (tests/test_gpu_perf_floor.py::_ms): ~30 ms of the same call first, then
the MEDIAN of five event-timed samples of 20 calls; the whole measurement is repeated --repeat times in the process with the code
types ALTERNATING inside every repeat, and the spread (max - min) / min of the repeats is reported next to the median, so that a
float32-code time of one build can be compared with the run-to-run spread of the other.  A call is the whole entry point: for
uint8 codes the encode / decode kernel through the float32 workspace plus the row-conversion launch.  A library without the 8-bit
codes (the parent build) answers code 8 with BAMD_ERR_INVALID before it launches anything; its uint8 entries are recorded as null."""
import argparse
import ctypes
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
U8 = 8      # (native.U8 of this tree; spelled out so that the tool runs against either library)


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


def knows_8bit_codes(h, x):
    """Does the loaded library know BAMD_U8?  Every library since the 16-bit codes checks z_dtype before it launches or writes
    anything, so the question is a 64-row encode into a buffer that is large enough for float32 rows either way."""
    out = torch.empty((64, h.z_dim), dtype=torch.float32, device="cuda")
    rc = native.lib().bamd_encode(h._h, ctypes.c_void_p(x.data_ptr()), native.F32, 64, None, ctypes.c_void_p(out.data_ptr()), U8, h._s())
    torch.cuda.synchronize()
    return rc == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "latent8_bench.json"))
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--label", default="this tree", help="what the loaded library is, for the record (e.g. \"parent build\")")
    args = ap.parse_args()
    native.require_gpu()
    res = {"device": torch.cuda.get_device_name(0), "library": args.label, "rows": N_ROWS,
           "timing": "ms per call (whole entry point); median over --repeat alternating repeats of the median of 5 event-timed samples of 20 calls",
           "entries": []}
    g = torch.Generator(device="cuda").manual_seed(1)
    F, Z = 24, 15
    dims = orc.ae_dims(F, Z)
    layout = models.tensor_layout(dims)[0]
    codes = (torch.float32, torch.float16, torch.uint8)
    for mode in ("fp32", "bf16"):
        flat = orc.formula_params(dims, 1)
        x = torch.rand((N_ROWS, F), generator=g, device="cuda", dtype=torch.float32)
        h = native.Handle(dims, mode)
        h.load_params(torch.from_numpy(np.concatenate([flat, [0.0]]).astype(np.float32)).cuda())
        z32 = h.encode(x).double()
        lo, hi = z32.min(dim=0).values.cpu().numpy(), z32.max(dim=0).values.cpu().numpy()
        folded = latent8.fold_flat(flat, layout, lo, hi - lo)
        h.load_params(torch.from_numpy(np.concatenate([folded, [0.0]]).astype(np.float32)).cuda())
        has8 = knows_8bit_codes(h, x)
        z = {c: torch.empty((N_ROWS, Z), dtype=c, device="cuda") for c in codes}
        out = torch.empty((N_ROWS, F), dtype=torch.float32, device="cuda")
        timed = [c for c in codes if c != torch.uint8 or has8]
        for c in timed:
            h.encode(x, out=z[c])
        if has8:
            assert np.array_equal(z[torch.uint8][:4096].cpu().numpy(), latent8.q8(z[torch.float32][:4096].cpu().numpy()))
            assert mode != "fp32" or (int(z[torch.uint8].min()) == 0 and int(z[torch.uint8].max()) == 255)
        t = {c: ([], []) for c in timed}
        for _ in range(args.repeat):              # alternately: clock ramps and neighbours hit every code type alike
            for c in timed:
                t[c][0].append(_ms(lambda: h.encode(x, out=z[c]), 20))
                t[c][1].append(_ms(lambda: h.decode(z[c], out=out), 20))
        for c in codes:
            name = str(c).split(".")[-1]
            if c not in timed:
                res["entries"].append({"model": f"AE({F}, {Z})", "mode": mode, "codes": name, "encode_ms": None, "decode_ms": None,
                                       "note": "this library predates the 8-bit codes"})
                print(res["entries"][-1], flush=True)
                continue
            entry = {"model": f"AE({F}, {Z})", "mode": mode, "path": h.path, "codes": name, "latent_bytes": z[c].numel() * z[c].element_size()}
            for what, v in (("encode", t[c][0]), ("decode", t[c][1])):
                entry[what + "_ms"] = round(float(np.median(v)), 4)
                entry[what + "_repeats_ms"] = [round(u, 4) for u in v]
                entry[what + "_spread"] = round((max(v) - min(v)) / min(v), 4)
                entry[what + "_mrows_per_s"] = round(N_ROWS / float(np.median(v)) / 1e3, 1)
            res["entries"].append(entry)
            print(entry, flush=True)
        h.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
