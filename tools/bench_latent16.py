#!/usr/bin/env python3
"""Time bamd_encode / bamd_decode of 1M rows with float32 codes and with 16-bit codes: the 24-column AE in fp32 and bf16 mode and a
run-time-width class shape, AE(40, 10), in fp32 mode.

Run:  python tools/bench_latent16.py [--out profiles/latent16_bench.json] [--repeat 3]
      BALER_AMD_LIB=/path/to/parent/libbaler_amd.so python tools/bench_latent16.py --out ...   (the yardstick: the parent build)

Timing as tests/test_gpu_perf_floor.py::_ms: ~30 ms of the same call first, then the MEDIAN of five event-timed samples; the whole
measurement is repeated --repeat times in the process, and the spread (max - min) / min of those repeats is reported next to the
median, so that a float32-code time of one build can be compared with the run-to-run spread of the other.  A library without the
16-bit codes (the parent build) is detected with a call that is safe on either build; its 16-bit entries are recorded as null."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from baler_amd import native  # noqa: E402
from oracle import c_oracle as orc  # noqa: E402

N_ROWS = 1_000_000


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


def knows_16bit_codes(h, z32):
    """Does the loaded library know BAMD_F16 / BAMD_BF16?  Asked with a call that is safe either way: out_dtype = BAMD_F16 of a
    decode into a buffer large enough for float32 rows.  A library with the codes refuses it before it writes anything; one from
    before them reads every dtype other than BAMD_F64 as float32 (and would overrun a 2-byte latent buffer if it were handed one)."""
    import ctypes
    n = 64
    out = torch.empty((n, h.dims[-1]), dtype=torch.float32, device="cuda")
    rc = native.lib().bamd_decode(h._h, ctypes.c_void_p(z32.data_ptr()), native.F32, n, None, None, ctypes.c_void_p(out.data_ptr()),
                                  native.F16, h._s())
    torch.cuda.synchronize()
    return rc == -1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "latent16_bench.json"))
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    native.require_gpu()
    res = {"device": torch.cuda.get_device_name(0), "library": native.LIB_PATH, "rows": N_ROWS, "entries": []}
    g = torch.Generator(device="cuda").manual_seed(1)
    # AE(24, 15): the exact instantiation (fp32 register chain, bf16.hip); AE(40, 10): a run-time-width class of the register chain
    for F, Z, mode in ((24, 15, "fp32"), (24, 15, "bf16"), (40, 10, "fp32")):
        dims = orc.ae_dims(F, Z)
        flat = orc.formula_params(dims, 1)
        x = torch.rand((N_ROWS, F), generator=g, device="cuda", dtype=torch.float32)
        h = native.Handle(dims, mode)
        h.load_params(torch.from_numpy(np.concatenate([flat, [0.0]]).astype(np.float32)).cuda())
        z32 = h.encode(x)
        has_codes = knows_16bit_codes(h, z32)
        for code in (torch.float32, torch.float16, torch.bfloat16):
            name = str(code).split(".")[-1]
            z = torch.empty((N_ROWS, Z), dtype=code, device="cuda")
            out = torch.empty((N_ROWS, F), dtype=torch.float32, device="cuda")
            if code != torch.float32 and not has_codes:
                res["entries"].append({"model": f"AE({F}, {Z})", "mode": mode, "codes": name, "encode_ms": None, "decode_ms": None,
                                       "note": "this library predates the 16-bit codes"})
                print(res["entries"][-1], flush=True)
                continue
            h.encode(x, out=z)
            assert torch.equal(z, z32.to(code))
            enc = [_ms(lambda: h.encode(x, out=z), 20) for _ in range(args.repeat)]
            dec = [_ms(lambda: h.decode(z, out=out), 20) for _ in range(args.repeat)]
            entry = {"model": f"AE({F}, {Z})", "mode": mode, "codes": name, "latent_bytes": z.numel() * z.element_size()}
            for what, t in (("encode", enc), ("decode", dec)):
                entry[what + "_ms"] = round(float(np.median(t)), 4)
                entry[what + "_repeats_ms"] = [round(v, 4) for v in t]
                entry[what + "_spread"] = round((max(t) - min(t)) / min(t), 4)
                entry[what + "_mrows_per_s"] = round(N_ROWS / float(np.median(t)) / 1e3, 1)
            res["entries"].append(entry)
            print(entry, flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
