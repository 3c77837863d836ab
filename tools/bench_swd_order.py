#!/usr/bin/env python3
"""Times bamd_swd at the three shapes of SWAE training: (n, d, ns) = (512, 15, 2000) float32, (6000, 7, 2000) float32 (the passes
through global memory) and (4096, 7, 2000) float64 (the largest one-workgroup sort).

Run on the GPU:  python tools/bench_swd_order.py out.json           (profiles/swd_order.json was made from such runs)
Another build of the library is timed by the same command with BALER_AMD_LIB=<its libbaler_amd.so>; to compare two builds, run
them in turns (A B A B A B), one process each, and take A's run-to-run spread as the yardstick for the difference.

Per shape: the call time (all launches of the call) as tests/test_gpu_perf_floor.py times (_ms: 30 ms of the same call, then the
median of five event-timed samples of 50 calls), and a SHA-256 of the loss and dz bytes on the seeded Gaussian inputs, so that two
builds can be compared for what they compute on finite, tie-free inputs as well."""
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402

from baler_amd import native  # noqa: E402
from test_gpu_perf_floor import _ms  # noqa: E402

SHAPES = ((512, 15, 2000, torch.float32), (6000, 7, 2000, torch.float32), (4096, 7, 2000, torch.float64))


def main(out):
    native.require_gpu()
    res = []
    for n, d, ns, dtype in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(n + d)
        z = torch.randn((n, d), dtype=dtype, device="cuda", generator=g) * 0.3 + 0.1
        prior = torch.randn((n, d), dtype=dtype, device="cuda", generator=g)
        proj = torch.randn((ns, d), dtype=dtype, device="cuda", generator=g)
        proj = (proj / proj.norm(dim=1, keepdim=True)).contiguous()
        rw = 100.0 / (n * (n - 1))
        loss, dz = native.swd(z, prior, proj, rw)
        digest = hashlib.sha256(loss.cpu().numpy().tobytes() + dz.cpu().numpy().tobytes()).hexdigest()
        ms = _ms(lambda: native.swd(z, prior, proj, rw), 50)
        row = {"n": n, "d": d, "ns": ns, "dtype": str(dtype).replace("torch.", ""), "call_ms": round(ms, 4), "loss": loss.item(), "sha256": digest}
        print(row, flush=True)
        res.append(row)
    with open(out, "w") as f:
        json.dump({"lib": os.path.basename(os.path.dirname(os.path.abspath(native.LIB_PATH))), "rows": res}, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
