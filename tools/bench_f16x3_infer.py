"""fp16x3 inference mode beside fp32 and bf16: encode / decode of 1M rows (float64 and float32 rows), the three handles timed
alternately in one process with the timing method of tests/test_gpu_perf_floor.py (_ms: warm for 30 ms, median of 5 samples of 5
calls), and the three modes' errors against the fp64 oracle on the trained C1 fixture (rel-L2, and the ratio to the fp32 handle's).

    python tools/bench_f16x3_infer.py [--out profiles/f16x3_infer_bench.json]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np      # noqa: E402
import torch            # noqa: E402

from baler_amd import native, synth      # noqa: E402
from oracle import c_oracle as orc       # noqa: E402

N = 1_000_000


def _ms(fn, reps=5, warm_ms=30.0, samples=5):
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
    return sorted(got)[len(got) // 2]


def handle(dims, flat, mode):
    h = native.Handle(dims, mode)
    h.load_params(torch.from_numpy(np.concatenate([flat, [0.0]]).astype(np.float32)).cuda())
    return h


def rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b))


def measure(modes, rounds=3):
    dims = orc.ae_dims(24, 15)
    flat = np.load(os.path.join(REPO, "tests", "golden", "g7_c1_model_f32.npz"))["final_params_f32"].astype(np.float64)
    hs = {m: handle(dims, flat, m) for m in modes}
    res = {m: {"path": hs[m].path} for m in modes}
    # errors against the oracle on the fixture's own kind of data
    xn = orc.normalize(synth.cms_rows(10000))
    zo = orc.encode(dims, flat, xn)
    ro = orc.decode(dims, flat, zo)
    for m, h in hs.items():
        x, z = torch.from_numpy(xn).cuda(), torch.from_numpy(zo).cuda()
        res[m]["rel_l2_encode"] = rel_l2(h.encode(x).cpu().numpy(), zo)
        res[m]["rel_l2_decode"] = rel_l2(h.decode(z).cpu().numpy(), ro)
        res[m]["rel_l2_forward"] = rel_l2(h.forward_loss(x)[0].cpu().numpy(), ro)
    for dt, name in ((torch.float64, "float64"), (torch.float32, "float32")):
        x = torch.rand((N, 24), dtype=dt, device="cuda")
        z = hs[modes[0]].encode(x)
        zout, dout = torch.empty_like(z), torch.empty_like(x)
        t = {m: ([], []) for m in modes}
        for _ in range(rounds):                  # alternately: clock ramps hit every mode alike
            for m in modes:
                t[m][0].append(_ms(lambda: hs[m].encode(x, out=zout)))
                t[m][1].append(_ms(lambda: hs[m].decode(z, out=dout)))
        for m in modes:
            res[m][f"encode_ms_1M_{name}_rows"] = sorted(t[m][0])[rounds // 2]
            res[m][f"decode_ms_1M_{name}_rows"] = sorted(t[m][1])[rounds // 2]
            res[m][f"encode_ms_1M_{name}_rows_all"] = t[m][0]
            res[m][f"decode_ms_1M_{name}_rows_all"] = t[m][1]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "f16x3_infer_bench.json"))
    a = ap.parse_args()
    native.require_gpu()
    modes = measure(["fp32", "bf16", "fp16x3"])
    for what in ("encode", "decode", "forward"):
        modes["fp16x3"][f"error_ratio_to_fp32_{what}"] = modes["fp16x3"][f"rel_l2_{what}"] / modes["fp32"][f"rel_l2_{what}"]
    for k in [k for k in modes["fp32"] if k.endswith("_rows")]:
        modes["fp16x3"]["speedup_over_fp32_" + k[:-5].replace("_ms_1M", "")] = modes["fp32"][k] / modes["fp16x3"][k]
    res = {"device": torch.cuda.get_device_name(0), "rows": N, "model": "AE(24, 15), tests/golden/g7_c1_model_f32.npz",
           "timing": "median of 3 alternating rounds of _ms (tests/test_gpu_perf_floor.py): median of 5 samples of 5 calls, ms per call; "
                     "*_all: the three rounds (their spread is the run-to-run variation)",
           "modes": modes}
    for m, v in res["modes"].items():
        print(m, {k: (round(x, 6) if isinstance(x, float) else x) for k, x in v.items() if not k.endswith("_all")})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
