#!/usr/bin/env python3
"""What 16-bit latent codes cost in reconstruction quality on the C1 workload (the 24-column CMS table, fixture g7's trained model).

Run:  python tools/latent16_quality.py [--rows 1000000] [--out profiles/latent16_quality.json]

The table is normalised and encoded once (fp32 handle); the float32 codes, their float16 and their bfloat16 roundings (made by
bamd_encode itself) are decoded with the un-normalise / int-truncation epilogue, as decompress does.  Per column: the RMS of the
residual decompressed - input for the three code types, and the RMS of the difference between the 16-bit-code and the float32-code
decompression.  A report, not a test: there is no derivable bound through the decoder."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from baler_amd import native, synth  # noqa: E402
from oracle import c_oracle as orc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "latent16_quality.json"))
    args = ap.parse_args()
    native.require_gpu()
    flat = np.load(os.path.join(REPO, "tests", "golden", "g7_c1_model_f32.npz"))["final_params_f32"].astype(np.float32)
    dims = orc.ae_dims(24, 15)
    h = native.Handle(dims, "fp32")
    h.load_params(torch.from_numpy(np.concatenate([flat, np.zeros(1, np.float32)])).cuda())
    raw = torch.from_numpy(synth.cms_rows(args.rows)).cuda()
    feats = native.minmax(raw)
    mask = torch.as_tensor(np.array([t == "int" for t in synth.CMS_TYPE_LIST], dtype=np.uint8)).cuda()
    dec = {}
    for name, dt in (("float32", torch.float32), ("float16", torch.float16), ("bfloat16", torch.bfloat16)):
        z = h.encode(raw, features=feats, out_dtype=dt)
        assert bool(torch.isfinite(z.float()).all())
        dec[name] = h.decode(z, features=feats, int_mask=mask, out_dtype=torch.float64)

    def rms(t):
        return [float(v) for v in torch.sqrt(torch.mean(t * t, dim=0)).cpu().numpy()]

    res = {"device": torch.cuda.get_device_name(0), "rows": args.rows, "model": "AE(24, 15), tests/golden/g7_c1_model_f32.npz",
           "columns": [str(n).split(".")[-1] for n in synth.CMS_NAMES],
           "value_range": [float(v) for v in feats[1].cpu().numpy()]}
    for name in dec:
        res["residual_rms_" + name] = rms(dec[name] - raw)
    for name in ("float16", "bfloat16"):
        res["rms_vs_float32_codes_" + name] = rms(dec[name] - dec["float32"])
    for k, name in enumerate(res["columns"]):
        print(f"{name:28s} residual RMS f32 {res['residual_rms_float32'][k]:.6g}  f16 {res['residual_rms_float16'][k]:.6g}  "
              f"bf16 {res['residual_rms_bfloat16'][k]:.6g}   vs f32 codes: f16 {res['rms_vs_float32_codes_float16'][k]:.3g}  "
              f"bf16 {res['rms_vs_float32_codes_bfloat16'][k]:.3g}", flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
