#!/usr/bin/env python3
"""What 8-bit codes cost in reconstruction quality on the C1 workload: the trained AE(24, 15) of tests/golden/g7_c1_model_f32.npz on
synthetic CMS rows, min-max normalised.  For float32, float16 and uint8 codes: the per-column RMS of the residual decode(codes) - x
in normalised units, and the rel-L2 distance of the 16-bit / 8-bit reconstructions from the float32-code one.

    python tools/latent8_quality.py [--out profiles/latent8_quality.json] [--rows 100000]

uint8 codes as compress makes them: the extrema of the float32 latent over the rows (bamd_col_minmax), the map onto [0, 255] folded
into the last encoder and the first decoder layer (baler_amd.latent8.fold), encode to bytes and decode of the bytes on the folded
handle (fp32 mode)."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from baler_amd import latent8, native, synth  # noqa: E402
from baler_amd.modules import models  # noqa: E402
from oracle import c_oracle as orc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "latent8_quality.json"))
    ap.add_argument("--rows", type=int, default=100000)
    a = ap.parse_args()
    native.require_gpu()
    flat = np.load(os.path.join(REPO, "tests", "golden", "g7_c1_model_f32.npz"))["final_params_f32"].astype(np.float64)
    xn = orc.normalize(synth.cms_rows(a.rows))
    x = torch.from_numpy(xn).to(torch.float32).cuda()
    model = models.AE(24, 15, mode="fp32").load_flat(flat).to("cuda:0")
    h = model.handle()
    z32 = h.encode(x)
    recon = {"float32": h.decode(z32), "float16": h.decode(h.encode(x, out_dtype=torch.float16))}
    mm = native.col_minmax(z32).cpu().numpy()
    scale = np.stack([mm[0], mm[1] - mm[0]])
    model.load_flat(latent8.fold(model, scale[0], scale[1]))
    h = model.handle()
    q = h.encode(x, out_dtype=torch.uint8)
    recon["uint8"] = h.decode(q)
    step = np.abs(latent8.unscale(q.cpu().numpy(), scale[0], scale[1]) - z32.double().cpu().numpy()) / (scale[1] / 255.0)
    ref = recon["float32"].double().cpu().numpy()
    res = {"device": torch.cuda.get_device_name(0), "model": "AE(24, 15), tests/golden/g7_c1_model_f32.npz, fp32 mode", "rows": a.rows,
           "units": "min-max normalised table", "columns": [str(n) for n in synth.CMS_NAMES],
           "latent_min": scale[0].tolist(), "latent_range": scale[1].tolist(), "worst_code_error_steps": float(step.max()), "codes": {}}
    for name, r in recon.items():
        r = r.double().cpu().numpy()
        res["codes"][name] = {
            "bytes_per_row": {"float32": 60, "float16": 30, "uint8": 15}[name],
            "residual_rms_per_column": np.sqrt(((r - xn) ** 2).mean(axis=0)).tolist(),
            "residual_rms": float(np.sqrt(((r - xn) ** 2).mean())),
            "rel_l2_from_float32_codes": float(np.linalg.norm(r - ref) / np.linalg.norm(ref)),
        }
        print(name, res["codes"][name]["residual_rms"], res["codes"][name]["rel_l2_from_float32_codes"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
