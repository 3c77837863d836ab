#!/usr/bin/env python3
"""What b-bit codes cost in reconstruction quality on the C1 workload, b = 1 .. 8: the trained AE(24, 15) of
tests/golden/g7_c1_model_f32.npz on synthetic CMS rows, min-max normalised, fp32 mode.  For every width: bytes per row, the RMS of
the residual decode(codes) - x in normalised units over all columns and per column, and the rel-L2 distance of the reconstruction
from the float32-code one.

    python tools/latentb_quality.py [--out profiles/latentb_quality.json] [--rows 100000]

Codes as compress makes them: the extrema of the float32 latent over the rows (bamd_col_minmax), the map onto [0, 2**b - 1] folded
into the last encoder and the first decoder layer (baler_amd.latent8.fold), encode to packed rows and decode of the packed rows on
the folded handle.  b = 8 is the uint8 route (one byte per code) and must reproduce profiles/latent8_quality.json: that checks this
tool, not a tolerance."""
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "latentb_quality.json"))
    ap.add_argument("--rows", type=int, default=100000)
    a = ap.parse_args()
    native.require_gpu()
    flat = np.load(os.path.join(REPO, "tests", "golden", "g7_c1_model_f32.npz"))["final_params_f32"].astype(np.float64)
    xn = orc.normalize(synth.cms_rows(a.rows))
    x = torch.from_numpy(xn).to(torch.float32).cuda()
    model = models.AE(24, 15, mode="fp32").load_flat(flat).to("cuda:0")
    h = model.handle()
    z32 = h.encode(x)
    ref = h.decode(z32).double().cpu().numpy()
    mm = native.col_minmax(z32).cpu().numpy()
    scale = np.stack([mm[0], mm[1] - mm[0]])
    z64 = z32.double().cpu().numpy()

    def figures(r, bytes_per_row):
        return {"bytes_per_row": bytes_per_row,
                "residual_rms_per_column": np.sqrt(((r - xn) ** 2).mean(axis=0)).tolist(),
                "residual_rms": float(np.sqrt(((r - xn) ** 2).mean())),
                "rel_l2_from_float32_codes": float(np.linalg.norm(r - ref) / np.linalg.norm(ref))}
    res = {"device": torch.cuda.get_device_name(0), "model": "AE(24, 15), tests/golden/g7_c1_model_f32.npz, fp32 mode", "rows": a.rows,
           "units": "min-max normalised table", "columns": [str(n) for n in synth.CMS_NAMES],
           "latent_min": scale[0].tolist(), "latent_range": scale[1].tolist(), "codes": {"float32": figures(ref, 60)}}
    for bits in range(1, 9):
        levels = latent8.levels(bits)
        model.load_flat(latent8.fold_flat(flat, model.layout, scale[0], scale[1], levels).astype(np.float32))
        h = model.handle()
        if bits == 8:
            data = h.encode(x, out_dtype=torch.uint8)
            q = data.cpu().numpy()
            r = h.decode(data)
        else:
            data = h.encode(x, out_dtype=torch.uint8, code_bits=bits)
            q = latent8.unpack_rows(data.cpu().numpy(), 15, bits)
            r = h.decode(data, code_bits=bits)
        entry = figures(r.double().cpu().numpy(), int(data.shape[1]))
        entry["worst_code_error_steps"] = float((np.abs(latent8.unscale(q, scale[0], scale[1], levels) - z64) / (scale[1] / levels)).max())
        res["codes"][f"uint{bits}"] = entry
        print(f"uint{bits}", entry["bytes_per_row"], entry["residual_rms"], entry["rel_l2_from_float32_codes"], entry["worst_code_error_steps"],
              flush=True)
    with open(os.path.join(REPO, "profiles", "latent8_quality.json")) as f:
        old = json.load(f)
    if a.rows == old["rows"]:
        res["uint8_against_latent8_quality_json"] = {
            k: [res["codes"]["uint8"][k], old["codes"]["uint8"][k]] for k in ("residual_rms", "rel_l2_from_float32_codes")}
        print("uint8 here / profiles/latent8_quality.json:", res["uint8_against_latent8_quality_json"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
