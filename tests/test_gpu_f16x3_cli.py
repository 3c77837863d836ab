"""The fp16x3 mode end to end on the GPU: train -> compress -> decompress of a 3,000 x 24 synthetic table through the CLI in a child
process in the fp32 mode, then compress -> decompress of the same trained model in the fp16x3 mode: the decompressed table is within
1e-5 rel-L2 of the fp32 mode's (the fp16 mode measures 6.6e-4 there) -- with float64 and with float16 latent codes.  The config has no
"int" columns, so that no truncation can turn a last-bit difference into a whole unit."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_colstats_cli import N_ROWS, REPO, _workspace

pytestmark = pytest.mark.gpu

# arguments: CLI modes, run in order; "mode=NAME" switches the compute mode of the models built from then on, "keep=TAG" copies the
# two archives written so far to <TAG>_compressed.npz / <TAG>_decompressed.npz
_WORKER = r'''
import os, shutil, sys
sys.path.insert(0, os.environ["REPO"])
import torch
from baler_amd import baler
from baler_amd.modules import helper, models
from oracle import c_oracle as orc
torch.cuda.set_device(0)
init = orc.formula_params(orc.ae_dims(24, 15), 5)
out = os.path.join("workspaces", "CMS_workspace", "CMS_project_v1", "output")

def factory(name):
    cls = getattr(models, name)
    def make(n_features, z_dim):
        return cls(n_features, z_dim).load_flat(init)
    return make
helper.model_init = factory
range_check = helper._check_fp16_mode_range
def reporting_range_check(h, *args):      # compress and decompress call it with their handle: say which kernels served them
    print("HANDLE PATH", h.path, flush=True)
    return range_check(h, *args)
helper._check_fp16_mode_range = reporting_range_check
for arg in sys.argv[1:]:
    if arg.startswith("mode="):
        models.set_default_mode(arg[5:])
    elif arg.startswith("keep="):
        for kind in ("compressed", "decompressed"):
            shutil.copy(os.path.join(out, kind + "_output", kind + ".npz"), arg[5:] + "_" + kind + ".npz")
    else:
        baler.main(["--project", "CMS_workspace", "CMS_project_v1", "--mode", arg])
'''

NO_INT = '\n    c.type_list = ["float64"] * 24\n'


def _cli(tmp_path, steps):
    script = tmp_path / "f16x3_worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, REPO=REPO)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "BALER_AMD_DIST_BACKEND", "BALER_AMD_FORCE_DEVICE", "BALER_AMD_FORCE_PG", "BALER_AMD_MODE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, str(script)] + steps, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _pair(tmp_path, tag):
    return np.load(tmp_path / f"{tag}_compressed.npz"), np.load(tmp_path / f"{tag}_decompressed.npz")


def _rel(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _compare(tmp_path, what, code_dtype):
    c32, d32 = _pair(tmp_path, "fp32")
    c3, d3 = _pair(tmp_path, "fp16x3")
    assert sorted(c3.files) == sorted(c32.files) and sorted(d3.files) == sorted(d32.files)
    assert all(c3[k].dtype == c32[k].dtype and c3[k].shape == c32[k].shape for k in c32.files)
    assert c3["data"].dtype == code_dtype and c3["data"].shape == (N_ROWS, 15) and d3["data"].shape == (N_ROWS, 24)
    e = _rel(d3["data"], d32["data"])
    ez = _rel(c3["data"], c32["data"])
    print(f"{what}: decompressed vs the fp32 mode {e:.3e}, latent codes {ez:.3e}")
    assert np.isfinite(d3["data"]).all() and e < 1e-5, what
    return e, ez


def test_cli_fp16x3_mode_decompresses_to_the_fp32_modes_table(tmp_path):
    _workspace(tmp_path, extra=NO_INT)
    out = _cli(tmp_path, ["mode=fp32", "train", "compress", "decompress", "keep=fp32", "mode=fp16x3", "compress", "decompress", "keep=fp16x3"])
    assert out.count("HANDLE PATH fused") == 2 and out.count("HANDLE PATH f16x3") == 2, out      # compress + decompress of each mode
    e, ez = _compare(tmp_path, "float64 codes", np.float64)
    assert e > 0 or ez > 0                                  # another summation order than the fp32 kernels': not a silent fp32 run
    # float16 latent codes: the same trained model, the archive's codes rounded to binary16 by both modes
    proj = tmp_path / "workspaces" / "CMS_workspace" / "CMS_project_v1"
    cfg = proj / "config" / "CMS_project_v1_config.py"
    cfg.write_text(cfg.read_text() + '\n    c.latent_dtype = "float16"\n')
    shutil.rmtree(proj / "config" / "__pycache__", ignore_errors=True)
    out = _cli(tmp_path, ["mode=fp32", "compress", "decompress", "keep=fp32", "mode=fp16x3", "compress", "decompress", "keep=fp16x3"])
    assert out.count("HANDLE PATH fused") == 2 and out.count("HANDLE PATH f16x3") == 2, out
    _compare(tmp_path, "float16 codes", np.float16)
