"""BALER_AMD_MODE=fp16 end to end on the GPU: train -> compress -> decompress of a 3,000 x 24 synthetic table through the CLI in a
child process, beside the same run in the fp32 and the bf16 mode: the artefacts have the fp32 run's keys and dtypes, training is the
fp32 run's bit for bit, the decompressed table is at least 4 x closer to the fp32 run's than the bf16 mode's is (half of the 2^3
that three more significand bits give) -- with float64 and with float16 latent codes -- and a row that leaves the float16 range
inside the model stops compress before an archive is written."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_colstats_cli import N_ROWS, REPO, _workspace

pytestmark = pytest.mark.gpu

# the worker of tests/test_gpu_colstats_cli.py without its set_default_mode("fp64"): the compute mode comes from BALER_AMD_MODE
_WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["REPO"])
import torch
from baler_amd import baler
from baler_amd.modules import helper, models
from oracle import c_oracle as orc
torch.cuda.set_device(0)
init = orc.formula_params(orc.ae_dims(24, 15), 5)

def factory(name):
    cls = getattr(models, name)
    def make(n_features, z_dim):
        return cls(n_features, z_dim).load_flat(init)
    return make
helper.model_init = factory
for mode in sys.argv[1:]:
    baler.main(["--project", "CMS_workspace", "CMS_project_v1", "--mode", mode])
'''


def _cli(tmp_path, mode, steps, check=True):
    script = tmp_path / "f16_worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, REPO=REPO, BALER_AMD_MODE=mode)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "BALER_AMD_DIST_BACKEND", "BALER_AMD_FORCE_DEVICE", "BALER_AMD_FORCE_PG"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, str(script)] + steps, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    if check:
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _set_config(tmp_path, extra):
    proj = tmp_path / "workspaces" / "CMS_workspace" / "CMS_project_v1"
    src = open(os.path.join(REPO, "workspaces", "CMS_workspace", "CMS_project_v1", "config", "CMS_project_v1_config.py")).read()
    (proj / "config" / "CMS_project_v1_config.py").write_text(src.replace("c.epochs = 25", "c.epochs = 3") + extra)


def _artefacts(out):
    comp, dec = np.load(out / "compressed_output" / "compressed.npz"), np.load(out / "decompressed_output" / "decompressed.npz")
    return ({k: (comp[k].dtype, comp[k].shape) for k in comp.files}, {k: (dec[k].dtype, dec[k].shape) for k in dec.files},
            dec["data"].astype(np.float64))


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_cli_fp16_mode_beside_fp32_and_bf16(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    out_a, out_b = _workspace(a), _workspace(b)
    _cli(a, "fp32", ["train", "compress", "decompress"])
    _cli(b, "fp16", ["train", "compress", "decompress"])
    loss_a, loss_b = np.load(out_a / "training" / "loss_data.npy"), np.load(out_b / "training" / "loss_data.npy")
    assert loss_a.dtype == loss_b.dtype and loss_a.tobytes() == loss_b.tobytes()          # training is fp32 in both
    sd_a, sd_b = (torch.load(str(o / "compressed_output" / "model.pt"), map_location="cpu") for o in (out_a, out_b))
    assert list(sd_a) == list(sd_b) and all(sd_a[k].dtype == sd_b[k].dtype and torch.equal(sd_a[k], sd_b[k]) for k in sd_a)
    for tag, extra in (("float64 codes", ""), ("float16 codes", '\n    c.latent_dtype = "float16"\n')):
        if extra:
            _set_config(a, extra)
            _set_config(b, extra)
            _cli(a, "fp32", ["compress", "decompress"])
            _cli(b, "fp16", ["compress", "decompress"])
        comp32, dec32, data32 = _artefacts(out_a)
        comp16, dec16, data16 = _artefacts(out_b)
        assert comp16 == comp32 and dec16 == dec32, tag                                    # keys, dtypes and shapes
        assert comp32["data"] == (np.dtype(np.float16 if extra else np.float64), (N_ROWS, 15))
        _cli(a, "bf16", ["compress", "decompress"])                                        # the same trained model, bf16 inference
        compb, decb, datab = _artefacts(out_a)
        assert compb == comp32 and decb == dec32
        e16, eb = _rel(data16, data32), _rel(datab, data32)
        print(f"{tag}: decompressed vs the fp32 mode: fp16 {e16:.3e}  bf16 {eb:.3e}  (1/{eb / e16:.1f})")
        assert np.isfinite(data16).all() and 0 < e16 <= eb / 4, tag


def test_cli_fp16_mode_refuses_rows_that_leave_the_float16_range(tmp_path):
    from baler_amd import synth
    from oracle import c_oracle as orc
    out = _workspace(tmp_path, extra="\n    c.apply_normalization = False\n")
    data_path = tmp_path / "workspaces" / "CMS_workspace" / "data" / "example_CMS_data.npz"
    table = orc.normalize(synth.cms_rows(N_ROWS))                # rows in [0, 1]: what the model expects without normalisation
    np.savez(data_path, data=table, names=synth.CMS_NAMES)
    _cli(tmp_path, "fp16", ["train", "compress"])
    comp = out / "compressed_output" / "compressed.npz"
    assert comp.exists() and np.isfinite(np.load(comp)["data"]).all()
    os.remove(comp)
    table[1234, 7] = 1e6                                         # binary16(1e6) = inf as a layer input, whatever the weights are
    np.savez(data_path, data=table, names=synth.CMS_NAMES)
    r = _cli(tmp_path, "fp16", ["compress"], check=False)
    assert r.returncode != 0
    assert "ValueError" in r.stderr and "1 rows" in r.stderr and "bf16" in r.stderr and "fp32" in r.stderr, r.stderr[-2000:]
    assert not comp.exists()
    _cli(tmp_path, "bf16", ["compress"])                         # the mode the message names takes the same table
    assert comp.exists()
