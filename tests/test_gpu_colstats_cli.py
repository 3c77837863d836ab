"""--mode report end to end on the GPU: train -> compress -> decompress -> report on a small synthetic 1-D workspace; the written
column_stats.npz equals numpy applied to the input and to the written decompressed.npz; two ranks on one GPU (gloo) agree with
one process."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import free_port

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-11
N_ROWS = 3000

_WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["REPO"])
import torch
from baler_amd import baler, dist as bdist
from baler_amd.modules import helper, models
from oracle import c_oracle as orc
rank, world, local = bdist.init_from_env()
torch.cuda.set_device(local)
models.set_default_mode("fp64")
init = orc.formula_params(orc.ae_dims(24, 15), 5)

def factory(name):
    cls = getattr(models, name)
    def make(n_features, z_dim):
        m = cls(n_features, z_dim)
        return m.load_flat(init) if rank == 0 else m
    return make
helper.model_init = factory
for mode in sys.argv[1:]:
    baler.main(["--project", "CMS_workspace", "CMS_project_v1", "--mode", mode])
bdist.barrier()
'''


def _workspace(tmp_path, extra=""):
    from baler_amd import synth
    ws = tmp_path / "workspaces"
    proj = ws / "CMS_workspace" / "CMS_project_v1"
    for d in ("config", "output/compressed_output", "output/decompressed_output", "output/plotting", "output/training"):
        os.makedirs(proj / d, exist_ok=True)
    os.makedirs(ws / "CMS_workspace" / "data", exist_ok=True)
    (ws / "__init__.py").write_text("")
    src = open(os.path.join(REPO, "workspaces", "CMS_workspace", "CMS_project_v1", "config", "CMS_project_v1_config.py")).read()
    assert "c.epochs = 25" in src
    (proj / "config" / "CMS_project_v1_config.py").write_text(src.replace("c.epochs = 25", "c.epochs = 3") + extra)
    np.savez(ws / "CMS_workspace" / "data" / "example_CMS_data.npz", data=synth.cms_rows(N_ROWS), names=synth.CMS_NAMES)
    return proj / "output"


def _run(tmp_path, modes, ranks):
    script = tmp_path / "report_worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, REPO=REPO)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "BALER_AMD_DIST_BACKEND", "BALER_AMD_FORCE_DEVICE", "BALER_AMD_FORCE_PG"):
        env.pop(k, None)
    if ranks == 1:
        cmd = [sys.executable, str(script)] + modes
    else:
        env.update(BALER_AMD_FORCE_DEVICE="0", BALER_AMD_DIST_BACKEND="gloo")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}", "--master-addr", "127.0.0.1",
               "--master-port", str(free_port()), str(script)] + modes
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _numpy_report(before, after, cut):
    keep = ~(before[:, cut[0]] < cut[1])
    b, a = before[keep], after[keep]
    with np.errstate(all="ignore"):
        resid, resp = np.subtract(a, b), np.divide(np.subtract(a, b), b) * 100
        s = b + a
        e_val = np.stack([np.linspace(s[:, k].min() - 0.1 * abs(s[:, k].max() - s[:, k].min()),
                                      s[:, k].max() + 0.1 * abs(s[:, k].max() - s[:, k].min()), 200) for k in range(b.shape[1])])
    return keep, b, a, resid, resp, e_val


def _close(got, want, scale, what):
    fin = np.isfinite(want) & np.isfinite(scale)
    np.testing.assert_array_equal(got[~fin], want[~fin], err_msg=what)
    err = np.abs(got[fin] - want[fin]) / np.maximum(scale[fin], 1e-300)
    print(f"{what}: worst error {err.max() if err.size else 0:.3e}")
    assert (np.abs(got[fin] - want[fin]) <= TOL * scale[fin]).all(), what


@pytest.mark.parametrize("chunk_rows", [None, 700], ids=["one-chunk", "chunks-of-700"])
def test_cli_report_equals_numpy_and_two_ranks_agree(tmp_path, chunk_rows):
    from baler_amd import synth
    out = _workspace(tmp_path, extra=f"\n    c.report_chunk_rows = {chunk_rows}\n" if chunk_rows else "")
    stdout = _run(tmp_path, ["train", "compress", "decompress", "report"], 1)
    assert "=== Column report ===" in stdout and stdout.count("residual mean") == 24
    before = synth.cms_rows(N_ROWS)
    after = np.load(out / "decompressed_output" / "decompressed.npz")["data"]
    assert after.shape == before.shape == (N_ROWS, 24)
    g = dict(np.load(out / "plotting" / "column_stats.npz"))
    assert list(g["names"]) == list(synth.CMS_NAMES) and tuple(g["cut"]) == (3.0, 1e-6)

    keep, b, a, resid, resp, e_val = _numpy_report(before, after, (3, 1e-6))
    np.testing.assert_array_equal(g["count"], np.full(24, keep.sum()))
    np.testing.assert_array_equal(g["edges_response"], np.arange(-20, 20, 0.1))
    np.testing.assert_array_equal(g["edges_residual"], np.arange(-1, 1, 0.01))
    np.testing.assert_array_equal(g["edges_value"], e_val)
    for k in range(24):
        np.testing.assert_array_equal(g["counts_response"][k], np.histogram(resp[:, k], bins=g["edges_response"])[0])
        np.testing.assert_array_equal(g["counts_residual"][k], np.histogram(resid[:, k], bins=g["edges_residual"])[0])
        np.testing.assert_array_equal(g["counts_before"][k], np.histogram(b[:, k], bins=e_val[k])[0])
        np.testing.assert_array_equal(g["counts_after"][k], np.histogram(a[:, k], bins=e_val[k])[0])
    with np.errstate(all="ignore"):
        for name, v in (("resid", resid), ("before", b), ("after", a), ("sum", b + a)):
            np.testing.assert_array_equal(g[name + "_min"], np.fmin.reduce(v, axis=0))
            np.testing.assert_array_equal(g[name + "_max"], np.fmax.reduce(v, axis=0))
        _close(g["resid_mean"], resid.mean(axis=0), np.abs(resid).mean(axis=0), "resid_mean")
        _close(g["resp_mean"], resp.mean(axis=0), np.abs(resp).mean(axis=0), "resp_mean")
        rms_d, rms_p = np.sqrt(np.mean(np.square(resid), axis=0)), np.sqrt(np.mean(np.square(resp), axis=0))
        _close(g["resid_rms"], rms_d, rms_d, "resid_rms")
        _close(g["resp_rms"], rms_p, rms_p, "resp_rms")

    # two ranks on one GPU: each reduces its row slice, the results are all-reduced, rank 0 writes
    os.rename(out / "plotting" / "column_stats.npz", out / "plotting" / "one_process.npz")
    _run(tmp_path, ["report"], 2)
    h = dict(np.load(out / "plotting" / "column_stats.npz"))
    with np.errstate(all="ignore"):
        for key in g:
            if key in ("resid_mean", "resp_mean"):
                _close(h[key], g[key], np.abs(resid if key == "resid_mean" else resp).mean(axis=0), "2 ranks " + key)
            elif key in ("resid_rms", "resp_rms"):
                _close(h[key], g[key], g[key], "2 ranks " + key)
            else:
                np.testing.assert_array_equal(h[key], g[key], err_msg="2 ranks " + key)
