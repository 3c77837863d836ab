"""PJ_Conv_AE data parallel: two ranks on one GPU over gloo (BALER_AMD_FORCE_DEVICE / BALER_AMD_DIST_BACKEND, as tests/test_gpu_dp.py)
train through training.train -- row shards, the [grads | loss] sum-all-reduce between bamd_fwd_bwd and bamd_adam_step, replicated
Adam -- and end with identical parameters that equal a single-process run of the same global batches."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import free_port

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["REPO"])
import numpy as np, torch
from baler_amd import dist as bdist
from baler_amd.modules import models, training
rank, world, local = bdist.init_from_env()
if world > 1:
    torch.cuda.set_device(local)

class Cfg: pass
c = Cfg()
c.deterministic_algorithm = False; c.test_size = 0; c.batch_size = 128; c.epochs = 2; c.lr = 1e-3
c.early_stopping = False; c.lr_scheduler = True; c.lr_scheduler_patience = 50; c.reg_param = 0.001
c.data_dimension = 2; c.model_type = "convolutional"; c.activation_extraction = False; c.intermittent_model_saving = False
c.intermittent_saving_patience = 100
data = np.random.default_rng(4).random((600, 28, 28)).astype(np.float32)
out = os.environ["OUT"] + f"/rank{rank}_w{world}"
os.makedirs(out, exist_ok=True)
torch.manual_seed(11 if rank == 0 else 12)   # only rank 0 holds the intended initial weights: train() must broadcast them
model = models.PJ_Conv_AE(784, 20)
training.train(model, 28, data, data, out, c)
np.save(os.environ["OUT"] + f"/params_rank{rank}_w{world}.npy", model.flat.cpu().numpy()[:-1])
if rank == 0:      # rank 0 alone writes the artefacts
    np.save(os.environ["OUT"] + f"/loss_rank{rank}_w{world}.npy", np.load(out + "/loss_data.npy"))
bdist.barrier()
'''


def test_two_ranks_equal_single_process(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, REPO=REPO, OUT=str(tmp_path), BALER_AMD_FORCE_DEVICE="0", BALER_AMD_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), str(script)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r1 = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r1.returncode == 0, r1.stdout[-3000:] + r1.stderr[-3000:]
    p0, p1 = np.load(tmp_path / "params_rank0_w2.npy"), np.load(tmp_path / "params_rank1_w2.npy")
    np.testing.assert_array_equal(p0, p1)                       # replicated Adam on the summed gradient
    single = np.load(tmp_path / "params_rank0_w1.npy").astype(np.float64)
    # the shards' float32 gradients are summed after rounding: equal to the single process to float32 rounding
    assert np.linalg.norm(p0 - single) / np.linalg.norm(single) < 1e-5
    l2, l1 = np.load(tmp_path / "loss_rank0_w2.npy"), np.load(tmp_path / "loss_rank0_w1.npy")
    assert np.all(np.abs(l2 / l1 - 1) < 1e-5)
