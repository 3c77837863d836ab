"""The re-timed role-split fp32 training pair: each layer's weight-gradient phase runs beside that layer's own dX chain (the barrier
sits between a layer's image writes and its chain), against the one-wave pair bit for bit and against the fp64 oracle.

BALER_AMD_TRAIN_ROLES (read per call): 0 = the one-wave pair, any other value = the role-split pair.  The re-timing moves barriers
and nothing else: every weight-gradient tile sums the same rows in the same order, so [grads | loss] must be torch.equal to the
one-wave pair's, and within the project's fp32 bar (rel() <= 1e-5, tests/test_gpu_parity.py) of the oracle.

Handles are created with BALER_AMD_LATENCY_ROWS=0 and BALER_AMD_TAIL_SPLIT=0, as in tests/test_gpu_train_roles.py, so that the
throughput pair runs at these sizes and a short remainder of the persistent loop stays on it.  Sizes:
  1, 17, 64, 65        partly empty waves; a full group; a second group of one row
  256 * 64 + 65        two workgroups run a second iteration: a group's last weight-gradient phase runs beside the next group's
                       forward and both image buffers are reused once
  2 * 256 * 64 + 65    a third iteration: the buffers are handed over twice before the flush"""
import functools

import numpy as np
import pytest
import torch

from baler_amd import native
from oracle import c_oracle as orc

pytestmark = pytest.mark.gpu

TOL32 = 1e-5
ONE_WAVE, ROLE_SPLIT = "0", "1"
LATENTS = [15, 12, 2]


def rel(a, b):
    """max(rel-L2, max-norm error), as in tests/test_gpu_parity.py"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    l2 = np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)
    mx = np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)
    return max(l2, mx)


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def make_handle(dims, flat):
    h = native.Handle(dims, "fp32")
    p = dev(np.concatenate([flat, [0.0]]), torch.float32)
    h.load_params(p)
    return h, p


@pytest.fixture()
def throughput_pair(monkeypatch):
    monkeypatch.setenv("BALER_AMD_LATENCY_ROWS", "0")
    monkeypatch.setenv("BALER_AMD_TAIL_SPLIT", "0")
    return monkeypatch


def run(h, p, xd, mp, roles):
    mp.setenv("BALER_AMD_TRAIN_ROLES", roles)
    g = torch.full_like(p, 3.0)
    h.fwd_bwd(xd, g)
    torch.cuda.synchronize()
    return g


@functools.lru_cache(maxsize=None)
def case(z, n):
    """(dims, parameters, rows, oracle loss, oracle gradient) of AE(24, z) on n rows, computed once per session.  The rows are
    float32-representable, so that the float64 and the float32 copy of them are the same numbers and share the reference."""
    dims = orc.ae_dims(24, z)
    flat = orc.formula_params(dims, 100 * z + n % 97)
    x = np.random.default_rng(2000 + 31 * z + n).random((n, 24)).astype(np.float32).astype(np.float64)
    lo, go = orc.fwd_bwd(dims, flat, x)
    return dims, flat, x, lo, go


def check(z, n, dtype, mp):
    dims, flat, x, lo, go = case(z, n)
    xd = dev(x, dtype)
    h, p = make_handle(dims, flat)
    assert h.path == "fused"
    old = run(h, p, xd, mp, ONE_WAVE)
    new = run(h, p, xd, mp, ROLE_SPLIT)
    gh = new.cpu().numpy().astype(np.float64)
    err, lerr = rel(gh[:-1], go), abs(gh[-1] - lo) / lo
    print(f"z={z} n={n} rel={err:.3e} loss_rel={lerr:.3e} equal={torch.equal(old, new)}")
    assert err <= TOL32 and lerr <= TOL32
    assert torch.equal(old, new)


@pytest.mark.parametrize("n", [1, 17, 64, 65])
@pytest.mark.parametrize("z", LATENTS)
def test_retimed_pair_small_groups(z, n, throughput_pair):
    check(z, n, torch.float64, throughput_pair)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64rows", "f32rows"])
@pytest.mark.parametrize("n", [256 * 64 + 65, 2 * 256 * 64 + 65], ids=["second_iteration", "third_iteration"])
@pytest.mark.parametrize("z", LATENTS)
def test_retimed_pair_later_iterations(z, n, dtype, throughput_pair):
    check(z, n, dtype, throughput_pair)


def test_retimed_pair_train_step_equals_fwd_bwd_then_adam(throughput_pair):
    """bamd_train_step == bamd_fwd_bwd + bamd_adam_step, bit for bit, on the re-timed role-split pair at n = 130."""
    throughput_pair.setenv("BALER_AMD_TRAIN_ROLES", ROLE_SPLIT)
    dims = orc.ae_dims(24, 15)
    p0 = orc.formula_params(dims, 11)
    xd = dev(np.random.default_rng(5).random((130, 24)))
    runs = []
    for fused in (False, True):
        h, flat = make_handle(dims, p0)
        m, v = torch.zeros_like(flat), torch.zeros_like(flat)
        grads = torch.zeros(h.nparams + 1, dtype=torch.float32, device="cuda")
        la = torch.zeros(1, dtype=torch.float64, device="cuda")
        for t in range(1, 4):
            if fused:
                h.train_step(xd, flat, m, v, t, 1e-3, loss_accum=la, grads=grads)
            else:
                h.fwd_bwd(xd, grads)
                h.adam_step(flat, grads, m, v, t, 1e-3, loss_accum=la)
        runs.append((flat.clone(), m.clone(), v.clone(), grads.clone(), la.item()))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b

