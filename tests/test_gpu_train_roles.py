"""The role-split fp32 training pair (train_dec_roles_kernel / train_enc_roles_kernel: chain waves + weight-gradient waves, two
waves per SIMD) against the fp64 oracle and, bit for bit, against the one-wave pair it stands beside.

BALER_AMD_TRAIN_ROLES (read per call) picks the pair: 1 = role-split, 0 = one wave per SIMD.  Every handle here is created with
BALER_AMD_LATENCY_ROWS=0, so that the throughput pair runs at these small sizes, and BALER_AMD_TAIL_SPLIT=0, so that a short
remainder of the persistent loop stays on the pair: 256 * 64 + 65 rows are 258 row groups on 256 workgroups, two of which then run
a second iteration (image-buffer reuse and the overlap of a group's last weight-gradient phase with the next group's forward).

Bar: the project's fp32 one, rel() <= 1e-5 against the oracle (tests/test_gpu_parity.py); old pair vs new pair: torch.equal on the
whole [grads | loss] buffer -- the same products summed in the same order."""
import numpy as np
import pytest
import torch

from baler_amd import native
from oracle import c_oracle as orc

pytestmark = pytest.mark.gpu

TOL32 = 1e-5


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


def both_pairs(h, p, xd, mp):
    out = []
    for roles in ("0", "1"):
        mp.setenv("BALER_AMD_TRAIN_ROLES", roles)
        g = torch.full_like(p, 3.0)
        h.fwd_bwd(xd, g)
        out.append(g)
    torch.cuda.synchronize()
    return out


def check(dims, flat, x, xd, mp):
    h, p = make_handle(dims, flat)
    assert h.path == "fused"
    old, new = both_pairs(h, p, xd, mp)
    lo, go = orc.fwd_bwd(dims, flat, x)
    gh = new.cpu().numpy().astype(np.float64)
    err, lerr = rel(gh[:-1], go), abs(gh[-1] - lo) / lo
    print(f"n={x.shape[0]} dims0={dims[0]} rel={err:.3e} loss_rel={lerr:.3e} equal={torch.equal(old, new)}")
    assert err <= TOL32 and lerr <= TOL32
    assert torch.equal(old, new)


@pytest.mark.parametrize("n", [1, 17, 63, 64, 65])
def test_roles_pair_small_groups(n, throughput_pair):
    """One row group with partly empty waves (invalid rows zeroed), a full one, and a second group of a single row."""
    dims = orc.ae_dims(24, 15)
    flat = orc.formula_params(dims, 41)
    x = np.random.default_rng(1000 + n).random((n, 24))
    check(dims, flat, x, dev(x), throughput_pair)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_roles_pair_second_iteration(dtype, throughput_pair):
    """256 * 64 + 65 rows: two workgroups run a second iteration; float64 and float32 input rows."""
    n = 256 * 64 + 65
    dims = orc.ae_dims(24, 15)
    flat = orc.formula_params(dims, 43)
    x = np.random.default_rng(7).random((n, 24))
    if dtype == torch.float32:
        x = x.astype(np.float32).astype(np.float64)
    check(dims, flat, x, dev(x, dtype), throughput_pair)


def test_roles_pair_class_handle(throughput_pair):
    """A run-time-width class handle (AE(30, 8) on Impl<31, 15, RT>) at n = 130.  The class instantiations do NOT fit the role-split
    pair: their chain role needs 16-20 bytes of scratch per lane at 256 registers, so they stay on the one-wave pair and the knob
    changes nothing for them.  The case holds the class to the same two bars for the day one of them moves."""
    dims = orc.ae_dims(30, 8)
    flat = orc.formula_params(dims, 130)
    x = np.random.default_rng(30).random((130, 30))
    check(dims, flat, x, dev(x), throughput_pair)


# one shape per tile count the shared text of the four kernels is instantiated for
TILE_SHAPES = [
    (24, 2),     # Impl<24, 2>: partial latent tile, two live slots
    (24, 12),    # Impl<24, 12>: partial latent tile
    (40, 10),    # Impl<47, 15, RT>: three input tiles
    (30, 20),    # Impl<31, 31, RT>: two latent tiles
    (45, 20),    # Impl<47, 31, RT>
    (60, 5),     # Impl<63, 15, RT>: four input tiles, bias fragments read from L2
    (63, 31),    # Impl<63, 31, RT>
]


@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("shape", TILE_SHAPES, ids=lambda s: f"ae{s[0]}_{s[1]}")
def test_roles_pair_every_tile_count(shape, n, throughput_pair):
    """Every instantiation family of the pair at n = 65 (a full group and a one-row group) and n = 130, on the throughput pair.  The
    two 24-column shapes have both layouts; for the classes the knob picks the same kernel twice (see the class case above).  Rows
    are plain seeded uniform draws, as in the cases above: none of the fourteen puts a float32 pre-activation on the other side of the
    LeakyReLU kink than its float64 twin (rel 1.5e-7 .. 2.9e-7), so none needs test_gpu_parity.off_the_kink."""
    dims = orc.ae_dims(*shape)
    flat = orc.formula_params(dims, 100 * shape[0] + shape[1])
    x = np.random.default_rng(1000 * shape[0] + n).random((n, shape[0]))
    check(dims, flat, x, dev(x), throughput_pair)


def test_roles_pair_train_step_equals_fwd_bwd_then_adam(throughput_pair):
    """bamd_train_step == bamd_fwd_bwd + bamd_adam_step, bit for bit, on the role-split pair at n = 130."""
    throughput_pair.setenv("BALER_AMD_TRAIN_ROLES", "1")
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
