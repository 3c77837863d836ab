"""The 17 instantiations of the short-side weight-gradient kernels (csrc/generic.hip: dw_short_k, dw_wide_k, dw_wide_bf16_k,
dw_short_bf16_k) at the smallest shapes that reach them, against the project's existing references and bars.

Every case runs under BALER_AMD_DW_SMALL_ROWS=0: up to 768 rows the one-launch kernel (dw_small_all_k) takes every weight gradient
otherwise.  plan_short_dw then gives each layer [dW | db] = dZ^T [X | 1] (K -> N columns) the side with fewer 16-column tiles as P
(P_IS_N: P = dZ), PT = its tiles, and the strided-tile kernels where PT = 13 and both widths are multiples of 4:

    AE(24, 15), layer-wise, fp32        layers 0..7: dw_short_k<2,2,false> <7,2,true> <4,2,true> <1,2,true> <1,2,false> <4,2,false>
                                        <7,2,false> <2,2,true>
    CFD_dense_AE(625, 7)   fp32         layers 0 and 7: dw_short_k<13,2,true>, <13,2,false>          (625 columns: rows not 16-byte)
                           bf16         ...             dw_short_bf16_k<13,2,true>, <13,2,false>
    CFD_dense_AE(512, 6)   fp32         layers 0 and 7: dw_wide_k<true>, <false>
                           bf16         ...             dw_wide_bf16_k<true>, <false, true>          (dL/drecon stored as bfloat16)
                           bf16, BALER_AMD_BF16_DZ16=0  dw_wide_bf16_k<false, false>
    16 -> 208 -> 16 -> 208 -> 16, fp32  K + 1 = 17 and 209 start a tile: the ones column is lane 0 of a tile of its own, as the last P
                                        tile (dw_short_k<2,2,false>, layers 0 and 2) and as the last Q tile (<1,2,true>, layers 1, 3)
    (layers 1..6 of the two wide models: the 200-100-50-Z-50-100-200 kernels of the first line, float32 on every handle.)
512 columns and not 2500: nothing in these kernels depends on the width beyond "a multiple of 4, more than 192".  Which kernel ran
cannot be asserted from here; profiles/dw_short_one_text.txt carries the kernel trace of this file with all 17 names.

Rows, and the row splits the plan cuts them into (at most rows / 64 splits, each a multiple of 16 rows; all of these layers: the same):
    128 -> 64 + 64         fp32: 4 blocks of 16 rows, the ping-pong's even exit;           bf16: 2 blocks of 32, no ragged block
    129 -> 80 + 49         fp32: 5 blocks, the odd exit / 3 blocks, the odd exit, + 1 row; bf16: 2 blocks + 16 rows (lane groups 2 and
                                                                                           3 hold no row) / 1 block + 17 rows
    257 -> 80 + 80 + 80 + 17   fp32: 5 blocks / ONE block, + 1 row;                        bf16: 2 blocks + 16 rows / no block, 17 rows
(257 stands where 177 -> 96 + 81 would: 6 and 5 blocks, no split of one block, which is the third exit of the ping-pong.)

fp32: the gradient tensor by tensor against the fp64 oracle (tests/grad_tensors.py) at the bar of tests/test_gpu_grad_tensors.py, on
rows off the LeakyReLU kink.  bf16: against bf16_ref.wide_train_pass under the training rule of tests/test_gpu_bf16_contract.py.
BALER_AMD_BF16_DZ16=0: the same rule, and the same bits as the default (the 16-bit store rounds as the kernels' loads do)."""
import numpy as np
import pytest
import torch

import grad_tensors as gt
from test_bf16_contract_host import training_rule, wide_train_case
from test_gpu_bf16_contract import make_handle, run_pass
from test_gpu_grad_tensors import TOL      # (the fp32 bar of that module: 1e-5)
from test_gpu_guard_bands import dev, family, host

pytestmark = pytest.mark.gpu

ROWS = (128, 129, 257)
SEED = 5000
ONES_OWN_TILE = ("dims", [16, 208, 16, 208, 16], 16, "fp32", {}, ("default",), ("default",))
FP32 = {"layerwise-ae24-fp32": None, "cfd625-fp32": None, "wide512-fp32": None, "ones-own-tile": ONES_OWN_TILE}
BF16 = ((625, 7), (512, 6))


@pytest.fixture(autouse=True)
def _per_layer_weight_gradients(monkeypatch):
    monkeypatch.setenv("BALER_AMD_DW_SMALL_ROWS", "0")


@pytest.mark.parametrize("name", list(FP32))
def test_fp32_gradient_tensors(name, monkeypatch):
    h, ref, _, cmode, _ = family(name, "default", monkeypatch, spec=FP32[name])
    assert cmode == "fp32"
    dims, bar = list(ref.dims), TOL["fp32"]
    for n in ROWS:
        x = ref.rows(n, SEED + n).astype(np.float32)      # float32 rows off the kink; the oracle on exactly these rows
        lo, go = ref.fwd_bwd(x.astype(np.float64))
        g = torch.full((h.nparams + 1,), 3.0, dtype=torch.float32, device="cuda")
        h.fwd_bwd(dev(x), g)
        g = host(g)
        lerr = abs(g[-1] - lo) / lo
        print(f"    {name} n={n}: loss {lerr:.3e} (bar {bar:g})")
        assert lerr <= bar, f"{name} n={n}: loss"
        gt.assert_per_tensor(g[:-1], go, dims, bar, f"{name} n={n} fwd_bwd")


@pytest.mark.parametrize("F,Z", BF16)
def test_bf16_training_rule(F, Z, monkeypatch):
    monkeypatch.setenv("BALER_AMD_WIDE_SMALL_ROWS", "0")      # (a BF16 handle's small batches run the float32 split launches by default)
    for n in ROWS:
        c = wide_train_case(F, Z, n)
        h, p = make_handle(c["dims"], c["flat"], path="fused")
        training_rule(f"{F}-{Z} n={n}", *run_pass(h, p, dev(c["x"])), c)


def test_bf16_dz16_off_is_the_same_bits(monkeypatch):
    """dL/drecon in float32 (dw_wide_bf16_k<false, false>) against the default's bfloat16 store (<false, true>)."""
    monkeypatch.setenv("BALER_AMD_WIDE_SMALL_ROWS", "0")
    F, Z = 512, 6
    for n in ROWS:
        c = wide_train_case(F, Z, n)
        h, p = make_handle(c["dims"], c["flat"], path="fused")
        g16 = torch.zeros_like(p)
        h.fwd_bwd(dev(c["x"]), g16)
        monkeypatch.setenv("BALER_AMD_BF16_DZ16", "0")
        loss, g = run_pass(h, p, dev(c["x"]))
        training_rule(f"{F}-{Z} n={n} BALER_AMD_BF16_DZ16=0", loss, g, c)
        g32 = torch.zeros_like(p)
        h.fwd_bwd(dev(c["x"]), g32)
        monkeypatch.delenv("BALER_AMD_BF16_DZ16")
        assert torch.equal(g16.view(torch.int32), g32.view(torch.int32)), f"{F}-{Z} n={n}: BALER_AMD_BF16_DZ16=0 changes the gradient's bits"
