"""Barrier-interval timeline of the role-split fp32 training pair: shader-clock stamps of one workgroup (wave 0 = chain role, wave 4 =
weight-gradient role) over two consecutive iterations in the middle of a 1M-row bamd_fwd_bwd.  Needs a -DBAMD_ROLES_TRACE build:

    cd baler_amd/csrc && mkdir -p ../../.abl && \
      hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -mllvm -amdgpu-mfma-vgpr-form=1 \
            -DBAMD_ROLES_TRACE -c fused.hip -o ../../.abl/fused_roles_trace.o && \
      hipcc --offload-arch=gfx950 -shared -fPIC -o ../../.abl/roles_trace.so $(ls *.o | grep -v '^fused.o$') ../../.abl/fused_roles_trace.o -ldl
    BALER_AMD_LIB=$PWD/.abl/roles_trace.so python tools/roles_trace.py [ROLES ...]   (on the GPU box)

ROLES are values of BALER_AMD_TRAIN_ROLES (default: 1; 0 traces wave 0 of the one-wave pair, whose waves run both columns in turn and
whose intervals are the other schedule's: the table's MFMA columns do not describe it).  Per role and barrier interval the table gives the cycles the role worked
(release from the barrier in front of the interval -> arrival at the barrier behind it), the cycles it then stood at that barrier, and
the MFMAs it issues in the interval.  s_memtime ticks at a fixed rate that need not be the shader clock: compare ticks within one
run only (the iteration's ticks against its microseconds give the rate)."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from baler_amd import native, synth                               # noqa: E402
from baler_amd.modules import models                              # noqa: E402

FWD = 1073
DX = {7: 104, 6: 364, 5: 112, 4: 16, 3: 16, 2: 112, 1: 364}       # chain MFMAs per 16 rows
DW = {7: 112, 6: 368, 5: 112, 4: 16, 3: 16, 2: 112, 1: 368, 0: 112}
FWD0 = 78                                                          # en1 recomputed by the encoder-gradient kernel: 13 tiles x 6 k-steps


def intervals(kernel):
    """[(name, chain MFMAs, weight-gradient MFMAs)] per barrier interval, starting behind barrier 0: dW(l) runs beside dX(l)"""
    if kernel == 0:
        return [(f"dX{l}" + (" + fwd" if l == 2 else "") + f" | dW{l}", DX[l] + (FWD if l == 2 else 0), DW[l]) for l in (7, 6, 5, 4, 3, 2)]
    return [("dX1 | dW1", DX[1], DW[1]), ("fwd0 | dW0", FWD0, DW[0])]


def table(t, kernel):
    """t: [role][iteration][stamp]"""
    nb = 6 if kernel == 0 else 2
    rows = intervals(kernel)
    print(f"{'interval':22s} {'C mfma':>7s} {'D mfma':>7s} | {'C work':>8s} {'C wait':>8s} | {'D work':>8s} {'D wait':>8s} | {'release to release':>18s}")
    tot = 0
    for k in range(nb):
        cells = []
        for role in (0, 1):
            rel = t[role][0][3 + 2 * k]                                      # released from barrier k, iteration 0
            arr, nxt = (t[role][0][2 + 2 * (k + 1)], t[role][0][3 + 2 * (k + 1)]) if k + 1 < nb else (t[role][1][2], t[role][1][3])
            cells += [arr - rel, nxt - arr]
            span = nxt - rel
        tot += span
        name, c, d = rows[k]
        print(f"{name:22s} {c:7d} {d:7d} | {cells[0]:8d} {cells[1]:8d} | {cells[2]:8d} {cells[3]:8d} | {span:18d}")
    fwd = t[0][1][1] - t[0][1][0]
    print(f"iteration (barrier 0 to barrier 0): {tot} ticks; the chain role's forward alone: {fwd} ticks; "
          f"MFMAs per SIMD and iteration: {sum(r[1] + r[2] for r in rows)}")


def main():
    dev = torch.device("cuda", 0)
    n = 1_000_000
    raw = torch.as_tensor(synth.cms_rows(n)).to(dev)
    x = native.normalize(raw, native.minmax(raw), torch.float64)
    torch.manual_seed(0)
    model = models.AE(24, 15, mode="fp32").to(dev)
    h = model.handle()
    grads = torch.zeros_like(model.flat)
    L = native.lib()
    L.bamd_debug_roles_trace.argtypes = [ctypes.c_void_p, ctypes.c_int]
    for roles in (sys.argv[1:] or ["1"]):
        os.environ["BALER_AMD_TRAIN_ROLES"] = roles
        for _ in range(20):
            h.fwd_bwd(x, grads)
        torch.cuda.synchronize()
        buf = (ctypes.c_ulonglong * 128)()
        rc = L.bamd_debug_roles_trace(buf, 128)
        t = np.array(buf[:], dtype=np.int64).reshape(2, 2, 2, 16)
        for kernel, kname in ((0, "train_dec_roles_kernel"), (1, "train_enc_roles_kernel")):
            print(f"\nBALER_AMD_TRAIN_ROLES={roles} rc={rc}  {kname}, workgroup 100, iterations 30 and 31 of 61; s_memtime ticks")
            table(t[kernel], kernel)


if __name__ == "__main__":
    main()
