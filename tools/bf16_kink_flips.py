#!/usr/bin/env python3
"""How much of a BF16 handle's gradient error is LeakyReLU units that sit within bfloat16 rounding of the kink?  CPU only (NumPy).

A float64 forward + backward of the dense autoencoder whose ONLY difference from the reference is that the LeakyReLU signs come from
a forward with bfloat16-rounded operands in the wide products (en1 and de4: what the wide bf16 kernels round) or in every layer;
everything else, the backward included, is exact.  Per layer (weights and bias together) and on the whole vector, rel-L2 against the
reference, with the latent term of tests/test_gpu_guard_bands.py at a fixed 0.01 N(0, 1) and without one.  The rows and parameters are
those of that test's cfd2500 / cfd625 cases at 129 rows.

    python tools/bf16_kink_flips.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle import c_oracle as orc                  # noqa: E402


def bf(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def fwd_bwd(dims, flat, x, lg, mode):
    """mode None: the reference; "wide": signs from a forward with bf16 operands in layers 0 and L-1; "all": in every layer."""
    L, lay, off = len(dims) - 1, [], 0
    for l in range(L):
        K, N = dims[l], dims[l + 1]
        lay.append((flat[off:off + K * N].reshape(N, K), flat[off + K * N:off + K * N + N]))
        off += K * N + N
    lin = (L // 2 - 1, L - 1)
    ys, yb, sign = [x], x, []
    for l, (W, b) in enumerate(lay):
        a = ys[-1] @ W.T + b
        rounded = mode == "all" or (mode == "wide" and l in (0, L - 1))
        ab = (bf(yb) @ bf(W).T + b) if rounded else (yb @ W.T + b)          # the perturbed forward, carried on
        sign.append((ab if mode else a) > 0)
        ys.append(a if l in lin else np.where(sign[-1], a, 0.01 * a))
        yb = ab if l in lin else np.where(ab > 0, ab, 0.01 * ab)
    dz, g = 2.0 * (ys[-1] - x) / dims[0], [None] * L
    for l in range(L - 1, -1, -1):
        if l not in lin:
            dz = dz * np.where(sign[l], 1.0, 0.01)
        if l == L // 2 - 1 and lg is not None:
            dz = dz + lg
        g[l] = np.concatenate([(dz.T @ ys[l]).ravel(), dz.sum(0)])
        dz = dz @ lay[l][0]
    return g


def main():
    import test_gpu_guard_bands as T                # (imports the library's Python side; no GPU is touched)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)      # noqa: E731
    for F, Z in ((2500, 25), (625, 7)):
        dims = orc.ae_dims(F, Z)
        flat = f32(orc.formula_params(dims, 100 + F + Z))
        x = f32(T.DenseRef(dims, flat).rows(129, 2129))
        for scale in (0.01, None):
            lg = None if scale is None else f32(np.random.default_rng(129).normal(size=(129, Z)) * scale)
            g0 = fwd_bwd(dims, flat, x, lg, None)
            for mode in ("wide", "all"):
                g1 = fwd_bwd(dims, flat, x, lg, mode)
                tot = np.linalg.norm(np.concatenate(g1) - np.concatenate(g0)) / np.linalg.norm(np.concatenate(g0))
                per = " ".join(f"{np.linalg.norm(a - b) / np.linalg.norm(b):.1e}" for a, b in zip(g1, g0))
                print(f"F={F} latent={scale} bf16 operands: {mode:4s}  whole vector {tot:.2e}  per layer {per}")


if __name__ == "__main__":
    main()
