"""Two builds of libbaler_amd.so in ONE process on the short-side weight-gradient kernels (csrc/generic.hip: dw_short_k, dw_wide_k,
dw_wide_bf16_k, dw_short_bf16_k): the same bits from fwd_bwd, and time per call.

    python tools/dw_short_ab.py PARENT_LIB [BRANCH_LIB] [--branch-first]      (BRANCH_LIB: default the in-tree library)
    rocprofv3 --kernel-trace --stats -- python tools/dw_short_ab.py --one LIB     (the same lines on ONE library, five calls each: the
                                                                                    workload of a per-kernel duration run)

Loading, comparison and timing are those of tools/wide_host_ab.py (12 rounds, parent and branch alternating inside every round, the
bar  branch median - parent median <= parent's max - min).  Lines: the shapes and row counts of tests/test_gpu_dw_short.py under its
knobs (BALER_AMD_DW_SMALL_ROWS=0, BALER_AMD_WIDE_SMALL_ROWS=0, and 512-6 in bf16 once more under BALER_AMD_BF16_DZ16=0), then the
full-size lines under the defaults: C4 (2500, 25) at 32,768 frames and (625, 7) at 131,072 blocks in fp32 and bf16, (512, 6) at 262,144
rows in bf16, AE(24, 15) through fwd_bwd_latent at 65,536 rows."""
import os
import sys

import torch

import wide_host_ab as ab

AE = lambda F, Z: [F, 200, 100, 50, Z, 50, 100, 200, F]      # noqa: E731
SMALL = {"BALER_AMD_DW_SMALL_ROWS": "0", "BALER_AMD_WIDE_SMALL_ROWS": "0"}
TEST_ROWS = (128, 129, 257)
# (label, dims, mode, knobs set while the handles are made and the calls run, rows, through fwd_bwd_latent)
LINES = [
    ("AE(24,15) layer-wise", AE(24, 15), "fp32", dict(SMALL, BALER_AMD_FORCE_GENERIC="1"), TEST_ROWS, False),
    ("16-208-16-208-16", [16, 208, 16, 208, 16], "fp32", SMALL, TEST_ROWS, False),
    ("(625, 7)", AE(625, 7), "fp32", SMALL, TEST_ROWS, False),
    ("(625, 7)", AE(625, 7), "bf16", SMALL, TEST_ROWS, False),
    ("(512, 6)", AE(512, 6), "fp32", SMALL, TEST_ROWS, False),
    ("(512, 6)", AE(512, 6), "bf16", SMALL, TEST_ROWS, False),
    ("(512, 6) DZ16=0", AE(512, 6), "bf16", dict(SMALL, BALER_AMD_BF16_DZ16="0"), TEST_ROWS, False),
    ("C4 (2500, 25)", AE(2500, 25), "fp32", {}, (32768,), False),
    ("C4 (2500, 25)", AE(2500, 25), "bf16", {}, (32768,), False),
    ("(625, 7)", AE(625, 7), "fp32", {}, (131072,), False),
    ("(625, 7)", AE(625, 7), "bf16", {}, (131072,), False),
    ("(512, 6)", AE(512, 6), "bf16", {}, (262144,), False),
    ("AE(24,15) latent", AE(24, 15), "fp32", {}, (65536,), True),
]


def main():
    one = sys.argv[1] == "--one"
    libs = {"parent": ab.load_native("native_one", sys.argv[2])} if one else ab.load_libs(sys.argv[1:])
    outside = differ = 0
    for label, dims, mode, env, sizes, latent in LINES:
        os.environ.update(env)
        hs, p = {}, None
        for who, nat in libs.items():
            hs[who] = nat.Handle(dims, mode)
            if p is None:
                p = ((torch.rand(hs[who].nparams + 1, generator=torch.Generator().manual_seed(dims[0])) - 0.5) * 0.1).cuda()
            hs[who].load_params(p)
        for n in sizes:
            x = torch.rand((n, dims[0]), dtype=torch.float32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(n))
            lg = 1e-3 * torch.randn((n, dims[len(dims) // 2]), dtype=torch.float32, device="cuda",
                                    generator=torch.Generator(device="cuda").manual_seed(n + 1))
            grads = {w: torch.zeros_like(p) for w in hs}
            call = (lambda w: hs[w].fwd_bwd_latent(x, lg, grads[w])) if latent else (lambda w: hs[w].fwd_bwd(x, grads[w]))
            if one:
                for _ in range(5):
                    call("parent")
                torch.cuda.synchronize()
                continue
            inside, same = ab.ab_line(f"{label:22s} {mode:5s} n={n:<6d} fwd_bwd{'_latent' if latent else '':7s}", list(hs), call,
                                      lambda w: [grads[w]])
            outside += not inside
            differ += not same
        del hs
        for k in env:
            del os.environ[k]
    if not one:
        print(f"{outside} lines outside the parent's spread; {differ} lines with different bits")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
