"""Two builds of libbaler_amd.so in ONE process on the small-batch training step of both precisions (csrc/small_step.hpp, fused.hip:
lat2_chain_kernel, lat4_chain_kernel, lat2_dw_kernel; fused64.hip / fused64q.hip: chain64_kernel, chain64r_kernel, chain64q_kernel,
dw64_kernel, dw64m_kernel, dw64x_kernel; generic.hip: dw_small_all_k): the same bits, and time per call.

    python tools/small_step_ab.py PARENT_LIB [BRANCH_LIB] [--branch-first] [--bits-only]      (BRANCH_LIB: default the in-tree library)
    rocprofv3 --kernel-trace --stats -- python tools/small_step_ab.py --one LIB     (the same lines on ONE library, five calls each)

Loading, comparison and timing are those of tools/wide_host_ab.py (12 rounds, parent and branch alternating inside every round, the
bar  branch median - parent median <= parent's max - min).  Bits per line: [grads | loss] of fwd_bwd, then params, m, v after three
train_steps and the next fwd_bwd on the stepped parameters -- a changed fragment map or scatter list shows up there.  Time per line:
fwd_bwd; on the TRAIN lines train_step as well."""
import os
import sys

import torch

import wide_host_ab as ab

AE = lambda F, Z: [F, 200, 100, 50, Z, 50, 100, 200, F]      # noqa: E731
CHUNK64 = {"BALER_AMD_LATENCY_ROWS": "32", "BALER_AMD_CLASS_CHUNK_ROWS": "64"}
SMALL_ALL = [30, 64, 32, 9, 32, 64, 30]
# (label, dims, mode, knobs set while the handles are made and the calls run, rows)
LINES = [
    ("AE(24,15)", AE(24, 15), "fp32", {}, (17, 513, 1040, 4099, 8192, 12288)),
    ("AE(24,15) LAT4_ROWS=0", AE(24, 15), "fp32", {"BALER_AMD_LAT4_ROWS": "0"}, (513,)),
    ("AE(24,15) LATENCY_ROWS=0", AE(24, 15), "fp32", {"BALER_AMD_LATENCY_ROWS": "0"}, (16449,)),
    ("AE(40,10)", AE(40, 10), "fp32", {}, (513,)),
    ("AE(100,12)", AE(100, 12), "fp32", {}, (513,)),
    ("AE(100,12) class-chunk64", AE(100, 12), "fp32", CHUNK64, (129,)),
    ("AE(24,15)", AE(24, 15), "fp64", {}, (17, 512, 1040, 1552, 16384)),
    ("AE(24,15) QCHAIN_BLKS=0", AE(24, 15), "fp64", {"BALER_AMD_F64_QCHAIN_BLKS": "0"}, (512,)),
    ("AE(24,15) REGCHAIN_BLKS=0", AE(24, 15), "fp64", {"BALER_AMD_F64_REGCHAIN_BLKS": "0"}, (512,)),
    ("AE(40,10)", AE(40, 10), "fp64", {}, (513,)),
    ("AE(80,16)", AE(80, 16), "fp64", {}, (512,)),
    ("30-64-32-9-32-64-30", SMALL_ALL, "fp32", {}, (129,)),
    ("30-64-32-9-32-64-30", SMALL_ALL, "fp64", {}, (129,)),
]
# train_step timed as well: (dims, mode, rows)
TRAIN = {(24, "fp32"): (512, 4096, 12288), (24, "fp64"): (512, 16384, 65536)}


def main():
    one = sys.argv[1] == "--one"
    bits_only = "--bits-only" in sys.argv
    argv = [a for a in sys.argv[1:] if a != "--bits-only"]
    libs = {"parent": ab.load_native("native_one", argv[1])} if one else ab.load_libs(argv)
    outside = differ = 0
    for label, dims, mode, env, sizes in LINES:
        os.environ.update(env)
        dt = torch.float64 if mode == "fp64" else torch.float32
        hs, p0 = {}, None
        for who, nat in libs.items():
            hs[who] = nat.Handle(dims, mode)
            if p0 is None:
                p0 = ((torch.rand(hs[who].nparams + 1, generator=torch.Generator().manual_seed(dims[0]), dtype=torch.float64) - 0.5) * 0.1).to(dt).cuda()
        extra = TRAIN.get((dims[0], mode), ()) if not env and len(dims) == 9 else ()
        for n in sorted(set(sizes) | set(extra)):
            x = torch.rand((n, dims[0]), dtype=torch.float32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(n))
            st = {w: dict(p=p0.clone(), m=torch.zeros_like(p0), v=torch.zeros_like(p0), g=torch.zeros_like(p0), g2=torch.zeros_like(p0))
                  for w in hs}

            def reset(w):
                st[w]["p"].copy_(p0)
                st[w]["m"].zero_()
                st[w]["v"].zero_()
                hs[w].load_params(st[w]["p"])

            def fwd_bwd(w):
                hs[w].fwd_bwd(x, st[w]["g"])

            def steps(w, k=3):
                for step in range(1, k + 1):
                    hs[w].train_step(x, st[w]["p"], st[w]["m"], st[w]["v"], step, 1e-3, grads=st[w]["g2"])

            def bits_call(w):      # fwd_bwd on the seeded parameters, three steps, fwd_bwd on the stepped ones
                reset(w)
                fwd_bwd(w)
                st[w]["g0"] = st[w]["g"].clone()
                steps(w)
                fwd_bwd(w)

            if one:
                for w in hs:
                    reset(w)
                    for _ in range(5):
                        fwd_bwd(w)
                    steps(w, 5)
                torch.cuda.synchronize()
                continue
            if n in sizes:
                for w in hs:
                    bits_call(w)
                torch.cuda.synchronize()
                outs = lambda w: [st[w][k] for k in ("g0", "p", "m", "v", "g2", "g")]      # noqa: E731
                same = all(torch.equal(ab.bits(a), ab.bits(b)) for a, b in zip(outs("parent"), outs("branch")))
                differ += not same
                if bits_only:
                    print(f"{label:26s} {mode:5s} n={n:<6d} fwd_bwd, 3 train_steps, fwd_bwd: same bits: {same}", flush=True)
                    continue
                print(f"{label:26s} {mode:5s} n={n:<6d} [grads | loss], params, m, v after 3 train_steps, next [grads | loss]: same bits: {same}")
                for w in hs:
                    reset(w)
                inside, _ = ab.ab_line(f"{label:26s} {mode:5s} n={n:<6d} fwd_bwd   ", list(hs), fwd_bwd, lambda w: [st[w]["g"]])
                outside += not inside
            if n in extra and not bits_only:
                for w in hs:
                    reset(w)
                # (every timed step is step 1 on whatever the steps before left: the time does not depend on the values)
                inside, _ = ab.ab_line(f"{label:26s} {mode:5s} n={n:<6d} train_step", list(hs), lambda w: steps(w, 1), lambda w: [])
                outside += not inside
        del hs
        for k in env:
            del os.environ[k]
    if not one:
        print(f"{outside} lines outside the parent's spread; {differ} lines with different bits")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
