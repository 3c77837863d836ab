"""Two builds of libbaler_amd.so in ONE process on the wide-layer family's entry points: same bits, and time per call.

    python tools/wide_host_ab.py PARENT_LIB [BRANCH_LIB] [--branch-first]      (BRANCH_LIB: default the in-tree library)

Both libraries are loaded through their own instance of baler_amd/native.py (BALER_AMD_LIB set around the import).  Cases:
CFD_dense_AE(2500, 25) on an fp32 and a bf16 handle at 60, 6,000 and 32,768 rows, AE(300, 20) (the run-time-width class) on an fp32
handle at 60 and 6,000 rows; calls encode, decode, forward_loss (with the reconstruction) and fwd_bwd on resident float32 rows.
"same bits": every output of the two libraries compared as bit patterns.  Time: 12 rounds, parent and branch alternating inside every
round and the order swapping from round to round (the interleaving of tools/train_roles_ab.py), each sample the mean of CALLS calls
between two HIP events; per line the medians, and the bar  branch median - parent median <= parent's max - min over its rounds."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
ROUNDS = 12
CASES = [((2500, 25), "fp32", (60, 6000, 32768)), ((2500, 25), "bf16", (60, 6000, 32768)), ((300, 20), "fp32", (60, 6000))]


def load_native(name, lib_path):
    os.environ["BALER_AMD_LIB"] = os.path.abspath(lib_path)
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "baler_amd", "native.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.lib()
    del os.environ["BALER_AMD_LIB"]
    return mod


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def ab_line(label, who, call, outs):
    """One line: call(w) for w in `who` = ["parent", "branch"] (in creation order); outs(w) -> the tensors compared as bit patterns.
    Prints the medians over ROUNDS rounds and whether branch - parent is within the parent's spread; returns (that, same bits)."""
    for w in who:
        call(w)
    torch.cuda.synchronize()
    same = all(torch.equal(bits(a), bits(b)) for a, b in zip(outs("parent"), outs("branch")))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call("parent")
    e1.record()
    e1.synchronize()
    ncall = int(min(50, max(3, 2.0 / max(e0.elapsed_time(e1), 1e-3))))      # ~2 ms per sample
    for w in who:
        for _ in range(ncall):
            call(w)
    us = {w: [] for w in who}
    for r in range(ROUNDS):
        for w in (("parent", "branch") if r % 2 == 0 else ("branch", "parent")):
            e0.record()
            for _ in range(ncall):
                call(w)
            e1.record()
            e1.synchronize()
            us[w].append(1e3 * e0.elapsed_time(e1) / ncall)
    pm, bm = float(np.median(us["parent"])), float(np.median(us["branch"]))
    spread = max(us["parent"]) - min(us["parent"])
    inside = bm - pm <= spread
    print(f"{label} parent med {pm:9.2f} us  min {min(us['parent']):9.2f}  max {max(us['parent']):9.2f}  "
          f"(spread {spread:7.2f}) | branch med {bm:9.2f}  min {min(us['branch']):9.2f}  max {max(us['branch']):9.2f} | "
          f"branch - parent {bm - pm:+8.2f} us: {'WITHIN' if inside else 'OUTSIDE'} spread; same bits: {same}", flush=True)
    return inside, same


def load_libs(argv):
    """argv: PARENT_LIB [BRANCH_LIB] [--branch-first] -> {"parent": native module, "branch": native module}"""
    args = [a for a in argv if a != "--branch-first"]      # --branch-first: the branch's library and handles are created first
    parent_lib = args[0]
    branch_lib = args[1] if len(args) > 1 else os.path.join(ROOT, "baler_amd", "libbaler_amd.so")
    order = [("parent", parent_lib), ("branch", branch_lib)][::-1 if "--branch-first" in argv else 1]
    return {who: load_native("native_" + who, path) for who, path in order}


def main():
    libs = load_libs(sys.argv[1:])
    outside = 0
    for (F, Z), mode, sizes in CASES:
        dims = [F, 200, 100, 50, Z, 50, 100, 200, F]
        hs, p = {}, None
        for who, nat in libs.items():
            hs[who] = nat.Handle(dims, mode)
            if p is None:
                p = ((torch.rand(hs[who].nparams + 1, generator=torch.Generator().manual_seed(F)) - 0.5) * 0.1).cuda()
            hs[who].load_params(p)
        for n in sizes:
            x = torch.rand((n, F), dtype=torch.float32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(n))
            z = {w: torch.empty((n, Z), dtype=torch.float32, device="cuda") for w in hs}
            rec = {w: torch.empty((n, F), dtype=torch.float32, device="cuda") for w in hs}
            loss = {w: torch.zeros(1, dtype=torch.float64, device="cuda") for w in hs}
            fl = {}
            grads = {w: torch.zeros_like(p) for w in hs}

            def fwd_loss(w):
                fl[w] = hs[w].forward_loss(x, loss_out=loss[w])[0]

            calls = {
                "encode": (lambda w: hs[w].encode(x, out=z[w]), lambda w: [z[w]]),
                "decode": (lambda w: hs[w].decode(z[w], out=rec[w]), lambda w: [rec[w]]),
                "forward_loss": (fwd_loss, lambda w: [fl[w], loss[w]]),
                "fwd_bwd": (lambda w: hs[w].fwd_bwd(x, grads[w]), lambda w: [grads[w]]),
            }
            for what, (call, outs) in calls.items():
                outside += not ab_line(f"({F}, {Z}) {mode:5s} n={n:<6d} {what:13s}", list(hs), call, outs)[0]
    print(f"{outside} lines outside the parent's spread")


if __name__ == "__main__":
    main()
