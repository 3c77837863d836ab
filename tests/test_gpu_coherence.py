"""Coherence tests: every call sees the parameters the last step left (tests/coherence.py; DESIGN.md, "Coherence of the weight copies").

One test per (family, training routing): TRAIN_CASES of tests/test_gpu_guard_bands.py plus the three EXTRA families of
tests/test_gpu_streams.py.  The plan of tests/coherence.py (eight writers, the row classes of its docstring) is walked on ONE long-lived
handle with one caller-side state (p, m, v, t, loss_accum) that is never reset.  After every writer:
  (a) every reader output of the long-lived handle equals, bit for bit, that of a fresh twin (same constructor arguments, same
      environment) loaded with bamd_load_params from the caller's current p.  No tolerance: all sums on these paths are fixed-order.
      The long-lived handle has run every larger row class before, so no call may read what an earlier one left in a workspace either.
      The reader that comes FIRST after the writer is the one that meets the stale flags (whichever entry point runs first re-packs and
      clears them): it rotates, so that every reader kind leads once per case and decode, forward_loss, fwd_bwd and fwd_bwd_latent each
      lead once at the largest row class straight after a writer that stepped (tests/coherence.py; asserted in test_plan_coverage).
  (b) the writer itself: p, m, v against coherence.adam_expect fed the call's own returned gradient and the device state from before
      the call, within 1 ulp of float32 (8 ulp of float64 on an fp64 handle); that returned gradient equals, bit for bit, fwd_bwd
      (fwd_bwd_latent) on the same rows of a fresh twin loaded with the parameters from before the call: the step was computed on the
      weights the last step left, not on those of one step ago; loss_accum equals the running sum of the returned loss slots; the two
      epoch writers equal, bit for bit, a twin that runs the same batches as single train_step calls from the same state.
  (c) negative control: a twin loaded with the parameters from BEFORE the writer differs from the long-lived handle in the bits of every
      reader output, and p differs from its old value in more than 99 % of its elements.  (FPGA_prototype_model: of the elements a
      gradient has reached, m or v non-zero, which must be more than half of the vector -- a ReLU unit that is off on every row has an
      exactly zero gradient, and with zero moments Adam has nothing to move its weights by: 29 % of this model at its starting weights.)
  (d) once, at the end: encode, forward_loss and fwd_bwd of the long-lived handle on 129 rows off the kink of the final parameters
      against the family's reference at host(p), under bar_ok / grad_ok of the guard-band module unchanged (the fp16 inference mode,
      which that module has no bar for: a quarter of its narrow bf16 bar, which is what tests/test_gpu_f16.py holds fp16 to against a
      bf16 handle).  tests/test_coherence_host.py shows that plain float32 arithmetic keeps half those bars at these parameters.
Every case prints family, h.path, compute mode, routing and the row classes.

Which kernels ran cannot be asserted from here; profiles/coherence_kernel_trace.txt is the kernel trace of this module.  It must name
  every kernel with an Adam epilogue   lat2_dw_kernel (fused.hip: the fp32 small-batch steps, bf16 / fp16 / fp16x3 handles included),
                                       dw64_kernel (fused64.hip), dw_small_all_k (generic.hip: the layer-wise path and the wide models up
                                       to BALER_AMD_DW_SMALL_ROWS), fpga_reduce_k (fpga.hip)
  the plain Adam launch                adam_k (elementwise.hip: adam_step, the larger batches of every family, PJ_Conv_AE)
  the pack / re-pack kernels           pack_k (fused.hip), pack_wide_bf16_k (fused.hip: pack_extra), pack16_k (bf16.hip), pack_train_k
                                       (bf16_train.hip), pack_bias_k (bf16_net.hpp), pack_split_k (f16x3.hip), pack64_k (fused64.hip)
each at least once per family that has it.  A name missing from the trace means a wrong row class in tests/coherence.py."""
import numpy as np
import pytest
import torch

import coherence as co
from baler_amd import native
from test_gpu_guard_bands import (FAMILIES, ROUTES, TOL, activation_means_raw, assert_same_bits, bar_ok, dev, feats_of, forward_loss_raw,
                                  grad_ok, host)
from test_gpu_parity import rel_l2
from test_gpu_streams import EXTRA, make_family, other_params

pytestmark = pytest.mark.gpu

F32, F64, F16 = torch.float32, torch.float64, torch.float16
CASES = co.cases(FAMILIES, EXTRA)
F16_BAR = 2e-2 / 4


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def differs(a, b):
    return not torch.equal(_bits(a), _bits(b))


def twin_of(case, h, p):
    """A fresh handle with the long-lived one's constructor arguments (the environment is the case's), loaded with p."""
    mode = (FAMILIES.get(case.name) or EXTRA[case.name])[3]
    if case.kind == "pj":
        t = native.Handle.pj_conv(h.z_dim, mode)
    elif case.kind == "fpga":
        t = native.Handle(h.dims, mode, act="relu")
    else:
        t = native.Handle(h.dims, mode)
    assert (t.path, t.compute_mode, t.nparams) == (h.path, h.compute_mode, h.nparams)
    t.load_params(p)
    return t


class Inputs:
    """The readers' inputs of one case, made once per row class."""

    def __init__(self, h):
        self.h, self.F, self.Z = h, h.dims[0], h.z_dim
        self.xdt = F64 if h.param_dtype == F64 else F32
        self.fnp, _ = feats_of(self.F)
        self.feats = dev(self.fnp)
        self.by_rows = {}

    def of(self, n):
        if n not in self.by_rows:
            x = dev(co.uniform_rows(n, self.F, 200 + n), self.xdt)
            z = dev(np.random.default_rng(300 + n).normal(size=(n, self.Z)) * 0.5, self.xdt)
            self.by_rows[n] = {"x": x, "xraw": dev(host(x) * self.fnp[1] + self.fnp[0], self.xdt), "z": z, "z16": z.to(F16),
                               "lg": dev(co.latent_term(n, self.Z, self.F, n), self.h.param_dtype)}
        return self.by_rows[n]


def read(h, r, ins):
    """One reader of the plan on handle h -> {name: output}."""
    d, pdt, np_ = ins.of(r.rows), h.param_dtype, h.nparams
    x, fe = (d["xraw"], ins.feats) if r.features else (d["x"], None)
    n = r.rows
    if r.kind == "encode":
        return {"z32": h.encode(x, features=fe, out_dtype=F32), "z64": h.encode(x, features=fe, out_dtype=F64)}
    if r.kind == "encode16":
        return {"z16": h.encode(x, out_dtype=F16)}
    if r.kind == "decode":
        return {"out": h.decode(d["z"], out_dtype=ins.xdt), "out_of_16": h.decode(d["z16"], out_dtype=F32)}
    if r.kind == "forward_loss":
        o = {"recon": torch.zeros((n, ins.F), dtype=ins.xdt, device="cuda"), "loss": torch.zeros(1, dtype=F64, device="cuda")}
        forward_loss_raw(h, x, fe, o["recon"], o["loss"])
        return o
    g = torch.zeros(np_ + 1, dtype=pdt, device="cuda")
    if r.kind == "fwd_bwd":
        h.fwd_bwd(x, g, features=fe)
        return {"g": g}
    if r.kind == "fwd_bwd_latent":
        h.fwd_bwd_latent(x, d["lg"], g)
        return {"g": g}
    assert r.kind == "activation_means"
    o = torch.zeros((len(h.dims) - 3, 200), dtype=F64, device="cuda")
    activation_means_raw(h, x, fe, o)
    return {"means": o}


def infer_ok(cmode, wide, got, want, odt, what):
    if cmode == "fp16":
        err = rel_l2(got, want)
        print(f"    oracle {what}: {err:.3e} (bar {F16_BAR:g})")
        assert err <= F16_BAR, what
    else:
        bar_ok(cmode, wide, got, want, odt, what)


@pytest.mark.parametrize("case", CASES, ids=[f"{c.name}-{c.route}" for c in CASES])
def test_every_call_sees_the_last_step(case, monkeypatch):
    h, ref, flat, cmode, wide = make_family(case.name, case.route, monkeypatch)
    print(f"[coherence] family={case.name} path={h.path} compute={cmode} routing={case.route} {ROUTES[case.route]} row classes={case.classes}")
    F, Z, np_, pdt = h.dims[0], h.z_dim, h.nparams, h.param_dtype
    npdt = np.float64 if pdt == F64 else np.float32
    bar = co.adam_bar(npdt)
    ins = Inputs(h)
    p, m, v = flat.clone(), torch.zeros_like(flat), torch.zeros_like(flat)
    acc = torch.full((1,), 0.25, dtype=F64, device="cuda")
    acc_want = 0.25
    g = torch.zeros(np_ + 1, dtype=pdt, device="cuda")

    def hp(s):
        return dict(beta1=s.b1, beta2=s.b2, eps=s.eps)

    def adam_ok(tag, s, t, before, g):
        want = co.adam_expect(*(host(a)[:np_] for a in (before[0], g, before[1], before[2])), t, s.lr, s.b1, s.b2, s.eps, npdt)
        worst = [co.ulps(host(a)[:np_], w, npdt).max() for a, w in zip((p, m, v), want)]
        print(f"    {tag}: Adam restated, worst ulp distance p {worst[0]:g} m {worst[1]:g} v {worst[2]:g} (bar {bar})")
        assert max(worst) <= bar, f"{tag}: p / m / v against adam_expect"
        assert_same_bits(p[np_:], before[0][np_:], f"{tag}: the slot behind the parameters")

    def loop(tw, s, x, state):
        """The batches of an epoch writer as single train_step calls on the twin; -> the running loss sum."""
        tp, tm, tv, tacc, tg = state
        run, r0 = float(tacc.item()), 0
        for i, n in enumerate(s.batches):
            tw.train_step(x[r0:r0 + n], tp, tm, tv, s.t + i, s.lr, loss_accum=tacc, grads=tg, **hp(s))
            run += float(tg[-1].item())
            assert float(tacc.item()) == run, f"writer {s.no} twin batch {i}: loss_accum is not the running sum of the loss slots"
            r0 += n
        return run

    for s in co.plan(case):
        tag = f"{case.name} {case.route} writer {s.no} ({s.writer}, rows {s.rows})"
        print(f"  {tag}: t={s.t} lr={s.lr} betas=({s.b1}, {s.b2}) eps={s.eps}; readers at {sorted({r.rows for r in s.readers})}")
        before = (p.clone(), m.clone(), v.clone(), acc.clone(), g.clone())
        old = twin_of(case, h, before[0])                      # (c): the parameters from before the writer
        if s.writer == "load_params":
            p = other_params(p)
            h.load_params(p)
        else:
            x = dev(co.uniform_rows(sum(s.batches), F, 100 * s.no + s.rows), ins.xdt)
            if s.writer == "train_step":
                h.train_step(x, p, m, v, s.t, s.lr, loss_accum=acc, grads=g, **hp(s))
            elif s.writer == "fwd_bwd+adam_step":
                h.fwd_bwd(x, g)
                h.adam_step(p, g, m, v, s.t, s.lr, loss_accum=acc, **hp(s))
            elif s.writer == "fwd_bwd_latent+adam_step":
                h.fwd_bwd_latent(x, dev(co.latent_term(s.rows, Z, F, s.rows), pdt), g)
                h.adam_step(p, g, m, v, s.t, s.lr, loss_accum=acc, **hp(s))
            elif s.writer == "train_epoch":
                assert h.train_epoch(x, s.rows, p, m, v, s.t, s.lr, loss_accum=acc, grads=g, **hp(s)) == len(s.batches)
            else:
                assert s.writer == "train_epoch_dp" and h.comm_world == 0
                h.train_epoch_dp(x, list(s.batches), p, m, v, s.t, s.lr, loss_accum=acc, grads=g, **hp(s))
            if len(s.batches) == 1:                            # (b): the gradient the step used, from a handle that never stepped
                g_old = torch.zeros_like(g)
                if s.writer == "fwd_bwd_latent+adam_step":
                    old.fwd_bwd_latent(x, dev(co.latent_term(s.rows, Z, F, s.rows), pdt), g_old)
                else:
                    old.fwd_bwd(x, g_old)
                assert_same_bits(g, g_old, f"{tag}: the gradient is not that of the parameters the last writer left")
        # (c), first half, and (a)
        live = torch.ones(np_, dtype=torch.bool, device="cuda")
        if case.kind == "fpga" and s.batches:
            # ReLU: a unit that is off on every row has an exactly zero gradient, and so have the weights behind it.  With m = v = 0
            # Adam has nothing to move them by (29 % of this model at its starting weights); they are left out of the count, never
            # more than half of the vector.
            live = (m[:np_] != 0) | (v[:np_] != 0)
            assert float(live.double().mean().item()) > 0.5, f"{tag}: most of the model never saw a gradient"
        moved = float((p[:np_] != before[0][:np_])[live].double().mean().item())
        print(f"    p moved in {100 * moved:.2f} % of its {int(live.sum())} of {np_} elements that a gradient has reached")
        assert moved > 0.99, f"{tag}: the writer left {100 * (1 - moved):.2f} % of p where it was"
        new = twin_of(case, h, p)
        for r in s.readers:
            what = f"{tag} -> {r.kind} rows={r.rows} features={r.features}"
            mine, fresh, stale = read(h, r, ins), read(new, r, ins), read(old, r, ins)
            for k in mine:
                assert_same_bits(mine[k], fresh[k], f"{what}: {k} differs from a fresh handle loaded with the current parameters")
                assert differs(mine[k], stale[k]), f"{what}: {k} is what a handle with the parameters of before the writer gives"
        new.close()
        # (b)
        if len(s.batches) == 1:
            adam_ok(tag, s, s.t, before, g)
            acc_want += float(g[-1].item())
        elif s.batches:
            state = tuple(a.clone() for a in before)           # `old` still holds the parameters from before the writer
            acc_want = loop(old, s, x, state)
            for k, a, b in zip(("params", "m", "v", "loss_accum", "grads"), (p, m, v, acc, g), state):
                assert_same_bits(a, b, f"{tag}: {k} differs from the same batches as single train_step calls")
        assert float(acc.item()) == acc_want, f"{tag}: loss_accum {acc.item()!r} is not the running sum of the loss slots {acc_want!r}"
        old.close()

    # (d) the anchor: eight writers from the formula weights, non-zero moments
    ref.flat = host(p)[:-1]
    x64 = ref.rows(129, co.ANCHOR_SEED)
    assert x64.shape == (129, F), "too few rows off the kink"
    xin = dev(x64, ins.xdt)
    seen = host(xin)
    tag = f"{case.name} {case.route} anchor"
    tmode = "fp32" if cmode in ("fp16", "fp16x3") else cmode      # those two train in exact float32
    z_want = ref.encode(seen)
    r_want = ref.decode(z_want)
    infer_ok(cmode, wide, host(h.encode(xin, out_dtype=ins.xdt)), z_want, ins.xdt, tag + " encode")
    recon, loss = h.forward_loss(xin)
    infer_ok(cmode, wide, host(recon), r_want, ins.xdt, tag + " forward_loss recon")
    lw = float(((r_want - seen) ** 2).sum() * (1.0 if case.kind == "pj" else 1.0 / F))
    lbar = (1e-3 if wide else 2e-2) if cmode == "bf16" else F16_BAR if cmode == "fp16" else TOL[tmode]
    print(f"    oracle {tag} forward_loss: loss {abs(loss.item() - lw) / lw:.3e} (bar {lbar:g})")
    assert abs(loss.item() - lw) <= lbar * lw
    h.fwd_bwd(xin, g)
    lo, go = ref.fwd_bwd(seen)
    grad_ok(tmode, wide, 129, g, lo, go, tag + " fwd_bwd")
