"""Coherence of a handle's weight copies: the plan of writers and readers, and the Adam step restated.  TEST INFRASTRUCTURE, NumPy and
plain Python only (tests/test_coherence_host.py proves it on the CPU, tests/test_gpu_coherence.py walks it on the GPU).

A handle keeps the model's weights in up to five device copies ("Coherence of the weight copies"), every one of which has to
follow every way the parameters can change.  Which writer runs, and which copy the next call reads, depends on the batch's row count.
`plan(case)` is one deterministic sequence of writers on ONE long-lived handle, each followed by every reader kind at two row classes;
the caller-side state (p, m, v, t, lr) is never reset.

Writers (Step.no):
  1  train_step on the smallest row class                                  t = 1, lr 1e-3, default betas / eps
  2  fwd_bwd on the largest row class, then adam_step                      next t
  3  train_step on the largest row class                                   next t
  4  load_params(other), other = roll(p, 7) * 0.9; m, v, t kept
  5  train_epoch over 2 bs + 1 rows, bs = the smallest row class           three steps (bs, bs, 1 rows); lr 5e-4 from here on
  6  train_step on every remaining row class in turn                       betas (0.8, 0.99), eps 1e-6
     (a family with two row classes has none left: there the largest one, so that the hyper-parameters are always carried)
  7  train_epoch_dp, batch_rows [bs, 1, bs], no communicator               default betas / eps again
  8  fwd_bwd_latent on the second row class, then adam_step                next t (PJ_Conv_AE: plain fwd_bwd)

Readers after every writer: encode (into float32 and into float64 at every reader row class), encode16 (float16 codes), decode (of
float32 / float64 codes and of float16 codes), forward_loss, fwd_bwd, fwd_bwd_latent (every family but PJ_Conv_AE), activation_means (the
dense LeakyReLU families).  One reader kind per step takes raw rows with `features`.  The two reader row classes rotate over the
consecutive pairs of the case's row classes; where that rotation leaves a (writer row class, reader row class) pair out -- a middle
class of the four-class families is a writer batch only twice -- the last step written on that class reads at the missing classes too.

The FIRST call after a writer is the one that meets the stale flags (wb_stale, packed_stale, infer16_stale ... are each tested at several
entry points, and whichever call comes first re-packs and clears them), so the reader that leads a step rotates: every reader kind leads
at least once per case, and decode, forward_loss, fwd_bwd and fwd_bwd_latent (FIRST_AT_LARGEST) each lead once at the LARGEST row class
straight after a writer that stepped -- the large-batch forward / backward launches are where a training step of that size reads the
lazily re-made copies.  Where too few stepping writers have the largest class among their readers, the next ones read there as well.

Row classes: one per launch route the family's dispatch distinguishes under the case's knobs (README's knob table):
  ae24-fp32, class40-fp32, default knobs     129 (4-row chain), 4099 (16-row small-batch kernels: above BALER_AMD_LAT4_ROWS = 2048, below
                                             BALER_AMD_LATENCY_ROWS = 12288), 16449 (throughput pair with the tail hand-off)
  the same, pair / lat4-0 routings           129, 513 (the knob sends every batch to one kernel; two sizes of it)
  ae24-fp64, class40-fp64, fpga-fp64         129 (4-row chain, up to BALER_AMD_F64_QCHAIN_BLKS = 96 blocks), 2049 (exchange chain), 16449
                                             (register chain from BALER_AMD_F64_REGCHAIN_BLKS = 1024 blocks), under each fp64 routing
  ae24-bf16, ae24z8-bf16                     129 (fp32 small-batch kernels, up to BALER_AMD_BF16_SMALL_ROWS = 3072), 4099 (bf16 training
                                             pair); bf16-small0: 129, 513
  class100-fp32                              129, 513 (small-batch class), 16449 (large pass on the wide class; class-chunk64: chunks of 64
                                             rows from 33 rows on; mid-hybrid0: the small-batch class alone)
  wide fp32 and bf16 (cfd625, cfd2500,       60 (one-launch dW + Adam on 16-row tiles), 513 (64-row groups: above BALER_AMD_WIDE_IN16_ROWS),
  wide512, wideclass300)                     769 (per-layer dW launches and adam_k: above BALER_AMD_DW_SMALL_ROWS = 768); wide512-* and
                                             cfd625-bf16 also 8193 (past BALER_AMD_WIDE_SMALL_ROWS = 8192)
  layerwise-*                                60, 769, 1025 (either side of BALER_AMD_DW_SMALL_ROWS = 768 and BALER_AMD_GEMM_SMALL_ROWS = 1024)
  fpga-fp32                                  129, 8193 (either side of the slab kernels' 8,192-row switch)
  pjconv-z10                                 65, 4097
  cfd625-fp64, ae24-fp16, ae24-fp16x3        60, 513 (training routing default)
"""
import collections

import numpy as np

Step = collections.namedtuple("Step", "no writer rows batches t lr b1 b2 eps readers")
Reader = collections.namedtuple("Reader", "kind rows features")
Case = collections.namedtuple("Case", "name route kind mode classes latent act_means")

DEFAULT_HP = (0.9, 0.999, 1e-8)
CHANGED_HP = (0.8, 0.99, 1e-6)
LR0, LR1 = 1e-3, 5e-4
ANCHOR_SEED = 5129                                                              # the anchor's 129 rows off the kink
FEATURE_KINDS = ("encode", "forward_loss", "fwd_bwd", "activation_means")       # the readers that take rows
FIRST_AT_LARGEST = ("decode", "forward_loss", "fwd_bwd", "fwd_bwd_latent")      # each leads a step once, at the largest row class


def row_classes(name, route, spec, extra=False):
    """The row classes of a (family, training routing): the table of the module docstring.  spec: the FAMILIES entry."""
    kind, F, _, mode, env = spec[:5]
    if extra:
        return (60, 513)
    if kind == "pj":
        return (65, 4097)
    if kind == "fpga":
        return (129, 2049, 16449) if mode == "fp64" else (129, 8193)
    if kind == "dims" or env:
        return (60, 769, 1025)
    if F > 127:
        return (60, 513, 769) + ((8193,) if name.startswith("wide512-") or name == "cfd625-bf16" else ())
    if F > 63:
        return (129, 513, 16449)
    if mode == "fp64":
        return (129, 2049, 16449)
    if mode == "bf16":
        return (129, 4099) if route == "default" else (129, 513)
    return (129, 4099, 16449) if route == "default" else (129, 513)


def case_of(name, route, spec, extra=False):
    kind = spec[0]
    return Case(name, route, kind, spec[3], row_classes(name, route, spec, extra), kind != "pj", kind in ("dense", "dims"))


def cases(families, extra):
    """Every (family, training routing) of FAMILIES plus the EXTRA families of the streams module (training routing default)."""
    out = [case_of(f, r, v) for f, v in families.items() for r in v[6]]
    return out + [case_of(f, "default", v, extra=True) for f, v in extra.items()]


def reader_kinds(case):
    return (("encode", "encode16", "decode", "forward_loss", "fwd_bwd") + (("fwd_bwd_latent",) if case.latent else ())
            + (("activation_means",) if case.act_means else ()))


def plan(case):
    """[Step]: the writers of the module docstring in order (writer 6 is one Step per row class), each with its readers."""
    c = case.classes
    small, big = c[0], c[-1]
    rest = c[1:-1] or (big,)
    raw, t = [], 1

    def add(no, writer, rows, batches, lr, hp=DEFAULT_HP):
        nonlocal t
        raw.append((no, writer, rows, tuple(batches), t if batches else None, lr) + tuple(hp))
        t += len(batches)

    add(1, "train_step", small, [small], LR0)
    add(2, "fwd_bwd+adam_step", big, [big], LR0)
    add(3, "train_step", big, [big], LR0)
    add(4, "load_params", None, [], LR0)
    add(5, "train_epoch", small, [small, small, 1], LR1)
    for n in rest:
        add(6, "train_step", n, [n], LR1, CHANGED_HP)
    add(7, "train_epoch_dp", small, [small, 1, small], LR1)
    add(8, "fwd_bwd_latent+adam_step" if case.latent else "fwd_bwd+adam_step", c[1], [c[1]], LR1)

    k = len(c)
    at = [list(dict.fromkeys((c[j % k], c[(j + 1) % k]))) for j in range(len(raw))]
    for w in c:                                                   # the pairs the rotation left out
        mine = [j for j, r in enumerate(raw) if r[2] == w]
        seen = {n for j in mine for n in at[j]}
        at[mine[-1]] += [n for n in c if n not in seen]
    kinds = reader_kinds(case)
    # the reader that leads each step (module docstring)
    steppers = [j for j, r in enumerate(raw) if r[3]]
    pool = [j for j in steppers if big in at[j]] + [j for j in steppers if big not in at[j]]
    at_largest = [q for q in FIRST_AT_LARGEST if q in kinds]
    lead = {}
    for q, j in zip(at_largest, pool):
        lead[j] = (q, big)
        if big not in at[j]:
            at[j].append(big)
    others = [q for q in kinds if q not in at_largest] + at_largest
    for i, j in enumerate(j for j in range(len(raw)) if j not in lead):
        lead[j] = (others[i % len(others)], at[j][0])
    takes_rows = [q for q in FEATURE_KINDS if q in kinds]
    steps = []
    for j, r in enumerate(raw):
        with_features = takes_rows[j % len(takes_rows)]
        readers = [Reader(q, n, q == with_features and i == 0) for i, n in enumerate(at[j]) for q in kinds]
        first = next(x for x in readers if (x.kind, x.rows) == lead[j])
        steps.append(Step(*r, [first] + [x for x in readers if x is not first]))
    return steps


def uniform_rows(n, F, seed):
    """Plain uniform rows (the bitwise checks need no kink care: both sides run the same kernels)."""
    return np.random.default_rng(seed).random((n, F))


def latent_term(n, Z, F, seed):
    """The latent term of training_calls (tests/test_gpu_guard_bands.py): N(0, 1) * 0.01 * 24 / F."""
    return np.random.default_rng(seed).normal(size=(n, Z)) * (0.01 * 24 / F)


def other_params(p, dtype=np.float64):
    """other_params of tests/test_gpu_streams.py on a NumPy vector (the handle's vector with its trailing slot), multiplied in `dtype`."""
    return (np.roll(p, 7).astype(dtype) * np.dtype(dtype).type(0.9)).astype(np.float64)


# ---- Adam, restated --------------------------------------------------------------------------------------------------------------
def adam_expect(p, g, m, v, t, lr, b1, b2, eps, dtype):
    """adam_scalars / adam_update of baler_amd/csrc/bamd_internal.hpp in float64 NumPy: the same operations in the same order, p, m and v
    each rounded to `dtype` once.  -> (p, m, v) as float64 arrays holding `dtype` values."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    bc1 = 1.0 - b1 ** float(t)
    bc2 = 1.0 - b2 ** float(t)
    step_size, bc2_sqrt = lr / bc1, np.sqrt(bc2)
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * g * g
    denom = np.sqrt(v) / bc2_sqrt + eps
    p = p - step_size * (m / denom)
    return tuple(a.astype(dtype).astype(np.float64) for a in (p, m, v))


def ulps(a, b, dtype):
    """Elementwise distance of a and b in units in the last place of `dtype` (both are rounded to it first): the number of
    representable values between them, +0 and -0 counting as one value.  A NaN on either side: the largest distance."""
    dt = np.dtype(dtype)
    ut = {4: np.uint32, 8: np.uint64}[dt.itemsize]
    a, b = np.asarray(a).astype(dt), np.asarray(b).astype(dt)
    top = ut(1) << ut(8 * dt.itemsize - 1)

    def key(x):                                   # monotonic in the value: negatives below `top` in reverse, positives above
        bits = np.ascontiguousarray(x).view(ut)
        return np.where(bits & top, top - (bits & ~top), bits | top)
    ka, kb = key(a), key(b)
    d = np.where(ka > kb, ka - kb, kb - ka).astype(np.float64)
    return np.where(np.isnan(a) | np.isnan(b), np.inf, d)


ULP_BAR = {np.dtype(np.float32): 1, np.dtype(np.float64): 8}


def adam_bar(dtype):
    """What test (b) allows between the device and adam_expect: 1 ulp of float32 (both sides round one float64 result once), 8 ulp of
    float64 (what ten float64 operations and the host's pow can differ by)."""
    return ULP_BAR[np.dtype(dtype)]


def walk(case, F, Z, p0, dtype, fwd_bwd, on_step=None):
    """The plan with a host model in place of the handle: fwd_bwd(p, x, latent_grad or None) -> (loss, gradient).  State rounded to
    `dtype` as the device keeps it; writer 4 rolls the vector WITH the slot behind the parameters, as the GPU test does.  The gradients
    are the host model's, so this is the trajectory next to the device's (they part by the rounding of each gradient), not the device's
    own.  on_step(step, t, p, g, m, v) sees every Adam step's inputs.  -> final (p, m, v)."""
    p = np.asarray(p0, dtype=np.float64).astype(dtype).astype(np.float64)
    m, v, slot = np.zeros_like(p), np.zeros_like(p), 0.0
    for s in plan(case):
        if s.writer == "load_params":
            e = other_params(np.append(p, slot), dtype)
            p, slot = e[:-1].copy(), e[-1]
            continue
        x, r0 = uniform_rows(sum(s.batches), F, 100 * s.no + s.rows), 0
        for i, n in enumerate(s.batches):
            lg = latent_term(n, Z, F, n).astype(dtype).astype(np.float64) if s.writer.startswith("fwd_bwd_latent") else None
            xb = x[r0:r0 + n].astype(dtype).astype(np.float64)
            r0 += n
            _, g = fwd_bwd(p, xb, lg)
            g = np.asarray(g).astype(dtype).astype(np.float64)
            if on_step:
                on_step(s, s.t + i, p, g, m, v)
            p, m, v = adam_expect(p, g, m, v, s.t + i, s.lr, s.b1, s.b2, s.eps, dtype)
    return p, m, v
