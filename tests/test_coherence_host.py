"""tests/coherence.py proved on the CPU before tests/test_gpu_coherence.py trusts it:
  * adam_expect in float64 agrees with the three reference Adam steps of the suite to 4 ulp of float64 over the plan's own eight
    changes of lr, betas and eps;
  * ulps passes a planted 1-ulp difference and flags a 2-ulp one;
  * every case's plan covers every (writer kind, reader kind) pair and every (writer row class, reader kind, reader row class) triple,
    makes every row class a writer batch, never restarts t and carries the changed hyper-parameters on writers 5 and 6;
  * the Adam bar of the GPU module (1 ulp of float32, 8 ulp of float64) rejects a catalogue of wrong updates on the plan's own
    trajectory: bias correction dropped, eps inside the root, t off by one, the previous step's lr, default betas where the plan
    changes them, and m / v updated from gradient products rounded to float32 (visible where the product nearly cancels m);
  * the anchor's inputs: at the parameters the plan ends on with the oracle as the model (next to the device's own: the two part by
    the rounding of each gradient), 129 rows off the kink exist and plain float32 arithmetic stays within half the family's bar (the
    argument of tests/test_grad_tensors_host.py)."""
import itertools

import numpy as np
import pytest

import coherence as co
import fpga_ref
import grad_tensors as gt
import pjconv_ref
from oracle import c_oracle as orc
from test_gpu_grad_tensors import bar_of, reference_of
from test_gpu_guard_bands import FAMILIES, DenseRef
from test_gpu_parity import rel
from test_gpu_streams import EXTRA

CASES = co.cases(FAMILIES, EXTRA)
IDS = [f"{c.name}-{c.route}" for c in CASES]


def _ae24():
    dims = orc.ae_dims(24, 15)
    return dims, orc.formula_params(dims, 139)


def _ae24_case():
    return next(c for c in CASES if (c.name, c.route) == ("ae24-fp32", "default"))


# ---- the Adam restatement ----------------------------------------------------------------------------------------------------------
def test_adam_expect_agrees_with_the_reference_steps():
    dims, p0 = _ae24()
    x = DenseRef(dims, p0).rows(129, 129)
    steps = [s for s in co.plan(_ae24_case()) if s.batches]
    assert len(steps) == 7 and {(s.lr, s.b1, s.b2, s.eps) for s in steps} == {(1e-3, 0.9, 0.999, 1e-8), (5e-4, 0.9, 0.999, 1e-8), (5e-4, 0.8, 0.99, 1e-6)}
    hps = [(s.t, s.lr, s.b1, s.b2, s.eps) for s in steps] + [(steps[-1].t + 1, steps[-1].lr) + co.CHANGED_HP]      # eight steps, the plan's own t
    assert [a[0] for a in hps] == [1, 2, 3, 4, 7, 8, 11, 12]
    for name, ref_step in (("oracle/c_oracle", orc.adam_step), ("fpga_ref", fpga_ref.adam_step), ("pjconv_ref", pjconv_ref.adam_step)):
        p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
        worst = 0.0
        for t, lr, b1, b2, eps in hps:
            _, g = orc.fwd_bwd(dims, p, x)
            want = co.adam_expect(p, g, m, v, t, lr, b1, b2, eps, np.float64)
            ref_step(p, g, m, v, t, lr, b1, b2, eps)
            for a, b in zip((p, m, v), want):
                worst = max(worst, co.ulps(a, b, np.float64).max())
        print(f"\nadam_expect against {name}: worst {worst:g} ulp of float64 over {len(hps)} steps")
        assert worst <= 4


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ulps_sees_two_and_passes_one(dtype):
    a = np.array([1.0, -1.0, 3e-5, -7.25, 0.0, 1.9999999, 2.0 ** -140 if dtype == np.float32 else 2.0 ** -1060], dtype=dtype)
    up1 = np.nextafter(a, dtype(np.inf))
    up2 = np.nextafter(up1, dtype(np.inf))
    down2 = np.nextafter(np.nextafter(a, dtype(-np.inf)), dtype(-np.inf))
    assert (co.ulps(a, a, dtype) == 0).all()
    assert (co.ulps(a, up1, dtype) == 1).all() and (co.ulps(up1, a, dtype) == 1).all()
    assert (co.ulps(a, up2, dtype) == 2).all() and (co.ulps(a, down2, dtype) == 2).all()
    assert co.ulps(dtype(0.0), dtype(-0.0), dtype) == 0
    assert co.ulps(np.array([-1.0]), np.array([1.0]), dtype)[0] > 2.0 ** (24 if dtype == np.float32 else 53)
    assert np.isinf(co.ulps(np.array([np.nan, 1.0]), np.array([1.0, np.nan]), dtype)).all()
    bar = co.adam_bar(dtype)
    assert (co.ulps(a, up1, dtype) <= bar).all()
    far = a
    for _ in range(bar + 1):
        far = np.nextafter(far, dtype(np.inf))
    assert (co.ulps(a, far, dtype) > bar).all()


# ---- plan coverage -----------------------------------------------------------------------------------------------------------------
def test_cases_are_the_training_cases_and_the_extra_families():
    assert [(c.name, c.route) for c in CASES] == [(f, r) for f, v in FAMILIES.items() for r in v[6]] + [(f, "default") for f in EXTRA]
    for c in CASES:
        assert 2 <= len(c.classes) <= 4 and list(c.classes) == sorted(set(c.classes))
        assert max(c.classes) <= 8193 or c.name.split("-")[0] in ("ae24", "class40", "class100", "fpga")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_plan_coverage(case):
    steps = co.plan(case)
    kinds = set(co.reader_kinds(case))
    assert [s.no for s in steps if s.no != 6] == [1, 2, 3, 4, 5, 7, 8] and [s.no for s in steps] == sorted(s.no for s in steps)
    # every (writer kind, reader kind) pair
    for s in steps:
        assert {r.kind for r in s.readers} == kinds, f"writer {s.no}"
        assert len({r.rows for r in s.readers}) >= 2 and sum(r.features for r in s.readers) == 1
    assert {s.writer for s in steps} >= {"train_step", "fwd_bwd+adam_step", "load_params", "train_epoch", "train_epoch_dp"}
    assert ("fwd_bwd_latent+adam_step" in {s.writer for s in steps}) == case.latent
    assert {k for s in steps for r in s.readers if r.features for k in [r.kind]} == set(co.FEATURE_KINDS) & kinds
    # every (writer row class, reader kind, reader row class) triple; every row class a writer batch
    have = {(s.rows, r.kind, r.rows) for s in steps for r in s.readers if s.rows is not None}
    assert have >= set(itertools.product(case.classes, kinds, case.classes))
    assert {n for s in steps for n in s.batches} >= set(case.classes)
    assert {r.rows for s in steps if s.rows is None for r in s.readers} <= set(case.classes)
    # the first call after a writer: every reader kind once, and the four of FIRST_AT_LARGEST at the largest class behind a writer that stepped
    assert {s.readers[0].kind for s in steps} == kinds
    big = case.classes[-1]
    for q in set(co.FIRST_AT_LARGEST) & kinds:
        assert [s.no for s in steps if s.batches and s.readers[0][:2] == (q, big)], f"{q} never leads at {big} rows"
    assert all(len(s.readers) == len(set(s.readers)) for s in steps)
    # t strictly increasing, never restarting
    ts = [s.t + i for s in steps for i in range(len(s.batches))]
    assert ts == list(range(1, len(ts) + 1))
    # the changed hyper-parameters
    s5 = [s for s in steps if s.no == 5]
    s6 = [s for s in steps if s.no == 6]
    assert len(s5) == 1 and s5[0].lr == 5e-4 and s5[0].batches == (case.classes[0], case.classes[0], 1)
    assert s6 and all((s.lr, s.b1, s.b2, s.eps) == (5e-4, 0.8, 0.99, 1e-6) for s in s6)
    assert {s.rows for s in s6} == (set(case.classes[1:-1]) or {case.classes[-1]})
    assert all(s.lr == (1e-3 if s.no < 5 else 5e-4) for s in steps)
    assert all((s.b1, s.b2, s.eps) == (0.9, 0.999, 1e-8) for s in steps if s.no != 6)
    s7 = [s for s in steps if s.no == 7][0]
    assert s7.batches == (case.classes[0], 1, case.classes[0])


# ---- power of the Adam bar ---------------------------------------------------------------------------------------------------------
def _scalars(t, lr, b1, b2):
    return lr / (1.0 - b1 ** float(t)), np.sqrt(1.0 - b2 ** float(t))


def _update(p, g, m, v, step_size, bc2_sqrt, b1, b2, eps, dtype, eps_inside=False, rounded_products=False):
    rnd = (lambda a: a.astype(np.float32).astype(np.float64)) if rounded_products else (lambda a: a)
    m = m + rnd((g - m) * (1.0 - b1))
    v = v * b2 + rnd((1.0 - b2) * g * g)
    denom = np.sqrt(v / bc2_sqrt ** 2 + eps) if eps_inside else np.sqrt(v) / bc2_sqrt + eps
    p = p - step_size * (m / denom)
    return tuple(a.astype(dtype).astype(np.float64) for a in (p, m, v))


def _wrong_updates(dtype):
    """name -> update(step, previous step or None, t, p, g, m, v) -> (p, m, v)"""
    def no_bias_correction(s, prev, t, p, g, m, v):
        return _update(p, g, m, v, s.lr, 1.0, s.b1, s.b2, s.eps, dtype)

    def eps_inside_the_root(s, prev, t, p, g, m, v):
        return _update(p, g, m, v, *_scalars(t, s.lr, s.b1, s.b2), s.b1, s.b2, s.eps, dtype, eps_inside=True)

    def t_off_by_one(s, prev, t, p, g, m, v):
        return _update(p, g, m, v, *_scalars(t + 1, s.lr, s.b1, s.b2), s.b1, s.b2, s.eps, dtype)

    def lr_of_the_previous_step(s, prev, t, p, g, m, v):
        return _update(p, g, m, v, *_scalars(t, (prev or s).lr, s.b1, s.b2), s.b1, s.b2, s.eps, dtype)

    def default_betas(s, prev, t, p, g, m, v):
        b1, b2, _ = co.DEFAULT_HP
        return _update(p, g, m, v, *_scalars(t, s.lr, b1, b2), b1, b2, s.eps, dtype)

    def rounded_products(s, prev, t, p, g, m, v):
        """m and v updated from the gradient products rounded to float32 instead of the float64 ones: where the product nearly cancels
        m, the half unit it is off by is many units of the sum."""
        return _update(p, g, m, v, *_scalars(t, s.lr, s.b1, s.b2), s.b1, s.b2, s.eps, dtype, rounded_products=True)
    return {f.__name__: f for f in (no_bias_correction, eps_inside_the_root, t_off_by_one, lr_of_the_previous_step, default_betas,
                                    rounded_products)}


def _trajectory(dtype, updates):
    """Walk the ae24 plan with the oracle as the model; -> {name: worst ulp distance from adam_expect over the steps, on p / m / v}."""
    dims, p0 = _ae24()
    case = _ae24_case()
    worst = {k: np.zeros(3) for k in updates}
    prev = [None]

    def on_step(s, t, p, g, m, v):
        want = co.adam_expect(p, g, m, v, t, s.lr, s.b1, s.b2, s.eps, dtype)
        for k, f in updates.items():
            got = f(s, prev[0], t, p, g, m, v)
            worst[k] = np.maximum(worst[k], [co.ulps(a, b, dtype).max() for a, b in zip(got, want)])
        prev[0] = s

    def model(p, x, lg):
        return DenseRef(dims, p).fwd_bwd(x, lg)
    co.walk(case, 24, 15, p0, dtype, model, on_step)
    return worst


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_adam_bar_rejects_the_wrong_updates(dtype):
    bar = co.adam_bar(dtype)
    for name, w in _trajectory(dtype, _wrong_updates(dtype)).items():
        print(f"\n{np.dtype(dtype).name} {name}: worst ulp distance p {w[0]:g} m {w[1]:g} v {w[2]:g} (bar {bar})")
        assert w.max() > bar, f"{name}: the bar of {bar} ulp does not see it"


# ---- the anchor's inputs -----------------------------------------------------------------------------------------------------------
ANCHOR = [c for c in CASES if c.kind in ("dense", "dims") and c.mode in ("fp32", "fp64") and c.name in FAMILIES
          and reference_of(c.name).dims[0] <= 100]
ANCHOR = list({(c.name, c.classes): c for c in ANCHOR}.values())         # the routings that share row classes share the walk


@pytest.mark.parametrize("case", ANCHOR, ids=[f"{c.name}-{'-'.join(map(str, c.classes))}" for c in ANCHOR])
def test_anchor_inputs(case):
    ref0 = reference_of(case.name)
    dims, bar = list(ref0.dims), bar_of(case.name)
    dt = np.float64 if case.mode == "fp64" else np.float32
    Z = dims[(len(dims) - 1) // 2]
    p, _, _ = co.walk(case, dims[0], Z, ref0.flat, dt, lambda p, x, lg: DenseRef(dims, p).fwd_bwd(x, lg))
    ref = DenseRef(dims, p)
    x = ref.rows(129, co.ANCHOR_SEED)                               # asserts that it found 129 rows off the kink
    assert x.shape == (129, dims[0])
    x = x.astype(dt).astype(np.float64)
    lo, go = ref.fwd_bwd(x)
    l32, g32 = gt.fwd_bwd_np(dims, p, x, dt)
    gerr, lerr = rel(g32, go), abs(float(l32) - lo) / lo
    L = len(dims) - 1
    z = x.astype(dt)
    sl = gt.tensor_slices(dims, names=False)
    for l in range(L):
        W, b = p[sl[2 * l]].reshape(dims[l + 1], dims[l]).astype(dt), p[sl[2 * l + 1]].astype(dt)
        z = z @ W.T + b
        if l not in (L // 2 - 1, L - 1):
            z = np.where(z > 0, z, dt(0.01) * z)
        if l == L // 2 - 1:
            zerr = rel(z, ref.encode(x))
    rerr = rel(z, ref.decode(ref.encode(x)))
    print(f"\n{case.name} {case.classes}: {np.dtype(dt).name} NumPy at the plan's final parameters: gradient {gerr:.3e} loss {lerr:.3e} "
          f"codes {zerr:.3e} reconstruction {rerr:.3e} (half the bar: {bar / 2:g})")
    assert max(gerr, lerr, zerr, rerr) <= bar / 2
