"""Gradients held tensor by tensor.  TEST INFRASTRUCTURE, a plain module without fixtures.

`rel()` of tests/test_gpu_parity.py on the whole flat gradient sees only the decoder: in AE(24, 15) en1.weight carries 2e-4 of the
vector's maximum and 6e-4 of its norm, so a 1e-5 bar on the vector is a 2 .. 5 % bar on that tensor -- the one at the end of the
backward chain, where a wrong ragged tail, a wrong mask or a dropped row ends up.  Here every tensor is measured against its OWN norm
and its OWN maximum; tests/test_grad_tensors_host.py proves on the CPU that this sees what the whole-vector bar does not.

`fwd_bwd_np` is the dense forward / loss / backward in NumPy at float32 or float64.  The float64 form restates oracle/c_oracle and
tests/fpga_ref.py (with the latent term the former lacks); the float32 form only shows what plain float32 arithmetic costs per tensor.
It is never a reference for the kernels."""
import numpy as np

import bf16_ref

NAMES_AE = ("en1", "en2", "en3", "en4", "de1", "de2", "de3", "de4")


def tensor_slices(dims, names=True):
    """[(name, slice)] of the 2 L tensors of a flat parameter / gradient vector (the layout of bf16_ref.tensor_slices): en1.weight ..
    de4.bias for the 9-entry topologies, L{l}.weight / L{l}.bias otherwise.  names=False: the slices alone."""
    sl = [s for _, s in bf16_ref.tensor_slices(dims)]
    if not names:
        return sl
    L = len(dims) - 1
    layer = NAMES_AE if L == 8 else [f"L{l}" for l in range(L)]
    return [(f"{layer[t // 2]}.{'bias' if t % 2 else 'weight'}", s) for t, s in enumerate(sl)]


def per_tensor(got, want, dims):
    """[(name, rel_l2, maxerr)]: |got - want|_2 / |want|_2 and max|got - want| / max|want| of every tensor, each against that tensor's
    own norm and own maximum.  A zero-size tensor is skipped.  A reference tensor whose norm is exactly 0 asks for exact zeros: both
    errors are 0.0 then, or inf."""
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    slices = tensor_slices(dims)
    assert got.size == want.size == slices[-1][1].stop, (got.size, want.size, slices[-1][1].stop)
    out = []
    for name, s in slices:
        g, w = got[s], want[s]
        if w.size == 0:
            continue
        nw = np.linalg.norm(w)
        if nw == 0.0:
            e = 0.0 if not g.any() else np.inf
            out.append((name, e, e))
        else:
            d = g - w
            out.append((name, float(np.linalg.norm(d) / nw), float(np.max(np.abs(d)) / np.max(np.abs(w)))))
    return out


def worst(errs):
    """(name, error) of the tensor with the largest max(rel_l2, maxerr); a NaN counts as the largest."""
    key = lambda e: np.inf if np.isnan(e[1]) or np.isnan(e[2]) else max(e[1], e[2])      # noqa: E731
    name, l2, mx = max(errs, key=key)
    return name, (np.nan if np.isnan(l2) or np.isnan(mx) else max(l2, mx))


def assert_per_tensor(got, want, dims, bar, what):
    """Every tensor's max(rel_l2, maxerr) <= bar.  Prints the worst tensor and its error; the message names the failing tensors."""
    errs = per_tensor(got, want, dims)
    name, err = worst(errs)
    print(f"    per tensor {what}: worst {name} {err:.3e} (bar {bar:g})")
    bad = [f"{n}: rel-L2 {l2:.3e} max-norm {mx:.3e}" for n, l2, mx in errs if not (l2 <= bar and mx <= bar)]
    assert not bad, f"{what}: above the bar of {bar:g} on its own scale: " + "; ".join(bad)
    return name, err


def fwd_bwd_np(dims, flat, x, dtype, act="leaky", latent_grad=None):
    """(loss, flat gradient) of loss = sum((r - x)^2) / n_features for the dense autoencoder of any even layer count, every operand
    and every intermediate in `dtype`.  Layers L/2 - 1 and L - 1 are linear; the others LeakyReLU(0.01) ("leaky": slope by the sign
    of the pre-activation) or ReLU ("relu": torch's rule, the gradient passes where the output is > 0).  latent_grad (rows, z) is added
    to dL/dz at the bottleneck."""
    assert act in ("leaky", "relu")
    dt = np.dtype(dtype).type
    L = len(dims) - 1
    assert L % 2 == 0
    lin = (L // 2 - 1, L - 1)
    flat, x = np.asarray(flat).astype(dt), np.ascontiguousarray(np.asarray(x).astype(dt))
    sl = tensor_slices(dims, names=False)
    lay = [(flat[sl[2 * l]].reshape(dims[l + 1], dims[l]), flat[sl[2 * l + 1]]) for l in range(L)]
    slope = dt(0.01 if act == "leaky" else 0.0)
    ys, pre = [x], []
    for l, (W, b) in enumerate(lay):
        a = ys[-1] @ W.T + b
        pre.append(a)
        ys.append(a if l in lin else np.where(a > 0, a, slope * a))
    e = ys[-1] - x
    loss = (e * e).sum(dtype=dt) / dt(dims[0])
    dz, g = e * (dt(2.0) / dt(dims[0])), [None] * L
    for l in range(L - 1, -1, -1):
        if l not in lin:
            dz = np.where(pre[l] > 0, dz, slope * dz)
        if l == L // 2 - 1 and latent_grad is not None:
            dz = dz + np.asarray(latent_grad).astype(dt)
        g[l] = np.concatenate([(dz.T @ ys[l]).ravel(), dz.sum(axis=0, dtype=dt)])
        dz = dz @ lay[l][0]
    out = np.concatenate(g)
    assert out.dtype == dt and loss.dtype == dt
    return loss, out
