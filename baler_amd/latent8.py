"""8-bit latent codes, host side: the rounding rule of BAMD_U8 stated in NumPy, and the per-column scale FOLDED INTO THE MODEL.

The library stores a float32 latent as a byte by rounding it to the nearest integer in [0, 255] and widens a byte exactly
(include/baler_amd.h, bamd_code8); it knows nothing about a scale.  A latent column k with calibrated extrema lo_k, lo_k + rng_k
reaches [0, 255] through c = (z - lo) * s with s_k = 255 / rng_k (1 where rng_k is not positive).  No activation follows the last
encoder layer of any served model, and none precedes the first decoder layer, so that map is exact algebra on two tensors each:

    last encoder layer  (W_e [z, in],  b_e):   W_e' = diag(s) W_e        b_e' = s * (b_e - lo)
    first decoder layer (W_d [out, z], b_d):   W_d' = W_d diag(1 / s)    b_d' = b_d + W_d lo

encode' (x) = (encode(x) - lo) * s and decode'(c) = decode(c / s + lo).  The fold is evaluated in float64 and rounded ONCE to the
model's parameter type; it returns a copy -- the model file on disk is never touched, the folded vector lives in the handle of one
compress or decompress run (``model.load_flat(fold(model, lo, rng))``).
"""
import numpy as np


def q8(v):
    """The store rule: float32(v) -> rint (half to even, in float32) -> clamp to [0, 255] -> uint8.  NaN and -inf give 0, +inf 255."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.asarray(v).astype(np.float32))
        r = np.where(r > 0, r, np.float32(0))          # NaN fails the comparison: 0
        r = np.where(r < 255, r, np.float32(255))
        return r.astype(np.uint8)


def widen8(q):
    """The load rule: a byte is the float32 of its value (exact)."""
    q = np.asarray(q)
    if q.dtype != np.uint8:
        raise ValueError(f"8-bit latent codes are uint8, got {q.dtype}")
    return q.astype(np.float32)


def scale_of(rng):
    """s_k = 255 / rng_k where rng_k > 0, else 1 (a constant latent column: every code is 0 and decodes to lo_k)."""
    rng = np.asarray(rng, dtype=np.float64)
    s = np.ones_like(rng)
    np.divide(255.0, rng, out=s, where=rng > 0)
    return s


def latent_tensors(layout):
    """(weight entry, bias entry) of the last encoder layer and of the first decoder layer in a model's tensor layout
    [(key, offset, shape)]: encoder.5 / decoder.0 of PJ_Conv_AE, layers L/2 - 1 and L/2 of the dense models (tensor_layout)."""
    by_key = {key: (key, off, shape) for key, off, shape in layout}
    if "encoder.5.weight" in by_key:
        return ((by_key["encoder.5.weight"], by_key["encoder.5.bias"]), (by_key["decoder.0.weight"], by_key["decoder.0.bias"]))
    n_layers = len(layout) // 2
    e, d = n_layers // 2 - 1, n_layers // 2
    return (layout[2 * e], layout[2 * e + 1]), (layout[2 * d], layout[2 * d + 1])


def fold_flat(flat, layout, lo, rng):
    """The fold on a flat parameter vector (any float array; the result is float64, NOT yet rounded): a copy with the four
    tensors of ``latent_tensors(layout)`` replaced."""
    out = np.array(flat, dtype=np.float64, copy=True)
    lo = np.asarray(lo, dtype=np.float64).reshape(-1)
    s = scale_of(np.asarray(rng, dtype=np.float64).reshape(-1))
    (we, be), (wd, bd) = latent_tensors(layout)
    z = we[2][0]
    if lo.shape != (z,) or s.shape != (z,) or wd[2][1] != z:
        raise ValueError(f"latent scale of {lo.shape[0]} columns for a model with {z} latent columns")
    n_we, n_wd = int(np.prod(we[2])), int(np.prod(wd[2]))
    w_e = out[we[1]:we[1] + n_we].reshape(we[2]).copy()
    b_e = out[be[1]:be[1] + z].copy()
    w_d = out[wd[1]:wd[1] + n_wd].reshape(wd[2]).copy()
    b_d = out[bd[1]:bd[1] + wd[2][0]].copy()
    out[we[1]:we[1] + n_we] = (s[:, None] * w_e).reshape(-1)
    out[be[1]:be[1] + z] = s * (b_e - lo)
    out[wd[1]:wd[1] + n_wd] = (w_d / s[None, :]).reshape(-1)
    out[bd[1]:bd[1] + wd[2][0]] = b_d + w_d @ lo
    return out


def fold(model, lo, rng):
    """A COPY of ``model``'s flat parameters (numpy, the model's parameter type, ``model.nparams`` long) with the latent scale
    folded in; ``model`` itself is not changed.  lo, rng: (z,) float64, the calibrated minimum and range of every latent column."""
    flat = model.flat[: model.nparams].detach().to("cpu").numpy()
    return fold_flat(flat, model.layout, lo, rng).astype(flat.dtype)


def unscale(codes, lo, rng):
    """The latent a code stands for: q / s + lo (float64)."""
    return widen8(codes).astype(np.float64) / scale_of(rng) + np.asarray(lo, dtype=np.float64)
