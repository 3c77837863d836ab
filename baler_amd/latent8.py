"""8-bit and packed sub-byte latent codes, host side: the rounding rule of BAMD_U8 / BAMD_U1 .. BAMD_U7 and the bit layout of packed
rows stated in NumPy, and the per-column scale FOLDED INTO THE MODEL.  The text below speaks of bytes and 255; b-bit codes are the
same with ``levels(b)`` = 2**b - 1 in the place of 255 (the ``levels`` arguments) plus pack_rows / unpack_rows.

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


def levels(bits):
    """The largest code of ``bits`` bits, 2**bits - 1 (bits = 1 .. 8): the value a column's calibrated maximum is mapped to."""
    bits = int(bits)
    if not 1 <= bits <= 8:
        raise ValueError(f"latent codes have 1 to 8 bits, got {bits}")
    return 2 ** bits - 1


def row_bytes(z, bits):
    """Bytes of one packed row of z codes of ``bits`` bits: ceil(z * bits / 8) -- rows are byte-aligned."""
    return (int(z) * int(bits) + 7) // 8


def qb(v, bits):
    """The store rule of b-bit codes (include/baler_amd.h, bamd_codeb): q8 with 2**bits - 1 in the place of 255; qb(v, 8) is q8(v).
    -> uint8, one code per element, NOT yet packed."""
    top = np.float32(levels(bits))
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.asarray(v).astype(np.float32))
        r = np.where(r > 0, r, np.float32(0))          # NaN fails the comparison: 0
        r = np.where(r < top, r, top)
        return r.astype(np.uint8)


def pack_rows(q, bits):
    """Codes (n, z), each below 2**bits -> packed rows, uint8 (n, ceil(z * bits / 8)).  Code k of a row occupies bits
    [k * bits, (k + 1) * bits) of the row's bit string; bit i of a row is bit i % 8 of its byte i // 8; the unused high bits of the
    last byte are zero.  Written from that rule: every code is shifted to its place and its (at most two) bytes are OR-ed in."""
    q = np.asarray(q)
    bits = int(bits)
    if q.ndim != 2 or q.dtype != np.uint8 or not 1 <= bits <= 8 or (q.size and int(q.max()) > levels(bits)):
        raise ValueError(f"pack_rows: uint8 codes of shape (n, z) below 2**{bits} expected")
    n, z = q.shape
    out = np.zeros((n, row_bytes(z, bits) + 1), dtype=np.uint8)      # (one spare byte takes the empty high half of the last code)
    start = np.arange(z) * bits
    byte, sh = start // 8, start % 8
    for k in range(z):
        w = q[:, k].astype(np.uint16) << np.uint16(sh[k])
        out[:, byte[k]] |= (w & 0xFF).astype(np.uint8)
        out[:, byte[k] + 1] |= (w >> np.uint16(8)).astype(np.uint8)
    return np.ascontiguousarray(out[:, :-1])


def unpack_rows(data, z, bits):
    """Packed rows, uint8 (n, ceil(z * bits / 8)) -> codes, uint8 (n, z); the padding bits of the last byte are ignored."""
    data = np.asarray(data)
    z, bits = int(z), int(bits)
    if data.ndim != 2 or data.dtype != np.uint8 or not 1 <= bits <= 8 or data.shape[1] != row_bytes(z, bits):
        raise ValueError(f"unpack_rows: uint8 rows of {row_bytes(z, bits)} bytes expected for {z} codes of {bits} bits, got {data.dtype} {data.shape}")
    wide = np.concatenate([data, np.zeros((data.shape[0], 1), dtype=np.uint8)], axis=1).astype(np.uint16)
    out = np.empty((data.shape[0], z), dtype=np.uint8)
    for k in range(z):
        j, sh = (k * bits) // 8, (k * bits) % 8
        w = wide[:, j] | (wide[:, j + 1] << np.uint16(8))
        out[:, k] = ((w >> np.uint16(sh)) & np.uint16(levels(bits))).astype(np.uint8)
    return out


def scale_of(rng, levels=255):
    """s_k = levels / rng_k where rng_k > 0, else 1 (a constant latent column: every code is 0 and decodes to lo_k)."""
    rng = np.asarray(rng, dtype=np.float64)
    s = np.ones_like(rng)
    np.divide(float(levels), rng, out=s, where=rng > 0)
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


def fold_flat(flat, layout, lo, rng, levels=255):
    """The fold on a flat parameter vector (any float array; the result is float64, NOT yet rounded): a copy with the four
    tensors of ``latent_tensors(layout)`` replaced."""
    out = np.array(flat, dtype=np.float64, copy=True)
    lo = np.asarray(lo, dtype=np.float64).reshape(-1)
    s = scale_of(np.asarray(rng, dtype=np.float64).reshape(-1), levels)
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


def fold(model, lo, rng, levels=255):
    """A COPY of ``model``'s flat parameters (numpy, the model's parameter type, ``model.nparams`` long) with the latent scale
    folded in; ``model`` itself is not changed.  lo, rng: (z,) float64, the calibrated minimum and range of every latent column;
    levels: the code that the maximum maps to (255 for bytes, 2**b - 1 for b-bit codes)."""
    flat = model.flat[: model.nparams].detach().to("cpu").numpy()
    return fold_flat(flat, model.layout, lo, rng, levels).astype(flat.dtype)


def unscale(codes, lo, rng, levels=255):
    """The latent a code stands for: q / s + lo (float64).  codes: uint8, one per element (unpacked)."""
    return widen8(codes).astype(np.float64) / scale_of(rng, levels) + np.asarray(lo, dtype=np.float64)
