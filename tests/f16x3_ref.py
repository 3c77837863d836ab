"""The fp16x3 inference mode (BAMD_MODE_F16X3) in NumPy: the contract paragraph of include/baler_amd.h as code.

Every fp32 operand a is split into two binary16 values,
    hi = binary16(a)                       (nearest even, no clamp: beyond 65504 it is +-inf)
    lo = binary16((a - hi) * scale)        (a - hi is exact in fp32; scale = 2^11 is a power of two)
and a layer is
    main = b + sum hi_w * hi_h             (fp32 bias as the start value)
    corr = sum (lo_w * hi_h + hi_w * lo_h)
    a    = main + corr / scale             (fp32)
with LeakyReLU as max(a, a * 0.01f) on the fp32 value BEFORE the split of the next layer's input.  The latent and the reconstruction
stay fp32.  Rows are rounded once to float32 (after the float64 normalisation, which the callers here have done already).

``chain`` takes the scale, the number of products (1: hi*hi only; 3: the contract; 4: with lo*lo) and the accumulation dtype as
parameters, so that the tests can show what each of them buys.  With scale = 1 it is the UNSCALED form: lo = binary16(a - hi) and all
products in ONE accumulator.  Every binary16 x binary16 product is exact in float32 and in float64; what the accumulation dtype
changes is the rounding of the sums (the MFMA's own is fp32 of unspecified order)."""
import numpy as np

SCALE = 2048.0


def round_f16(a):
    """float32 array -> the float32 values of its binary16 rounding (nearest even; beyond 65504: +-inf)."""
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


def split(a, scale=SCALE):
    """float32 array -> (hi, lo) as float32 arrays holding binary16 values; a is hi + lo / scale up to lo's rounding."""
    a = np.asarray(a, dtype=np.float32)
    hi = round_f16(a)
    with np.errstate(invalid="ignore", over="ignore"):
        lo = round_f16((a - hi) * np.float32(scale))
    return hi, lo


def layer_offsets(dims):
    offs, off = [], 0
    for l in range(len(dims) - 1):
        offs.append(off)
        off += dims[l + 1] * dims[l] + dims[l + 1]
    return offs


def chain(dims, flat, x, lo, hi, scale=SCALE, products=3, acc=np.float32):
    """Layers lo .. hi - 1 of the autoencoder `dims` (encode: 0, 4; decode: 4, 8; forward: 0, 8) on rows `x` in the split
    arithmetic.  Returns float32.  A forward pass hands the fp32 latent to the decoder unrounded, so chain(0, 8) is the kernel's
    bamd_forward_loss."""
    assert products in (1, 3, 4)
    flat32 = np.asarray(flat, dtype=np.float64).astype(np.float32)
    L = len(dims) - 1
    offs = layer_offsets(dims)
    h = np.asarray(x, dtype=np.float64).astype(np.float32)
    inv = np.float32(1.0 / scale)

    def mm(a, b):
        return a.astype(acc) @ b.astype(acc).T

    with np.errstate(over="ignore", invalid="ignore"):
        for l in range(lo, hi):
            K, N = dims[l], dims[l + 1]
            w = flat32[offs[l]:offs[l] + N * K].reshape(N, K)
            b = flat32[offs[l] + N * K:offs[l] + N * K + N]
            wh, wl = split(w, scale)
            hh, hl = split(h, scale)
            if products == 1:
                a = (mm(hh, wh) + b.astype(acc)).astype(np.float32)
            elif scale == 1:      # the unscaled form: one accumulator
                a = (mm(hh, wh) + b.astype(acc) + mm(hh, wl) + mm(hl, wh) + (mm(hl, wl) if products == 4 else 0)).astype(np.float32)
            else:
                main = (mm(hh, wh) + b.astype(acc)).astype(np.float32)
                corr = mm(hh, wl) + mm(hl, wh)
                if products == 4:
                    corr = corr + mm(hl, wl) * acc(1.0 / scale)
                a = main + corr.astype(np.float32) * inv
            if not (l == L // 2 - 1 or l == L - 1):
                a = np.maximum(a, a * np.float32(0.01))
            h = a.astype(np.float32)
    return h


def fp32_chain(dims, flat, x, lo, hi):
    """The same layers in plain float32 (NumPy's float32 matmul): the yardstick the split chain is measured against."""
    flat32 = np.asarray(flat, dtype=np.float64).astype(np.float32)
    L = len(dims) - 1
    offs = layer_offsets(dims)
    h = np.asarray(x, dtype=np.float64).astype(np.float32)
    for l in range(lo, hi):
        K, N = dims[l], dims[l + 1]
        w = flat32[offs[l]:offs[l] + N * K].reshape(N, K)
        b = flat32[offs[l] + N * K:offs[l] + N * K + N]
        a = h @ w.T + b
        if not (l == L // 2 - 1 or l == L - 1):
            a = np.maximum(a, a * np.float32(0.01))
        h = a.astype(np.float32)
    return h


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def rel(a, b):
    """max(rel-L2, max-norm error) over the whole tensor: the parity measure of tests/test_gpu_parity.py."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return max(rel_l2(a, b), float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)))
