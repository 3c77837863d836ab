"""NumPy emulation of the arithmetic contract of the bfloat16 kernels of the 24-column autoencoder and of the wide models (include/baler_amd.h,
"BF16 arithmetic"): csrc/bf16.hip (encode / decode / forward + loss) and csrc/bf16_train.hip (the
training pair).  TEST INFRASTRUCTURE: the GPU tests compare the kernels with it element by element (tests/test_gpu_bf16_contract.py),
the host test proves that the comparison notices every deviation it is meant to notice (tests/test_bf16_contract_host.py).

The contract, as code:

  inference   W_l = bf16(fp32 master), b_l stays fp32.  A row goes float64 (normalised in float64 when features are given) ->
              float32 -> bf16.  Per layer  a = b_l + sum_k W_l[., k] h[k]  in fp32 (the bias is the accumulator's start value);
              an activated layer hands  bf16(max(a, a * 0.01f))  on -- LeakyReLU on the fp32 accumulator with the fp32 slope, ONE
              rounding per layer input; the latent and the reconstruction stay fp32.  forward = decode(encode(x)): the fp32 latent
              passes through memory and is rounded by the decoder's loader.  Loss: float64 sum of (fp32 recon - fp32 x)^2 / F.
              Un-normalisation: float64(recon) * range + min with two float64 roundings, trunc() on the int columns.
  training    W_l AND b_l = bf16(fp32 master): the bias is column K of the packed weights and meets a ones column of the input
              image, so it is one more product of the fp32 sum (no separate start value).  Every layer input X_l is a bf16 image,
              the latent X_4 included; the forward is otherwise the inference one.  recon (fp32) - x (fp32, NOT the bf16 image) =
              e; loss = float64 sum e^2 / F; dL/drecon = e * (2.0f / F) in fp32, rounded to bf16 = dZ_7.  Backward, l = 7 .. 1:
              dX_l = dZ_l W_l (bf16 x bf16, fp32 sum) and dZ_{l-1} = bf16(dX_l) where the STORED bf16 activation X_l is >= 0,
              bf16(dX_l * 0.01f) where its sign bit is set (no mask under the latent).  [dW_l | db_l] = dZ_l^T [X_l | 1]: bf16 x
              bf16 products, fp32 sums over the batch.  Gradients and loss are returned in float32.

Every function takes the accumulation as a parameter (`ACCS`: NumPy float32 matmul, float64 accumulation rounded once, float32
partial sums over k blocks of 32 and of 4): the contract fixes what is rounded where, not the order of an fp32 sum, and the distance
between these variants is what the tests derive their bars from.  `Contract` holds the knobs; `WRONG` lists deliberately wrong
settings, each a deviation a kernel could have."""
import dataclasses

import numpy as np

from baler_amd import hostio

F32 = np.float32


# ---- roundings ------------------------------------------------------------------------------------------------------------------
def round_bf16(a):
    """float32 array -> the float32 values of its bfloat16 rounding (nearest even)."""
    return hostio.bf16_widen(hostio.bf16_bits(np.asarray(a, dtype=F32))).astype(F32).reshape(np.shape(a))


def trunc_bf16(a):
    """The WRONG rounding: the low 16 bits dropped."""
    u = np.ascontiguousarray(a, dtype=F32).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(F32).reshape(np.shape(a))


def round_f16(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=F32).astype(np.float16).astype(F32)


# ---- accumulation variants: acc(a (n, K), b (K, N), c = None) -> float32 (c + a @ b) -----------------------------------------------
def acc_f32(a, b, c=None):
    s = np.asarray(a, dtype=F32) @ np.asarray(b, dtype=F32)
    return s if c is None else (s + c).astype(F32)


def acc_f64(a, b, c=None):
    s = np.asarray(a, dtype=np.float64) @ np.asarray(b, dtype=np.float64)
    return (s if c is None else s + c).astype(F32)


def _acc_blocks(blk):
    def acc(a, b, c=None):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        s = np.zeros((a.shape[0], b.shape[1]), dtype=F32)
        if c is not None:
            s = s + np.asarray(c, dtype=F32)
        for k in range(0, a.shape[1], blk):
            s = s + (a[:, k:k + blk] @ b[k:k + blk]).astype(F32)      # float32 partial sum of the block, float32 running sum
        return s
    return acc


acc_k32, acc_k4 = _acc_blocks(32), _acc_blocks(4)
ACCS = {"f32": acc_f32, "f64": acc_f64, "k32": acc_k32, "k4": acc_k4}


# ---- the knobs --------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Contract:
    rnd: object = round_bf16
    slope: object = F32(0.01)
    act: str = "fp32"                 # "fp32": round(lrelu(a)) | "after": lrelu of the rounded value | "in16": lrelu IN the 16-bit type
    infer_bias_rounded: bool = False
    train_bias_rounded: bool = True
    drop: object = ()                 # (layer, k block) pairs: that block of 32 input features is lost for the last row of a ragged 64-row group
    db_col: object = None             # column of X_l that [dW | db] takes for db; None: the ones column
    dz_rounded: bool = True


RIGHT = Contract()
F16 = Contract(rnd=round_f16, slope=round_f16(F32(0.01)), act="in16")      # BAMD_MODE_F16 (inference only): test_f16_host.f16_chain
WRONG = {
    "truncating rounding": dataclasses.replace(RIGHT, rnd=trunc_bf16),
    "training bias in fp32, inference bias rounded": dataclasses.replace(RIGHT, infer_bias_rounded=True, train_bias_rounded=False),
    "slope bf16(0.01)": dataclasses.replace(RIGHT, slope=round_bf16(F32(0.01))),
    "LeakyReLU after the rounding": dataclasses.replace(RIGHT, act="after"),
    "k block dropped for one ragged row": dataclasses.replace(RIGHT, drop=((1, 2), (7, 3))),      # one encoder, one decoder layer
    "db from another column": dataclasses.replace(RIGHT, db_col=0),
    "dZ left in fp32": dataclasses.replace(RIGHT, dz_rounded=False),
}
TRAINING_ONLY = ("db from another column", "dZ left in fp32")


# ---- pieces -----------------------------------------------------------------------------------------------------------------------
def layers(dims, flat):
    """[(W (N, K), b (N,))] of the float32 master copy of `flat` (state-dict order)."""
    flat32 = np.asarray(flat, dtype=np.float64).astype(F32)
    out, off = [], 0
    for l in range(len(dims) - 1):
        K, N = dims[l], dims[l + 1]
        out.append((flat32[off:off + N * K].reshape(N, K), flat32[off + N * K:off + N * K + N]))
        off += N * K + N
    return out


def linear_layers(dims):
    L = len(dims) - 1
    return (L // 2 - 1, L - 1)


def rows32(x, feats=None):
    """Rows as the loaders see them: float64 (float32 rows widened), normalised in float64 when `feats` = [min; range], one rounding
    to float32."""
    d = np.asarray(x).astype(np.float64)
    if feats is not None:
        d = (d - feats[0]) / feats[1]
    return d.astype(F32)


def _lrelu(a, slope):
    return np.maximum(a, (a * slope).astype(F32))


def _activate(c, a):
    """fp32 accumulator of an activated layer -> the 16-bit layer input (as float32 values)."""
    if c.act == "fp32":
        return c.rnd(_lrelu(a, c.slope))
    r = c.rnd(a)
    if c.act == "in16":
        return np.maximum(r, c.rnd(r * c.slope))
    return c.rnd(_lrelu(r, c.slope))


def _activate32(c, a):
    """fp32 accumulator of an activated layer -> the layer's fp32 output; a 16-bit layer rounds it when it reads it (a value that
    is a 16-bit number already passes that rounding unchanged)."""
    return _lrelu(a, c.slope) if c.act == "fp32" else _activate(c, a)


def _product(c, acc, l, h, wt, bias):
    a = acc(h, wt, bias)
    n = h.shape[0]
    for dl, q in c.drop:
        if dl == l and n % 64:
            hr = h[n - 1:n].copy()
            hr[:, 32 * q:32 * q + 32] = 0
            a[n - 1] = acc(hr, wt, bias)[0]
    return a


# ---- inference --------------------------------------------------------------------------------------------------------------------
def infer(dims, flat, x, lo, hi, acc=acc_f32, c=RIGHT, feats=None, fp32_layers=()):
    """Layers lo .. hi - 1 (encode: 0, 4; decode: 4, 8) of the inference contract on rows `x`.  Returns float32.  `fp32_layers`: the
    layers that run in exact fp32 on the fp32 master weights (narrow layers of some wide-model kernels); their input is not rounded."""
    lay, lin = layers(dims, flat), linear_layers(dims)
    h = rows32(x, feats)
    with np.errstate(over="ignore", invalid="ignore"):
        for l in range(lo, hi):
            W, b = lay[l]
            if l in fp32_layers:
                a = _product(c, acc, l, h, W.T, b)
            else:
                a = _product(c, acc, l, c.rnd(h), c.rnd(W).T, c.rnd(b) if c.infer_bias_rounded else b)
            h = a if l in lin else _activate32(c, a)
    return h


def encode(dims, flat, x, acc=acc_f32, c=RIGHT, feats=None, fp32_layers=()):
    return infer(dims, flat, x, 0, (len(dims) - 1) // 2, acc, c, feats, fp32_layers)


def decode(dims, flat, z, acc=acc_f32, c=RIGHT, feats=None, int_mask=None, fp32_layers=()):
    """decode(z) in float32; with `feats` the un-normalised float64 table (int columns truncated) the kernel stores."""
    y = infer(dims, flat, z, (len(dims) - 1) // 2, len(dims) - 1, acc, c, None, fp32_layers)
    return y if feats is None else unnormalise(y, feats, int_mask)


def unnormalise(y, feats, int_mask=None):
    d = np.asarray(y, dtype=F32).astype(np.float64) * feats[1] + feats[0]      # two float64 roundings
    if int_mask is not None:
        m = np.asarray(int_mask).astype(bool)
        d[:, m] = np.trunc(d[:, m])
    return d


def forward(dims, flat, x, acc=acc_f32, c=RIGHT, feats=None):
    """(reconstruction float32, loss): decode(encode(x)) with the float32 latent in between, loss = sum (recon - x)^2 / F in float64."""
    x32 = rows32(x, feats)
    recon = decode(dims, flat, encode(dims, flat, x32, acc, c), acc, c)
    return recon, float(((recon.astype(np.float64) - x32.astype(np.float64)) ** 2).sum() / dims[0])


# ---- one training pass ------------------------------------------------------------------------------------------------------------
def train_rows(dims, flat, x, acc=acc_f32, c=RIGHT, feats=None):
    """The row-local part of a training pass (forward, loss terms, input-gradient chain): every row's images X_l and dZ_l.  Rows do
    not see each other here, so a prefix of the result is the result of the prefix (but for the row `drop` picks)."""
    lay, lin = layers(dims, flat), linear_layers(dims)
    L = len(dims) - 1
    x32 = rows32(x, feats)
    n = x32.shape[0]
    ones = np.ones((n, 1), dtype=F32)
    wb = [np.concatenate([c.rnd(W), (c.rnd(b) if c.train_bias_rounded else b)[:, None]], axis=1) for W, b in lay]      # [W | b]
    X = [c.rnd(x32)]
    for l in range(L):
        a = _product(c, acc, l, np.concatenate([X[l], ones], axis=1), wb[l].T.copy(), None)
        if l == L - 1:
            recon = a
        else:
            X.append(c.rnd(a) if l in lin else _activate(c, a))
    e = recon - x32                                                        # fp32 subtraction against the fp32 row
    d = (e * (F32(2.0) / F32(dims[0]))).astype(F32)
    dZ = [None] * L
    dZ[L - 1] = c.rnd(d) if c.dz_rounded else d
    rz = c.rnd if c.dz_rounded else (lambda a: a)
    for l in range(L - 1, 0, -1):
        dx = acc(dZ[l], wb[l][:, :-1].copy())
        if l - 1 in lin:
            dZ[l - 1] = rz(dx)
        else:
            dZ[l - 1] = np.where(np.signbit(X[l]), rz((dx * c.slope).astype(F32)), rz(dx))      # the mask is the stored activation's sign
    return dict(X=X, dZ=dZ, e=e, recon=recon, F=dims[0], n=n)


def train_grads(rows, n=None, acc=acc_f32, c=RIGHT):
    """(loss, flat float32 gradient in state-dict order) of the first n rows of `train_rows`' result."""
    n = rows["n"] if n is None else n
    g = []
    for X, dZ in zip(rows["X"], rows["dZ"]):
        last = np.ones((n, 1), dtype=F32) if c.db_col is None else X[:n, c.db_col:c.db_col + 1]
        G = acc(dZ[:n].T.copy(), np.concatenate([X[:n], last], axis=1))       # [dW | db], summed over the batch
        g += [G[:, :-1].ravel(), G[:, -1]]
    loss = F32((rows["e"][:n].astype(np.float64) ** 2).sum() / rows["F"])
    return float(loss), np.concatenate(g).astype(F32)


def train_pass(dims, flat, x, acc=acc_f32, c=RIGHT, feats=None):
    return train_grads(train_rows(dims, flat, x, acc, c, feats), None, acc, c)


WIDE_DW_MIN_ROWS = 128      # csrc/generic.hip plan_short_dw: below it no layer's weight gradient runs on the streamed (bf16) kernels


def wide_clear_of_the_kink(dims, flat, n, seed, margin=2e-5, c=RIGHT):
    """`clear_of_the_kink` in the arithmetic of the wide models' training pass (only en1 and de4 round their operands)."""
    x = np.random.default_rng(seed).random((2 * n + 64, dims[0]))
    lay, lin = layers(dims, flat), linear_layers(dims)
    keep, h = np.ones(x.shape[0], dtype=bool), rows32(x)
    for l, (W, b) in enumerate(lay):
        a = acc_f64(c.rnd(h), c.rnd(W).T, b) if l in (0, len(lay) - 1) else acc_f64(h, W.T, b)
        if l not in lin:
            keep &= np.abs(a).min(axis=1) > margin
            a = _lrelu(a, c.slope)
        h = a
    assert keep.sum() >= n
    return np.ascontiguousarray(x[keep][:n])


def wide_train_pass(dims, flat, x, acc=acc_f32, c=RIGHT, feats=None):
    """One training pass of a wide model on the bf16 launches (csrc/fused.hip wide_bf16_train_fwd / _bwd_kernel, csrc/generic.hip
    dw_wide_bf16_k / dw_short_bf16_k): (loss, flat float32 gradient).  Only the two WIDE layers touch bfloat16:
      forward   en1 and de4: input and weights rounded to bfloat16, fp32 bias as start value, fp32 sums; the six narrow layers in exact
                fp32 on the fp32 master weights; every activation is stored in fp32 (LeakyReLU in fp32, never rounded).
      loss      e = fp32 reconstruction - fp32 row; float64 sum of e^2 / F; dL/drecon = e * (2.0f / F), bfloat16 for its bf16 readers.
      backward  de4's input-gradient product bfloat16(dL/drecon) x bfloat16(W_7) with fp32 sums; masks from the stored fp32 activations
                (y > 0 ? 1 : 0.01f); layers 6 .. 1 and every dZ below de4 in exact fp32.
      gradients [dW_7 | db_7] = bf16(dL/drecon)^T [bf16(y_7) | 1] and [dW_0 | db_0] = bf16(dZ_0)^T [bf16(x) | 1] with fp32 sums -- in passes
                of at least WIDE_DW_MIN_ROWS rows; a smaller pass takes the one-tile-per-workgroup fp32 product for every layer, on the
                UNROUNDED fp32 dL/drecon, dZ_0, rows and y_7; the six narrow layers' gradients in exact fp32 always."""
    lay, lin = layers(dims, flat), linear_layers(dims)
    L = len(dims) - 1
    wide = (0, L - 1)
    x32 = rows32(x, feats)
    n = x32.shape[0]
    ones = np.ones((n, 1), dtype=F32)
    y = [x32]
    for l, (W, b) in enumerate(lay):
        a = acc(c.rnd(y[l]), c.rnd(W).T, c.rnd(b) if c.infer_bias_rounded else b) if l in wide else acc(y[l], W.T, b)
        y.append(a if l in lin else _lrelu(a, c.slope))
    e = y[L] - x32
    loss = F32((e.astype(np.float64) ** 2).sum() / dims[0])
    dz = (e * (F32(2.0) / F32(dims[0]))).astype(F32)      # fp32 here; bfloat16 for whoever reads it as a bf16 MFMA operand
    dw16 = n >= WIDE_DW_MIN_ROWS
    g = [None] * L
    for l in range(L - 1, -1, -1):
        W = lay[l][0]
        if l in wide and dw16:
            G = acc(c.rnd(dz).T, np.concatenate([c.rnd(y[l]), ones], axis=1))
        else:
            G = acc(dz.T, np.concatenate([y[l], ones], axis=1))
        g[l] = np.concatenate([G[:, :-1].ravel(), G[:, -1]])
        if l:
            dx = acc(c.rnd(dz), c.rnd(W)) if l in wide else acc(dz, W)
            dz = dx if l - 1 in lin else (dx * np.where(y[l] > 0, F32(1.0), c.slope)).astype(F32)
    return float(loss), np.concatenate(g).astype(F32)


def tie_clearance(dims, flat, x, lo, hi, c=RIGHT, fp32_layers=()):
    """Per row: how far the values that layers lo .. hi - 1 round to bfloat16 on the way stay from a rounding boundary (the midpoint
    of two neighbouring bfloat16 numbers), in units of 2^-24 x (|b| + sum_k |w_k h_k|) -- the scale of the difference between two
    orders of the fp32 sum behind the value.  A row whose clearance is a few units takes the same roundings in every summation
    order: what `clear_of_the_kink` is for the sign, this is for the 16-bit roundings.  (The rows themselves and a decode's codes are
    given numbers: their rounding does not depend on an order.)"""
    lay, lin = layers(dims, flat), linear_layers(dims)
    h = rows32(x)
    clear = np.full(h.shape[0], np.inf)
    for l in range(lo, hi):
        W, b = lay[l]
        if l not in fp32_layers:
            h, W = c.rnd(h), c.rnd(W)
        a = acc_f64(h, W.T, b)
        s = np.abs(h).astype(np.float64) @ np.abs(W).T.astype(np.float64) + np.abs(b)
        if l not in lin:
            s = np.where(a < 0, s * np.float64(c.slope), s)
            a = _lrelu(a, c.slope)
        h = a if l + 1 in fp32_layers else c.rnd(a)
        if l + 1 < hi and l + 1 not in fp32_layers:     # the last layer's result and the input of an fp32 layer are not rounded
            bits = hostio.bf16_bits(np.abs(h)).astype(np.int64)
            up = hostio.bf16_widen((bits + 1).astype(np.uint16)).astype(np.float64).reshape(h.shape)
            dn = hostio.bf16_widen(np.maximum(bits - 1, 0).astype(np.uint16)).astype(np.float64).reshape(h.shape)
            m, v = np.abs(h).astype(np.float64), np.abs(a).astype(np.float64)
            dist = np.minimum((m + up) / 2 - v, v - (m + dn) / 2)
            clear = np.minimum(clear, (dist / (2.0 ** -24 * s)).min(axis=1))
    return clear


def tensor_slices(dims):
    """[(name, slice)] of the 2 L tensors of a flat parameter / gradient vector."""
    out, off = [], 0
    for l in range(len(dims) - 1):
        for name, k in ((f"W{l}", dims[l + 1] * dims[l]), (f"b{l}", dims[l + 1])):
            out.append((name, slice(off, off + k)))
            off += k
    return out


def clear_of_the_kink(dims, flat, n, seed, margin=2e-5, c=RIGHT):
    """n uniform random rows none of whose LeakyReLU pre-activations -- in THIS emulation's arithmetic, on the encode path and on
    the forward path of the training pass (float64 accumulation) -- lies within `margin` of zero (tests/test_gpu_parity.py:
    off_the_kink, which does it for the float64 forward): a sign that depends on the order of an fp32 sum is a property of the
    comparison, not of the kernel."""
    x = np.random.default_rng(seed).random((2 * n + 64, dims[0]))
    lay, lin = layers(dims, flat), linear_layers(dims)
    keep = np.ones(x.shape[0], dtype=bool)
    for bias_rounded in (True, False):            # the training pass; encode followed by decode (forward)
        h = c.rnd(rows32(x))
        for l, (W, b) in enumerate(lay):
            a = acc_f64(h, c.rnd(W).T, c.rnd(b) if bias_rounded else b)
            if l not in lin:
                keep &= np.abs(a).min(axis=1) > margin
                h = _activate(c, a)
            else:
                h = c.rnd(a)
    assert keep.sum() >= n
    return np.ascontiguousarray(x[keep][:n])
