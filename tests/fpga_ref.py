"""NumPy float64 restatement of the reference's FPGA_prototype_model (models.py:410-463) with the loss and Adam of its
training loop: forward, mse_sum_loss_l1(validate=True) = sum((r - x)^2) / n_features, backward with torch's ReLU rules
(relu(nan) = nan; the gradient passes where the layer's output is > 0) and torch.optim.Adam.

Parameters are the flat state-dict vector: for en1 en2 en3 de1 de2 de3, W[out][in] row-major then b[out]."""
import numpy as np

NAMES = ("en1", "en2", "en3", "de1", "de2", "de3")


def dims(n_features, z_dim):
    return [int(n_features), 20, 10, int(z_dim), 10, 20, int(n_features)]


def unflatten(d, flat):
    flat = np.asarray(flat, dtype=np.float64)
    out, off = [], 0
    for l in range(len(d) - 1):
        w = flat[off:off + d[l + 1] * d[l]].reshape(d[l + 1], d[l])
        off += d[l + 1] * d[l]
        b = flat[off:off + d[l + 1]]
        off += d[l + 1]
        out.append((w, b))
    return out


def nparams(d):
    return sum(d[l + 1] * d[l] + d[l + 1] for l in range(len(d) - 1))


def has_act(l, L=6):
    return not (l == L // 2 - 1 or l == L - 1)


def relu(v):
    return np.where(np.isnan(v) | (v > 0), v, 0.0)


def _layers(d, flat, x, l0, l1):
    ys = [np.asarray(x, dtype=np.float64)]
    for l, (w, b) in list(enumerate(unflatten(d, flat)))[l0:l1]:
        y = ys[-1] @ w.T + b
        ys.append(relu(y) if has_act(l) else y)
    return ys


def encode(d, flat, x):
    return _layers(d, flat, x, 0, 3)[-1]


def decode(d, flat, z):
    return _layers(d, flat, z, 3, 6)[-1]


def forward(d, flat, x):
    return _layers(d, flat, x, 0, 6)[-1]


def pre_activations(d, flat, x):
    """The pre-activation of every ReLU layer (en1, en2, de1, de2) -- for choosing rows away from the kink."""
    ys = _layers(d, flat, x, 0, 6)
    out = []
    for l, (w, b) in enumerate(unflatten(d, flat)):
        if has_act(l):
            out.append(ys[l] @ w.T + b)
    return out


def off_the_kink(d, flat, x, margin=2e-5):
    """Rows whose ReLU pre-activations all stay farther than `margin` from 0."""
    keep = np.ones(x.shape[0], dtype=bool)
    for a in pre_activations(d, flat, x):
        keep &= np.all(np.abs(a) > margin, axis=1)
    return keep


def fwd_bwd(d, flat, x, latent_grad=None):
    """(loss, flat gradient) of loss = sum((r - x)^2) / n_features; latent_grad (rows, z) is added to dL/dz."""
    x = np.asarray(x, dtype=np.float64)
    layers = unflatten(d, flat)
    ys = _layers(d, flat, x, 0, 6)
    e = ys[-1] - x
    loss = float(np.sum(e * e) / d[0])
    dz = 2.0 * e / d[0]
    grads = [None] * 6
    for l in range(5, -1, -1):
        w, b = layers[l]
        grads[l] = (dz.T @ ys[l], dz.sum(axis=0))
        if l == 0:
            break
        dy = dz @ w
        if has_act(l - 1):
            dy = np.where(ys[l] <= 0, 0.0, dy)
        if l == 3 and latent_grad is not None:
            dy = dy + np.asarray(latent_grad, dtype=np.float64)
        dz = dy
    return loss, np.concatenate([np.concatenate([gw.ravel(), gb]) for gw, gb in grads])


def adam_step(params, grad, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam (single tensor, no weight decay) in place on flat float64 arrays."""
    m += (grad - m) * (1.0 - beta1)
    v *= beta2
    v += (1.0 - beta2) * grad * grad
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    params -= (lr / bc1) * (m / denom)
    return params, m, v
