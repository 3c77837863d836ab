"""float64 restatement of the reference's PJ_Conv_AE (models.py:668-715) with the loss and Adam of its 2-D training loop, for the
tests: forward as written in the model definition (torch on the CPU in float64: conv2d / conv_transpose2d / linear / leaky_relu 0.2),
loss = utils.mse_sum_loss_l1(validate=True) of the 2-D path = sum((recon - x)^2) / true_data.shape[1] where shape[1] is the channel
count 1, the backward pass by autograd, and torch.optim.Adam's update written out in NumPy.

Parameters are the flat state-dict vector: per tensor (encoder.0, encoder.2, encoder.4, encoder.5, decoder.0, decoder.2, decoder.4,
decoder.5) the weight row-major, then the bias."""
import numpy as np
import torch
import torch.nn.functional as F

FRAME = 784


def layout(z):
    spec = [("encoder.0", (20, 1, 5, 5), 20), ("encoder.2", (50, 20, 5, 5), 50), ("encoder.4", (500, 2450), 500),
            ("encoder.5", (z, 500), z), ("decoder.0", (500, z), 500), ("decoder.2", (2450, 500), 2450),
            ("decoder.4", (50, 20, 5, 5), 20), ("decoder.5", (20, 1, 5, 5), 1)]
    out, off = [], 0
    for name, ws, nb in spec:
        n = int(np.prod(ws))
        out.append((name + ".weight", off, ws))
        out.append((name + ".bias", off + n, (nb,)))
        off += n + nb
    return out, off


def nparams(z):
    return layout(z)[1]


def tensors(z, flat, requires_grad=False):
    flat = torch.as_tensor(np.asarray(flat, dtype=np.float64))
    out = []
    for _, off, shape in layout(z)[0]:
        t = flat[off:off + int(np.prod(shape))].reshape(shape).clone()
        t.requires_grad_(requires_grad)
        out.append(t)
    return out


def _enc(p, x):
    h = F.leaky_relu(F.conv2d(x.reshape(-1, 1, 28, 28), p[0], p[1], stride=2, padding=2), 0.2)
    h = F.conv2d(h, p[2], p[3], stride=2, padding=2).reshape(-1, 2450)
    return F.linear(F.linear(h, p[4], p[5]), p[6], p[7])


def _dec(p, z):
    h = F.linear(F.leaky_relu(F.linear(z, p[8], p[9]), 0.2), p[10], p[11]).reshape(-1, 50, 7, 7)
    h = F.conv_transpose2d(h, p[12], p[13], stride=2, padding=2, output_padding=1)
    h = F.conv_transpose2d(h, p[14], p[15], stride=2, padding=2, output_padding=1)
    return F.leaky_relu(h, 0.2).reshape(-1, FRAME)


def _x(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float64)).reshape(-1, FRAME)


def encode(z, flat, x):
    with torch.no_grad():
        return _enc(tensors(z, flat), _x(x)).numpy()


def decode(z, flat, code):
    with torch.no_grad():
        return _dec(tensors(z, flat), torch.as_tensor(np.asarray(code, dtype=np.float64))).numpy()


def forward(z, flat, x):
    with torch.no_grad():
        p = tensors(z, flat)
        return _dec(p, _enc(p, _x(x))).numpy()


def loss(z, flat, x):
    r = forward(z, flat, x)
    return float(np.sum((r - np.asarray(x, dtype=np.float64).reshape(-1, FRAME)) ** 2))


def fwd_bwd(z, flat, x):
    """-> (loss, flat gradient)"""
    p = tensors(z, flat, requires_grad=True)
    xt = _x(x)
    l = ((_dec(p, _enc(p, xt)) - xt) ** 2).sum()
    l.backward()
    return float(l.item()), np.concatenate([t.grad.numpy().ravel() for t in p])


def adam_step(p, g, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam (defaults, no weight decay) on flat float64 arrays, in place."""
    m += (g - m) * (1 - b1)
    v *= b2
    v += (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p -= (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))


def rel(a, b):
    """max(rel-L2, max-norm): the suite's parity measure."""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    d = a - b
    return float(max(np.linalg.norm(d) / max(np.linalg.norm(b), 1e-300), np.max(np.abs(d)) / max(np.max(np.abs(b)), 1e-300)))
