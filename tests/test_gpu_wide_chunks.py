"""The SECOND iteration of the wide-layer family's row-chunk loops on the staged paths (fused.hip: wide_in_chunks / wide_out_chunks):
encode and decode walk the rows in chunks of 262,144 and forward_loss in chunks of 65,536, through a float32 staging buffer when
the call normalises on load / un-normalises on store.  Each case runs one call that crosses its chunk by 17 rows and holds it

  * bit for bit to two calls on the row blocks [0, chunk) and [chunk, n): the inference kernels are row-local with a fixed order,
    so no bit of a row may depend on how the rows were cut -- a wrong row offset, staging pointer or output pointer in the second
    iteration shows here;
  * at the seam (the last 16 rows of the first chunk and the 17 of the second) to the scalar fp64 oracle with `rel()` <= 1e-5,
    so that "the same bits twice" cannot be the same wrong bits.

Rows are made on the device; the oracle sees the seam rows only (forward_loss: all rows once, its loss is a sum over them).
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from oracle import c_oracle as orc
from test_gpu_parity import TOL32, dev, make_handle, rel

pytestmark = pytest.mark.gpu

CHUNK = 1 << 18           # encode / decode
CHUNK_LOSS = 1 << 16      # forward_loss
EXTRA = 17


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def raw_rows(n, F, mn, rg, seed):
    """n float64 rows on the device with column j uniform in [mn[j], mn[j] + rg[j])"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand((n, F), dtype=torch.float64, device="cuda", generator=g) * dev(rg) + dev(mn)


@pytest.fixture(scope="module")
def ae128():
    """AE(128, 3) on an fp32 handle: the narrowest table whose only state is the wide class"""
    dims = orc.ae_dims(128, 3)
    flat = orc.formula_params(dims, 128)
    h, _ = make_handle(dims, flat, "fp32")
    assert h.path == "fused"
    F = dims[0]
    mn, rg = np.linspace(-3.0, 40.0, F), np.linspace(0.5, 6.0, F)
    return h, dims, flat, mn, rg, dev(np.stack([mn, rg]))


def test_encode_decode_with_features_across_the_staging_chunk(ae128):
    h, dims, flat, mn, rg, feats = ae128
    F, n = dims[0], CHUNK + EXTRA
    raw = raw_rows(n, F, mn, rg, 1)
    mask = np.zeros(F, dtype=np.uint8)
    mask[::5] = 1
    dmask = dev(mask)
    z = h.encode(raw, features=feats)
    assert z.dtype == torch.float64
    z_blocks = torch.cat([h.encode(raw[:CHUNK], features=feats), h.encode(raw[CHUNK:], features=feats)])
    assert same_bits(z, z_blocks), "encode: whole call vs two row blocks"
    out = h.decode(z, features=feats, int_mask=dmask, out_dtype=torch.float64)
    out_blocks = torch.cat([h.decode(z[:CHUNK], features=feats, int_mask=dmask, out_dtype=torch.float64),
                            h.decode(z[CHUNK:], features=feats, int_mask=dmask, out_dtype=torch.float64)])
    assert same_bits(out, out_blocks), "decode: whole call vs two row blocks"
    # the seam against the oracle
    seam = slice(CHUNK - 16, n)
    xn = (raw[seam].cpu().numpy() - mn) / rg
    z_seam = z[seam].cpu().numpy()
    e = rel(z_seam, orc.encode(dims, flat, xn))
    print("encode seam rel", e)
    assert e <= TOL32
    pre = orc.decode(dims, flat, z_seam) * rg + mn
    got = out[seam].cpu().numpy()
    m1 = mask == 1
    e = rel(got[:, ~m1], pre[:, ~m1])
    print("decode seam rel", e)
    assert e <= TOL32
    # integer columns are truncated on store; a value within the fp32 error of an integer may land on either side of it
    edge = np.abs(pre[:, m1] - np.round(pre[:, m1])) < 1e-4 * np.maximum(1.0, np.abs(pre[:, m1]))
    assert np.array_equal(got[:, m1][~edge], np.trunc(pre[:, m1])[~edge])


def test_forward_loss_with_features_across_its_chunk(ae128):
    h, dims, flat, mn, rg, feats = ae128
    F, n = dims[0], CHUNK_LOSS + EXTRA
    raw = raw_rows(n, F, mn, rg, 2)
    recon, loss = h.forward_loss(raw, features=feats)
    blocks = torch.cat([h.forward_loss(raw[:CHUNK_LOSS], features=feats)[0], h.forward_loss(raw[CHUNK_LOSS:], features=feats)[0]])
    assert same_bits(recon, blocks), "reconstruction: whole call vs two row blocks"
    # the loss is a sum over all rows whose order follows the chunking: the oracle's bar, no bit comparison.  (The staging buffer
    # rounds the normalised rows to float32: 6e-8 relative, far inside the bar.)
    xn = (raw.cpu().numpy() - mn) / rg
    with ThreadPoolExecutor(8) as pool:      # (the oracle is scalar and row-local: row blocks side by side, seconds instead of many)
        fw = np.concatenate(list(pool.map(lambda b: orc.forward(dims, flat, b), np.array_split(xn, 8))))
    want = orc.loss(xn, fw)
    e = abs(loss.item() - want) / want
    print("forward_loss rel", e)
    assert e <= TOL32
    seam = slice(CHUNK_LOSS - 16, n)
    e = rel(recon[seam].cpu().numpy(), fw[seam])
    print("reconstruction seam rel", e)
    assert e <= TOL32


def test_bf16_encode_decode_across_the_staging_chunk():
    """(512, 6) on a bf16 handle, float32 rows, no features: the chunk loop of the bf16 kernels (their accuracy bar is held at small
    sizes by test_gpu_bf16_contract.py and test_gpu_parity.py)."""
    dims = orc.ae_dims(512, 6)
    h, _ = make_handle(dims, orc.formula_params(dims, 512), "bf16")
    assert h.path == "fused"
    n = CHUNK + EXTRA
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.rand((n, 512), dtype=torch.float32, device="cuda", generator=g)
    z = h.encode(x)
    assert same_bits(z, torch.cat([h.encode(x[:CHUNK]), h.encode(x[CHUNK:])])), "bf16 encode: whole call vs two row blocks"
    out = h.decode(z)
    assert same_bits(out, torch.cat([h.decode(z[:CHUNK]), h.decode(z[CHUNK:])])), "bf16 decode: whole call vs two row blocks"
