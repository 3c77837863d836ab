"""config.latent_dtype = "uint5" (and once "uint1") end to end on the GPU: train -> compress -> decompress on the 3,000-row synthetic
CMS table with the workspace and worker of tests/test_gpu_latent8_cli.py: the archive's members and shapes, model.pt left alone,
decompression against the public Handle API on the unpacked codes and the archive's scale, decompression without the config key,
two ranks on one GPU (gloo) against one process, and the error-bounded deltas side channel on the decoded packed bytes."""
import os

import numpy as np
import pytest
import torch

import test_gpu_latent8_cli as c8
from test_gpu_colstats_cli import N_ROWS, _workspace

pytestmark = pytest.mark.gpu

Z = 15
BITS = 5
S = 10      # ceil(15 * 5 / 8)


def _folded_handle(out, scale, bits):
    """The public API's side of decompress: the model of model.pt in the CLI worker's mode, the archive's scale folded in for
    2**bits - 1 levels."""
    from baler_amd import latent8
    from baler_amd.modules import data_processing, models
    models.set_default_mode("fp64")
    try:
        model = data_processing.load_model(data_processing.initialise_model("AE"), str(out / "compressed_output" / "model.pt"),
                                           n_features=24, z_dim=Z)
    finally:
        models.set_default_mode("fp32")
    model.eval()
    model.load_flat(latent8.fold(model, scale[0], scale[1], latent8.levels(bits)))
    return model, model.handle()


def _check_archive(comp, bits):
    from baler_amd import latent8
    a = np.load(comp)
    assert sorted(a.files) == ["data", "latent_dtype", "latent_scale", "names", "normalization_features"]      # no new key
    data, scale = a["data"], a["latent_scale"]
    width = -(-Z * bits // 8)
    assert data.dtype == np.uint8 and data.shape == (N_ROWS, width) and data.nbytes == N_ROWS * width
    assert str(a["latent_dtype"]) == f"uint{bits}"
    assert scale.dtype == np.float64 and scale.shape == (2, Z) and np.isfinite(scale).all() and (scale[1] > 0).all()
    q = latent8.unpack_rows(data, Z, bits)
    assert (q.min(axis=0) == 0).all() and (q.max(axis=0) == 2 ** bits - 1).all()      # the calibration is the table's own extrema
    pad = 8 * width - Z * bits
    assert pad == 0 or not (data[:, -1] >> (8 - pad)).any()
    return data, scale, q


def test_cli_uint5_archive_decompression_and_two_ranks(tmp_path):
    from baler_amd import latent8, native, synth
    out = _workspace(tmp_path)
    comp, dec = out / "compressed_output" / "compressed.npz", out / "decompressed_output" / "decompressed.npz"
    model_pt = out / "compressed_output" / "model.pt"
    c8._set_config(tmp_path, f'\n    c.latent_dtype = "uint{BITS}"\n')
    c8._run(tmp_path, ["train", "compress", "decompress"])
    model_bytes = model_pt.read_bytes()
    data, scale, q = _check_archive(comp, BITS)
    assert data.shape == (N_ROWS, S)
    print(f"compressed.npz: {os.path.getsize(comp)} bytes with uint{BITS} codes, {data.nbytes} of them codes ({N_ROWS * Z} with uint8)")

    # the decompressed table is the decode of the unpacked codes on the folded handle, bit for bit -- and of the packed bytes
    got = np.load(dec)["data"]
    model, h = _folded_handle(out, scale, BITS)
    feats, mask = c8._renorm(out)
    want = h.decode(torch.from_numpy(q.astype(np.float32)).cuda(), features=feats, int_mask=mask, out_dtype=torch.float64).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(h.decode(torch.from_numpy(data).cuda(), features=feats, int_mask=mask, out_dtype=torch.float64,
                                           code_bits=BITS).cpu().numpy(), want)
    # the codes are the folded handle's
    x = torch.from_numpy(synth.cms_rows(N_ROWS)).cuda()
    np.testing.assert_array_equal(h.encode(x, features=native.minmax(x), out_dtype=torch.uint8, code_bits=BITS).cpu().numpy(), data)
    z32 = h.encode(x, features=native.minmax(x), out_dtype=torch.float32).cpu().numpy()
    np.testing.assert_array_equal(latent8.pack_rows(latent8.qb(z32, BITS), BITS), data)

    # decompress takes everything from the archive: without the config key the same table comes out
    one_c, one_d = comp.read_bytes(), dec.read_bytes()
    os.remove(dec)
    c8._set_config(tmp_path, "")
    c8._run(tmp_path, ["decompress"])
    assert dec.read_bytes() == one_d

    # two ranks on one GPU write the archive and the table one process writes
    os.remove(comp)
    os.remove(dec)
    c8._set_config(tmp_path, f'\n    c.latent_dtype = "uint{BITS}"\n')
    c8._run(tmp_path, ["compress", "decompress"], ranks=2)
    assert comp.read_bytes() == one_c and dec.read_bytes() == one_d
    assert model_pt.read_bytes() == model_bytes

    # one bit per code: the run ends without error (no quality bar); 15 bits in 2 bytes per row
    c8._set_config(tmp_path, '\n    c.latent_dtype = "uint1"\n')
    c8._run(tmp_path, ["compress", "decompress"])
    d1, _, q1 = _check_archive(comp, 1)
    assert d1.shape == (N_ROWS, 2) and np.load(dec)["data"].shape == got.shape and np.isfinite(np.load(dec)["data"]).all()


def test_cli_deltas_on_the_decoded_packed_bytes(tmp_path):
    """save_error_bounded_deltas with uint5 codes: the side channel is computed from decode() of the PACKED BYTES on the folded handle,
    which is what decompress decodes, so the bound holds after decompression.  Stated as for the uint8 codes
    (tests/test_gpu_latent8_cli.py), with oracle/deltas.py on the float columns of the normalised table:

    * every element with |x| >= 0.02 meets the 10 % bound.  Below that the reference's float16 deltas cannot restore it: a delta is
      float16(float16(decoded) - float16(x)), an absolute error of up to about 2e-3 for normalised values, which is 10 % of 0.02;
    * the elements that remain above the bound are exactly those that oracle/deltas.py's own side channel leaves above it when it
      is given the same decoded table."""
    from baler_amd import synth
    from baler_amd.modules import helper
    from oracle import c_oracle as orc
    from oracle import deltas as odeltas
    out = _workspace(tmp_path)
    c8._set_config(tmp_path, f'\n    c.latent_dtype = "uint{BITS}"\n    c.save_error_bounded_deltas = True\n    c.error_bounded_requirement = 10\n')
    c8._run(tmp_path, ["train", "compress", "decompress"])
    data, scale, q = _check_archive(out / "compressed_output" / "compressed.npz", BITS)
    rows, cols, vals = helper.load_deltas(str(out / "compressed_output" / "compressed_deltas.npz.gz"),
                                          str(out / "compressed_output" / "compressed_batch_index_metadata.npz.gz"), 512)
    assert len(rows) > 100
    raw = synth.cms_rows(N_ROWS)
    nf, x_n = orc.find_minmax(raw), orc.normalize(raw)
    fl = np.array([t != "int" for t in synth.CMS_TYPE_LIST])
    dec = np.load(out / "decompressed_output" / "decompressed.npz")["data"]
    restored = ((dec - nf[0]) / nf[1])[:, fl]
    x_f = x_n[:, fl]
    _, (br, bc) = odeltas.error_bounded_requirement(10, restored, x_f)
    small = np.abs(x_f[br, bc]) < 0.02
    print(f"{len(rows)} deltas; {len(br)} float-column elements above the 10 % bound after decompression, largest |x| among them "
          f"{np.abs(x_f[br, bc]).max() if len(br) else 0:.3e}")
    assert small.all(), f"{int((~small).sum())} elements with |x| >= 0.02 miss the bound"
    # the oracle's side channel on the same decoded table (decode of the packed bytes, normalised units)
    model, h = _folded_handle(out, scale, BITS)
    dec_n = h.decode(torch.from_numpy(data).cuda(), out_dtype=torch.float64, code_bits=BITS).cpu().numpy()
    want = dec_n.copy()
    for s in range(0, N_ROWS, 512):
        d, idx = odeltas.error_bounded_requirement(10, dec_n[s:s + 512], x_n[s:s + 512])
        odeltas.apply_deltas(want[s:s + 512], d, idx)
    assert np.abs(restored - want[:, fl]).max() < 1e-12
    _, (wr, wc) = odeltas.error_bounded_requirement(10, want[:, fl], x_f)
    assert set(zip(br.tolist(), bc.tolist())) == set(zip(wr.tolist(), wc.tolist()))
