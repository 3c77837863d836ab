"""config.latent_dtype = "uint8" end to end on the GPU: train -> compress -> decompress on the 3,000-row synthetic CMS table (the
workspace tests/test_gpu_colstats_cli.py builds, 3 epochs): the archive's members and size, model.pt left alone, decompression
against the public Handle API on the same codes and scale, two ranks on one GPU (gloo) against one process, the error-bounded
deltas side channel on the decoded bytes, the refusal of a table without a finite latent range, and one FPGA_prototype_model and one
PJ_Conv_AE round trip."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import free_port
from test_gpu_colstats_cli import N_ROWS, REPO, _workspace

pytestmark = pytest.mark.gpu

Z = 15
CONFIG = os.path.join(REPO, "workspaces", "CMS_workspace", "CMS_project_v1", "config", "CMS_project_v1_config.py")

# the worker of tests/test_gpu_colstats_cli.py with the model's own default init (so that it serves every model class)
_WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["REPO"])
import torch
from baler_amd import baler, dist as bdist
from baler_amd.modules import helper, models
rank, world, local = bdist.init_from_env()
torch.cuda.set_device(local)
models.set_default_mode("fp64")

def factory(name):
    cls = getattr(models, name)
    def make(n_features, z_dim):
        torch.manual_seed(11)
        return cls(n_features, z_dim)
    return make
helper.model_init = factory
for mode in sys.argv[1:]:
    baler.main(["--project", "CMS_workspace", "CMS_project_v1", "--mode", mode])
bdist.barrier()
'''


def _run(tmp_path, modes, ranks=1, check=True):
    script = tmp_path / "latent8_worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, REPO=REPO)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "BALER_AMD_DIST_BACKEND", "BALER_AMD_FORCE_DEVICE", "BALER_AMD_FORCE_PG"):
        env.pop(k, None)
    if ranks == 1:
        cmd = [sys.executable, str(script)] + modes
    else:
        env.update(BALER_AMD_FORCE_DEVICE="0", BALER_AMD_DIST_BACKEND="gloo")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}", "--master-addr", "127.0.0.1",
               "--master-port", str(free_port()), str(script)] + modes
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    if check:
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _set_config(tmp_path, extra, model="AE"):
    proj = tmp_path / "workspaces" / "CMS_workspace" / "CMS_project_v1"
    src = open(CONFIG).read().replace("c.epochs = 25", "c.epochs = 3")
    if model != "AE":
        src = src.replace('c.model_name = "AE"', f'c.model_name = "{model}"').replace("c.activation_extraction = True", "c.activation_extraction = False")
        assert f'c.model_name = "{model}"' in src
    (proj / "config" / "CMS_project_v1_config.py").write_text(src + extra)


def _folded_handle(out, scale, model_name="AE"):
    """The public API's side of decompress: the model of model.pt in the CLI worker's mode, the archive's scale folded in."""
    from baler_amd import latent8
    from baler_amd.modules import data_processing, models
    models.set_default_mode("fp64")
    try:
        model = data_processing.load_model(data_processing.initialise_model(model_name), str(out / "compressed_output" / "model.pt"),
                                           n_features=24, z_dim=Z)
    finally:
        models.set_default_mode("fp32")
    model.eval()
    model.load_flat(latent8.fold(model, scale[0], scale[1]))
    return model, model.handle()


def _renorm(out):
    from baler_amd import synth
    nf = np.load(out / "training" / "normalization_features.npy")
    feats = torch.as_tensor(np.asarray(nf, dtype=np.float64).reshape(2, -1)).cuda().contiguous()
    mask = torch.as_tensor(np.array([t == "int" for t in synth.CMS_TYPE_LIST], dtype=np.uint8)).cuda()
    return feats, mask


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _check_archive(comp):
    a = np.load(comp)
    assert sorted(a.files) == ["data", "latent_dtype", "latent_scale", "names", "normalization_features"]
    data, scale = a["data"], a["latent_scale"]
    assert data.dtype == np.uint8 and data.shape == (N_ROWS, Z) and data.nbytes == N_ROWS * Z
    assert str(a["latent_dtype"]) == "uint8"
    assert scale.dtype == np.float64 and scale.shape == (2, Z) and np.isfinite(scale).all() and (scale[1] > 0).all()
    assert data.min() == 0 and data.max() == 255          # the calibration is the table's own extrema: both ends are reached
    assert (data.min(axis=0) == 0).all() and (data.max(axis=0) == 255).all()
    return data, scale


def test_cli_uint8_archive_model_file_decompression_and_two_ranks(tmp_path):
    out = _workspace(tmp_path)
    comp, dec = out / "compressed_output" / "compressed.npz", out / "decompressed_output" / "decompressed.npz"
    model_pt = out / "compressed_output" / "model.pt"
    _set_config(tmp_path, "")
    _run(tmp_path, ["train", "compress", "decompress"])
    base_size, base_dec = os.path.getsize(comp), np.load(dec)["data"]          # codes at the working precision (float64 here)
    _set_config(tmp_path, '\n    c.latent_dtype = "float16"\n')
    _run(tmp_path, ["compress", "decompress"])
    f16_size, f16_dec = os.path.getsize(comp), np.load(dec)["data"]
    model_bytes = model_pt.read_bytes()

    _set_config(tmp_path, '\n    c.latent_dtype = "uint8"\n')
    _run(tmp_path, ["compress"])
    assert model_pt.read_bytes() == model_bytes, "compress changed model.pt"
    _run(tmp_path, ["decompress"])
    assert model_pt.read_bytes() == model_bytes, "decompress changed model.pt"
    data, scale = _check_archive(comp)
    u8_size = os.path.getsize(comp)
    print(f"compressed.npz: {base_size} bytes with float64 codes, {f16_size} with float16, {u8_size} with uint8")
    assert u8_size < f16_size - N_ROWS * Z // 2 < base_size         # most of the second byte per code is gone (the scale costs 240 bytes)

    # the decompressed table is what the public API gives for the same codes, scale and renorm, bit for bit
    got = np.load(dec)["data"]
    assert got.dtype == base_dec.dtype and got.shape == base_dec.shape
    model, h = _folded_handle(out, scale)
    feats, mask = _renorm(out)
    want = h.decode(torch.from_numpy(data).cuda(), features=feats, int_mask=mask, out_dtype=torch.float64).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    # the scale is the extrema of the float32 latent of the unfolded model over the table (compress's first pass)
    from baler_amd import synth
    from baler_amd.modules import data_processing, models
    models.set_default_mode("fp64")
    try:
        plain = data_processing.load_model(data_processing.initialise_model("AE"), str(model_pt), n_features=24, z_dim=Z)
    finally:
        models.set_default_mode("fp32")
    x = torch.from_numpy(synth.cms_rows(N_ROWS)).cuda()
    from baler_amd import native
    z32 = plain.handle().encode(x, features=native.minmax(x), out_dtype=torch.float32).double().cpu().numpy()
    np.testing.assert_array_equal(scale, np.stack([z32.min(axis=0), z32.max(axis=0) - z32.min(axis=0)]))
    # ... and the codes are the folded handle's
    np.testing.assert_array_equal(h.encode(x, features=native.minmax(x), out_dtype=torch.uint8).cpu().numpy(), data)

    # quality, recorded and not asserted (profiles/latent8_quality.json holds the C1 figures)
    print(f"rel-L2 distance from the decompression of float64 codes: uint8 codes {_rel(got, base_dec):.3e}, float16 codes {_rel(f16_dec, base_dec):.3e}")

    # two ranks on one GPU write the archive and the table one process writes
    one_c, one_d = comp.read_bytes(), dec.read_bytes()
    os.remove(comp)
    os.remove(dec)
    _run(tmp_path, ["compress", "decompress"], ranks=2)
    two = np.load(comp)
    assert two["data"].tobytes() == data.tobytes() and two["latent_scale"].tobytes() == scale.tobytes()
    assert comp.read_bytes() == one_c and dec.read_bytes() == one_d
    assert model_pt.read_bytes() == model_bytes

    # extra_compression: the same members through np.savez_compressed
    _set_config(tmp_path, '\n    c.latent_dtype = "uint8"\n    c.extra_compression = True\n')
    _run(tmp_path, ["compress", "decompress"])
    data_x, scale_x = _check_archive(comp)
    assert data_x.tobytes() == data.tobytes() and scale_x.tobytes() == scale.tobytes()
    np.testing.assert_array_equal(np.load(dec)["data"], got)


def test_cli_deltas_on_the_decoded_bytes(tmp_path):
    """save_error_bounded_deltas with uint8 codes: the side channel is computed from decode() of the BYTES on the folded handle,
    which is what decompress decodes, so the bound holds after decompression.  Stated with oracle/deltas.py on the float columns
    of the normalised table (the int columns are truncated after un-normalisation):

    * every element with |x| >= 0.02 meets the 10 % bound.  Below that the reference's float16 deltas cannot restore it: a delta is
      float16(float16(decoded) - float16(x)), an absolute error of up to about 2^-11 (|decoded| + |x|) + 2^-11 |decoded - x| <= 2e-3
      for normalised values, which is 10 % of 0.02.  (On the fp64 oracle alone, formula parameters seed 5, the side channel leaves 9
      of 65,699 flagged elements above the bound, all with |x| <= 2.2e-4.)
    * the elements that remain above the bound are exactly those that oracle/deltas.py's own side channel leaves above it when it
      is given the same decoded table."""
    from baler_amd import synth
    from baler_amd.modules import helper
    from oracle import c_oracle as orc
    from oracle import deltas as odeltas
    out = _workspace(tmp_path)
    _set_config(tmp_path, '\n    c.latent_dtype = "uint8"\n    c.save_error_bounded_deltas = True\n    c.error_bounded_requirement = 10\n')
    _run(tmp_path, ["train", "compress", "decompress"])
    data, scale = _check_archive(out / "compressed_output" / "compressed.npz")
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
    # the oracle's side channel on the same decoded table (decode of the bytes, normalised units)
    model, h = _folded_handle(out, scale)
    dec_n = h.decode(torch.from_numpy(data).cuda(), out_dtype=torch.float64).cpu().numpy()
    want = dec_n.copy()
    for s in range(0, N_ROWS, 512):
        d, idx = odeltas.error_bounded_requirement(10, dec_n[s:s + 512], x_n[s:s + 512])
        odeltas.apply_deltas(want[s:s + 512], d, idx)
    assert np.abs(restored - want[:, fl]).max() < 1e-12
    _, (wr, wc) = odeltas.error_bounded_requirement(10, want[:, fl], x_f)
    assert set(zip(br.tolist(), bc.tolist())) == set(zip(wr.tolist(), wc.tolist()))


def test_cli_non_finite_calibration_is_refused(tmp_path):
    """A table with a NaN row has no finite latent range: compress raises ValueError naming latent_dtype = "uint8" and writes
    no archive."""
    from baler_amd import synth
    out = _workspace(tmp_path, extra='\n    c.latent_dtype = "uint8"\n')
    _run(tmp_path, ["train"])
    comp = out / "compressed_output" / "compressed.npz"
    raw = synth.cms_rows(N_ROWS)
    raw[1234, :] = np.nan
    np.savez(tmp_path / "workspaces" / "CMS_workspace" / "data" / "example_CMS_data.npz", data=raw, names=synth.CMS_NAMES)
    for ranks in (1, 2):
        r = _run(tmp_path, ["compress"], ranks=ranks, check=False)
        assert r.returncode != 0
        assert "ValueError" in r.stderr and "uint8" in r.stderr and "non-finite" in r.stderr, r.stderr[-2000:]
        assert not comp.exists()


def test_cli_fpga_prototype_model_round_trips(tmp_path):
    from baler_amd import latent8, native, synth
    from baler_amd.modules import models
    out = _workspace(tmp_path)
    _set_config(tmp_path, '\n    c.latent_dtype = "uint8"\n', model="FPGA_prototype_model")
    _run(tmp_path, ["train", "compress", "decompress"])
    data, scale = _check_archive(out / "compressed_output" / "compressed.npz")
    sd = torch.load(out / "compressed_output" / "model.pt")
    m = models.FPGA_prototype_model(24, Z, mode="fp64")
    m.load_state_dict(sd)
    m.to("cuda")
    m.load_flat(latent8.fold(m, scale[0], scale[1]))
    feats, mask = _renorm(out)
    want = m.handle().decode(torch.from_numpy(data).cuda(), features=feats, int_mask=mask, out_dtype=torch.float64).cpu().numpy()
    got = np.load(out / "decompressed_output" / "decompressed.npz")["data"]
    np.testing.assert_array_equal(got, want)
    x = torch.from_numpy(synth.cms_rows(N_ROWS)).cuda()
    np.testing.assert_array_equal(m.handle().encode(x, features=native.minmax(x), out_dtype=torch.uint8).cpu().numpy(), data)


def test_cli_pjconv_round_trips(tmp_path, monkeypatch):
    """PJ_Conv_AE through the CLI (the workspace tests/test_gpu_pjconv_cli.py builds): uint8 codes beside the float32-code run of the
    same training (bitwise repeatable); the frames are decode() of the bytes on the folded model, cast to float32."""
    from baler_amd import latent8, native
    from baler_amd.modules import models
    from test_gpu_pjconv_cli import frames, run_cli
    n, z = 64, int(np.ceil(784 / 20))
    data = frames(n, 28, 1)
    base = run_cli(tmp_path / "a", monkeypatch, data)
    c32 = np.load(base / "compressed_output" / "compressed.npz")["data"]
    model_bytes = (base / "compressed_output" / "model.pt").read_bytes()
    out = run_cli(tmp_path / "b", monkeypatch, data, latent_dtype='"uint8"')
    assert (out / "compressed_output" / "model.pt").read_bytes() == model_bytes
    a = np.load(out / "compressed_output" / "compressed.npz")
    q, scale = a["data"], a["latent_scale"]
    assert q.dtype == np.uint8 and q.shape == (n, z) and q.nbytes == n * z and str(a["latent_dtype"]) == "uint8"
    np.testing.assert_array_equal(scale, np.stack([c32.min(axis=0).astype(np.float64), c32.max(axis=0).astype(np.float64) - c32.min(axis=0)]))
    err = np.abs(latent8.unscale(q, scale[0], scale[1]) - c32) / np.where(scale[1] > 0, scale[1] / 255.0, 1.0)
    print(f"PJ_Conv_AE: worst |q / s + lo - z32| = {err.max():.4f} steps")
    assert (err <= 0.51).all()
    m = models.PJ_Conv_AE(784, z, mode="fp32")
    m.load_state_dict(torch.load(out / "compressed_output" / "model.pt"))
    m.to("cuda")
    m.load_flat(latent8.fold(m, scale[0], scale[1]))
    feats = torch.as_tensor(np.load(out / "training" / "normalization_features.npy").astype(np.float64).reshape(2, -1)).cuda().contiguous()
    want = m.handle().decode(torch.from_numpy(q).cuda(), features=feats, out_dtype=torch.float64).cpu().numpy().astype(np.float32)
    dec = np.load(out / "decompressed_output" / "decompressed.npz")["data"]
    assert dec.shape == (n, 1, 28, 28) and dec.dtype == np.float32
    np.testing.assert_array_equal(dec, want.reshape(n, 1, 28, 28))
    ref = np.load(base / "decompressed_output" / "decompressed.npz")["data"]
    print(f"PJ_Conv_AE: rel-L2 of the uint8-code frames from the float32-code frames {_rel(dec.astype(np.float64), ref.astype(np.float64)):.3e}")
