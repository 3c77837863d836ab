"""config.latent_dtype end to end on the GPU: train -> compress -> decompress on a small synthetic 1-D workspace (the one
test_gpu_colstats_cli.py builds) with the key unset, "float16" and "bfloat16"; the archive format and size, decompression against the
Python API on the widened codes, two ranks on one GPU (gloo) against one process, the error-bounded deltas side channel on rounded
codes, the refusal of a model whose latents overflow float16, and one PJ_Conv_AE workspace (2-D data) with float16 codes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_colstats_cli import N_ROWS, REPO, _WORKER, _run, _workspace

pytestmark = pytest.mark.gpu

Z = 15


def _set_config(tmp_path, extra):
    """Rewrite the project's config with other trailing keys (the trained model and the normalisation features stay)."""
    proj = tmp_path / "workspaces" / "CMS_workspace" / "CMS_project_v1"
    src = open(os.path.join(REPO, "workspaces", "CMS_workspace", "CMS_project_v1", "config", "CMS_project_v1_config.py")).read()
    (proj / "config" / "CMS_project_v1_config.py").write_text(src.replace("c.epochs = 25", "c.epochs = 3") + extra)


def _handle(out):
    from baler_amd.modules import data_processing, models
    models.set_default_mode("fp64")          # what the CLI worker computes in
    try:
        model = data_processing.load_model(data_processing.initialise_model("AE"), str(out / "compressed_output" / "model.pt"),
                                           n_features=24, z_dim=Z)
    finally:
        models.set_default_mode("fp32")
    model.eval()
    return model, model.handle()


def _api_decompress(out, codes32):
    """What decompress must write for these (widened) codes: decode + un-normalise with the training features + int truncation."""
    from baler_amd import synth
    model, h = _handle(out)
    nf = np.load(out / "training" / "normalization_features.npy")
    feats = torch.as_tensor(np.asarray(nf, dtype=np.float64).reshape(2, -1)).cuda().contiguous()
    mask = torch.as_tensor(np.array([t == "int" for t in synth.CMS_TYPE_LIST], dtype=np.uint8)).cuda()
    z = torch.from_numpy(np.ascontiguousarray(codes32)).cuda()
    return h.decode(z, features=feats, int_mask=mask, out_dtype=torch.float64).cpu().numpy()


def test_cli_latent_dtype_unset_float16_bfloat16_and_two_ranks(tmp_path):
    from baler_amd import hostio
    out = _workspace(tmp_path)
    comp, dec = out / "compressed_output" / "compressed.npz", out / "decompressed_output" / "decompressed.npz"
    _run(tmp_path, ["train", "compress", "decompress"], 1)
    base = np.load(comp)
    assert base.files == ["data", "names", "normalization_features"]          # unset: the archive of every earlier version
    c64 = base["data"]
    assert c64.dtype == np.float64 and c64.shape == (N_ROWS, Z)
    base_bytes, base_dec = comp.read_bytes(), np.load(dec)["data"]
    np.testing.assert_array_equal(base_dec, _api_decompress(out, c64))
    # unset and an explicit None are the same run, byte for byte
    _set_config(tmp_path, "\n    c.latent_dtype = None\n")
    _run(tmp_path, ["compress"], 1)
    assert comp.read_bytes() == base_bytes

    c32 = c64.astype(np.float32)       # the value the fp64 handle would have stored as float32: the codes are ITS rounding
    with np.errstate(over="ignore"):
        want = {"float16": c32.astype(np.float16).view(np.uint16), "bfloat16": hostio.bf16_bits(c32)}
    wide = {"float16": want["float16"].view(np.float16).astype(np.float32), "bfloat16": hostio.bf16_widen(want["bfloat16"])}
    for name in ("float16", "bfloat16"):
        _set_config(tmp_path, f'\n    c.latent_dtype = "{name}"\n')
        _run(tmp_path, ["compress", "decompress"], 1)
        a = np.load(comp)
        data = a["data"]
        assert data.shape == (N_ROWS, Z) and data.nbytes == N_ROWS * Z * 2
        if name == "float16":
            assert data.dtype == np.float16 and "latent_dtype" not in a.files
        else:
            assert data.dtype == np.uint16 and str(a["latent_dtype"]) == "bfloat16"
        np.testing.assert_array_equal(data.view(np.uint16), want[name])
        assert os.path.getsize(comp) < len(base_bytes) - N_ROWS * Z * 5       # 6 of the 8 bytes per code are gone
        got = np.load(dec)["data"]
        assert got.dtype == base_dec.dtype and got.shape == base_dec.shape
        np.testing.assert_array_equal(got, _api_decompress(out, wide[name]))
        # two ranks on one GPU write the archive and the table one process writes
        one_c, one_d = comp.read_bytes(), dec.read_bytes()
        os.remove(comp)
        os.remove(dec)
        _run(tmp_path, ["compress", "decompress"], 2)
        assert comp.read_bytes() == one_c and dec.read_bytes() == one_d


def test_cli_deltas_on_rounded_codes(tmp_path):
    """save_error_bounded_deltas with 16-bit codes: the side channel is computed from decode() of the ROUNDED codes, so after
    decompression every flagged element is the input up to the float16 rounding of its delta -- the bound check of
    tests/test_gpu_deltas.py (normalised units, float columns)."""
    from baler_amd import synth
    from baler_amd.modules import helper
    from oracle import c_oracle as orc
    out = _workspace(tmp_path)
    _run(tmp_path, ["train"], 1)
    raw = synth.cms_rows(N_ROWS)
    nf, data_n = orc.find_minmax(raw), orc.normalize(raw)
    int_mask = np.array([t == "int" for t in synth.CMS_TYPE_LIST])
    for name in ("float16", "bfloat16"):
        _set_config(tmp_path, f'\n    c.latent_dtype = "{name}"\n    c.save_error_bounded_deltas = True\n    c.error_bounded_requirement = 10\n')
        _run(tmp_path, ["compress", "decompress"], 1)
        rows, cols, vals = helper.load_deltas(str(out / "compressed_output" / "compressed_deltas.npz.gz"),
                                              str(out / "compressed_output" / "compressed_batch_index_metadata.npz.gz"), 512)
        assert len(rows) > 100
        dec = np.load(out / "decompressed_output" / "decompressed.npz")["data"]
        restored_n = (dec[rows, cols] - nf[0][cols]) / nf[1][cols]
        fl = ~int_mask[cols]
        worst = np.abs(restored_n[fl] - data_n[rows, cols][fl]).max()
        print(f"{name}: {len(rows)} deltas, worst |restored - x| at flagged float positions {worst:.3e}")
        assert worst < 1e-3


def test_cli_float16_overflow_is_refused(tmp_path):
    """A model whose latents leave the float16 range: compress fails with the count and the pointer to "bfloat16", and writes no
    archive; the same model compresses with "bfloat16"."""
    out = _workspace(tmp_path, extra='\n    c.latent_dtype = "float16"\n')
    _run(tmp_path, ["train"], 1)
    comp = out / "compressed_output" / "compressed.npz"
    path = out / "compressed_output" / "model.pt"
    sd = torch.load(str(path), map_location="cpu")
    keys = list(sd.keys())
    for k in keys[6:8]:          # the last encoder layer: the latent is linear in it
        sd[k] = sd[k] * 2.0 ** 22
    torch.save(sd, str(path))
    script = tmp_path / "report_worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, REPO=REPO)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "BALER_AMD_DIST_BACKEND", "BALER_AMD_FORCE_DEVICE", "BALER_AMD_FORCE_PG"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, str(script), "compress"], env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode != 0
    assert "float16" in r.stderr and "bfloat16" in r.stderr and "latent codes" in r.stderr, r.stderr[-2000:]
    assert not comp.exists()
    _set_config(tmp_path, '\n    c.latent_dtype = "bfloat16"\n')
    _run(tmp_path, ["compress", "decompress"], 1)
    assert np.load(comp)["data"].dtype == np.uint16
    assert np.isfinite(np.load(out / "decompressed_output" / "decompressed.npz")["data"]).all()


def test_cli_pjconv_float16_round_trips(tmp_path, monkeypatch):
    """PJ_Conv_AE through the CLI (the workspace tests/test_gpu_pjconv_cli.py builds) with c.latent_dtype = "float16": the archive
    holds the float16 rounding of the codes the same run stores without the key (training is bitwise repeatable), n * z * 2 bytes of
    them, and the decompressed frames are decode() of the widened codes with the un-normalise epilogue, cast to float32 as the
    reference's convolutional artefact is."""
    from baler_amd import native
    from test_gpu_pjconv_cli import frames, run_cli
    n, z = 64, int(np.ceil(784 / 20))
    data = frames(n, 28, 1)
    base = run_cli(tmp_path / "a", monkeypatch, data)
    c32 = np.load(base / "compressed_output" / "compressed.npz")["data"]
    assert c32.dtype == np.float32 and c32.shape == (n, z)
    out = run_cli(tmp_path / "b", monkeypatch, data, latent_dtype='"float16"')
    a = np.load(out / "compressed_output" / "compressed.npz")
    c16 = a["data"]
    assert a.files == ["data", "names", "normalization_features"]
    assert c16.dtype == np.float16 and c16.shape == (n, z) and c16.nbytes == n * z * 2
    np.testing.assert_array_equal(c16.view(np.uint16), c32.astype(np.float16).view(np.uint16))
    dec = np.load(out / "decompressed_output" / "decompressed.npz")["data"]
    assert dec.shape == (n, 1, 28, 28) and dec.dtype == np.float32
    sd = torch.load(out / "compressed_output" / "model.pt")
    flat = np.concatenate([v.numpy().ravel() for v in sd.values()] + [np.zeros(1, np.float32)]).astype(np.float32)
    h = native.Handle.pj_conv(z)
    h.load_params(torch.from_numpy(flat).cuda())
    feats = torch.as_tensor(np.load(out / "training" / "normalization_features.npy").astype(np.float64).reshape(2, -1)).cuda().contiguous()
    wide = torch.from_numpy(c16.astype(np.float32)).cuda()
    want = h.decode(wide, features=feats, out_dtype=torch.float64).cpu().numpy().astype(np.float32).reshape(n, 1, 28, 28)
    np.testing.assert_array_equal(dec, want)
    # and it is close to the float32-code run: float16 keeps 11 bits of every code
    ref = np.load(base / "decompressed_output" / "decompressed.npz")["data"]
    assert np.linalg.norm(dec.astype(np.float64) - ref) / np.linalg.norm(ref) < 1e-2
