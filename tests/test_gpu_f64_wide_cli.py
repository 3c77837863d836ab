"""The fp64 default mode end to end on a wide 2-D field: train -> compress -> decompress of a 30 x 30 field (CFD_dense_AE(900, 9),
100 frames, batches of 45 + 45 + 10) through the CLI, as test_cli_cfd_dense_2d_class_shape runs it in the fp32 mode.  Training runs on
the layer-wise fp64 kernels, compress and decompress on the fused fp64 wide kernels (fused64w.hip); the artefacts are compared with
the fp64 checker replaying the same run.

Bar 1e-9: what test_layerwise_path_at_the_references_batch_sizes_fp64 holds parameters to after optimiser steps.  2-D data is
float32 in the archives (as the fp32 run writes it: the reference casts 2-D data to float32 behind the normalisation) and so is the
checkpoint of CFD_dense_AE, so parameters, codes and reconstruction are compared with the checker's values rounded to float32 at the
same places: a difference then is a last-bit flip of a value that sits on a float32 rounding boundary, 6e-8 / sqrt(values) in rel-L2,
below the bar at these sizes."""
import numpy as np
import pytest
import torch

from baler_amd import synth
from oracle import c_oracle as orc
from test_gpu_cli import _CFD_CONFIG, _write_project, rel

pytestmark = pytest.mark.gpu


def test_cli_fp64_mode_wide_field(tmp_path, monkeypatch, capfd):
    from baler_amd import baler
    from baler_amd.modules import helper, models
    monkeypatch.delenv("BALER_AMD_QUIET", raising=False)
    monkeypatch.delenv("BALER_AMD_F64_WIDE", raising=False)
    field = synth.cfd_field(100, 30, 30)
    cfg = _CFD_CONFIG.replace("c.batch_size = 6000", "c.batch_size = 45").replace("c.epochs = 3", "c.epochs = 2")
    out = _write_project(tmp_path, monkeypatch, "CFD", "anim", cfg, field, np.array([]))
    dims = orc.ae_dims(900, 9)
    init = orc.formula_params(dims, 80)
    models.set_default_mode("fp64")
    try:
        monkeypatch.setattr(helper, "model_init",
                            lambda name: (lambda n_features, z_dim: getattr(models, name)(n_features, z_dim).load_flat(init)))
        capfd.readouterr()
        for mode in ("train", "compress", "decompress"):
            baler.main(["--project", "CFD", "anim", "--mode", mode])
    finally:
        models.set_default_mode("fp32")
    err = capfd.readouterr().err
    assert "has fused encode / decode / validation kernels only" in err and "no fused kernel instantiation" not in err, err[-2000:]
    x = field.astype(np.float32).astype(np.float64).reshape(100, 900)
    st = orc.FitState(dims, init)
    want = [orc.fit_epoch(st, x, 45, 1e-3)[0] for _ in range(2)]
    loss = np.load(out / "training" / "loss_data.npy")
    sd = torch.load(out / "compressed_output" / "model.pt")
    assert tuple(sd["en1.weight"].shape) == (200, 900) and tuple(sd["en4.weight"].shape) == (9, 50)
    final = np.concatenate([v.numpy().ravel().astype(np.float64) for v in sd.values()])
    comp = np.load(out / "compressed_output" / "compressed.npz")
    dec = np.load(out / "decompressed_output" / "decompressed.npz")["data"]
    # the replay saves its checkpoint as the run does: CFD_dense_AE's state dict is float32 (the reference's format), and compress /
    # decompress compute in float64 on what they load from it
    saved = st.params.astype(np.float32).astype(np.float64)
    z_want = orc.encode(dims, saved, x).astype(np.float32)
    rec_want = orc.decode(dims, saved, comp["data"].astype(np.float64)).astype(np.float32)
    print(f"fp64 CLI run of CFD_dense_AE(900, 9): loss {rel(loss[0], want):.3e}, parameters {rel(final, saved):.3e}, "
          f"codes {rel(comp['data'], z_want):.3e}, reconstruction {rel(dec.reshape(100, 900), rec_want):.3e}")
    assert rel(loss[0], want) < 1e-9
    assert sd["en1.weight"].dtype == torch.float32 and rel(final, saved) < 1e-9
    assert comp["data"].shape == (100, 9) and comp["data"].dtype == np.float32
    assert rel(comp["data"], z_want) < 1e-9
    assert dec.shape == (100, 30, 30) and dec.dtype == np.float32
    assert rel(dec.reshape(100, 900), rec_want) < 1e-9
