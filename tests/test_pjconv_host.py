"""PJ_Conv_AE without a GPU: state-dict keys, shapes, dtype and the seeded init against the reference fixture g19, the model lookup,
model.pt and encoder.pt / decoder.pt round trips, the float64 restatement against g19, the C header, and the convolutional
configurations the CLI refuses before any GPU work."""
import os
import types

import numpy as np
import pytest
import torch

import pjconv_ref
from pjconv_ref import rel
from baler_amd import native
from baler_amd.modules import data_processing, helper, models

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def seeded(g):
    torch.manual_seed(int(g["seed"]))
    return models.PJ_Conv_AE(784, int(g["z_dim"]))


def test_state_dict_keys_shapes_dtype_and_seeded_init(golden):
    g = golden("g19_pjconv.npz")
    m = seeded(g)
    sd = m.state_dict()
    assert list(sd.keys()) == list(g["keys"])
    for t, shape, dt in zip(sd.values(), g["shapes"], g["dtypes"]):
        assert tuple(t.shape) == tuple(int(s) for s in shape if s)
        assert str(t.dtype) == str(dt) == "torch.float32"
    for k, t in sd.items():
        a = t.numpy().ravel()
        np.testing.assert_array_equal(a[:32], g[f"init.{k}.head"])
        assert a.astype(np.float64).sum() == pytest.approx(float(g[f"init.{k}.sum"]), rel=1e-12, abs=1e-12)
    assert m.nparams == 2504541 + 1001 * int(g["z_dim"]) == pjconv_ref.nparams(int(g["z_dim"]))
    assert not m.supports_activation_extraction
    with pytest.raises(NotImplementedError):
        m.store_hooks()


def test_initialise_model_resolves():
    assert data_processing.initialise_model("PJ_Conv_AE") is models.PJ_Conv_AE
    m = models.PJ_Conv_AE(n_features=28, z_dim=157)      # the reference passes the frame width, which the model ignores
    assert m.z_dim == 157 and m.dims == [784, 157, 784]
    for bad in (0, 2451):
        with pytest.raises(ValueError):
            models.PJ_Conv_AE(784, bad)
    with pytest.raises(NotImplementedError, match="float32"):
        models.PJ_Conv_AE(784, 10, mode="fp64")


def test_model_pt_and_separate_files_round_trip(tmp_path):
    torch.manual_seed(3)
    a = models.PJ_Conv_AE(784, 9)
    data_processing.save_model(a, str(tmp_path / "model.pt"))
    torch.manual_seed(4)
    b = models.PJ_Conv_AE(784, 9)
    assert not torch.equal(a.flat, b.flat)
    b.load_state_dict(torch.load(str(tmp_path / "model.pt")), strict=False)
    assert torch.equal(a.flat, b.flat)
    enc, dec = a.encoder_state_dict(), a.decoder_state_dict()
    assert list(enc) == ["0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias", "5.weight", "5.bias"]
    assert list(dec) == ["0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias", "5.weight", "5.bias"]
    torch.save(enc, str(tmp_path / "encoder.pt"))
    torch.save(dec, str(tmp_path / "decoder.pt"))
    torch.manual_seed(5)
    c = models.PJ_Conv_AE(784, 9)
    c.load_part_state_dict("encoder", torch.load(str(tmp_path / "encoder.pt")))
    n_enc = sum(v.numel() for v in enc.values())
    assert torch.equal(c.flat[:n_enc], a.flat[:n_enc]) and not torch.equal(c.flat[n_enc:-1], a.flat[n_enc:-1])
    c.load_part_state_dict("decoder", torch.load(str(tmp_path / "decoder.pt")))
    assert torch.equal(c.flat, a.flat)


def test_restatement_reproduces_fixture(golden):
    g = golden("g19_pjconv.npz")
    z = int(g["z_dim"])
    init = seeded(g).flat[:-1].numpy().astype(np.float64)
    x = g["x"]
    assert rel(pjconv_ref.encode(z, init, x), g["z"]) <= 2e-6
    assert rel(pjconv_ref.forward(z, init, x), g["recon"]) <= 2e-6
    l, gr = pjconv_ref.fwd_bwd(z, init, x)
    assert l == pytest.approx(float(g["loss"]), rel=2e-6)
    for k, off, shape in pjconv_ref.layout(z)[0]:
        a = gr[off:off + int(np.prod(shape))]
        if f"grad.{k}" in g.files:
            assert rel(a, g[f"grad.{k}"]) <= 1e-5, k
        else:
            assert rel(a[g[f"grad.{k}.idx"]], g[f"grad.{k}.sample"]) <= 1e-5, k


def test_header_declares_create_pjconv():
    with open(os.path.join(REPO, "include", "baler_amd.h")) as f:
        src = f.read()
    assert "int bamd_create_pjconv(int z_dim, int mode, int device, bamd_handle **out);" in src
    assert "bamd_create_pjconv" in native.SYMBOLS


def conv_config(tmp_path, shape=(8, 28, 28), **over):
    np.savez(str(tmp_path / "d.npz"), data=np.zeros(shape, np.float32), names=np.array(["x"]))
    c = types.SimpleNamespace(input_path=str(tmp_path / "d.npz"), data_dimension=2, model_type="convolutional",
                              model_name="PJ_Conv_AE", convert_to_blocks=False, apply_normalization=True,
                              save_error_bounded_deltas=False, custom_loss_function=None)
    for k, v in over.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize("over, match", [
    (dict(model_name="Conv_AE"), "out of scope"),
    (dict(model_name="TransformerAE"), "out of scope"),
    (dict(shape=(8, 32, 32)), "28 x 28"),
    (dict(shape=(8, 56, 56), convert_to_blocks=[1, 14, 14], apply_normalization=False), "28 x 28"),
    (dict(custom_loss_function="loss_function_swae"), "Wasserstein"),
    (dict(save_error_bounded_deltas=True), "error-bounded"),
    (dict(shape=(4, 56, 56), convert_to_blocks=[1, 28, 28]), "broadcast"),
])
def test_refusals_raise_before_gpu_work(tmp_path, over, match, monkeypatch):
    monkeypatch.setattr(native, "require_gpu", lambda: pytest.fail("GPU touched before the refusal"))
    shape = over.pop("shape", (8, 28, 28))
    c = conv_config(tmp_path, shape, **over)
    from baler_amd import baler
    for run in (baler.perform_training, baler.perform_compression, baler.perform_decompression):
        with pytest.raises(NotImplementedError, match=match):
            run(str(tmp_path), c, False)


def test_fp64_mode_refused(tmp_path, monkeypatch):
    monkeypatch.setattr(native, "require_gpu", lambda: pytest.fail("GPU touched before the refusal"))
    monkeypatch.setattr(models, "_DEFAULT_MODE", "fp64")
    with pytest.raises(NotImplementedError, match="float32"):
        helper.check_convolutional(conv_config(tmp_path))


def test_blocked_56_frames_accepted_without_normalisation(tmp_path):
    helper.check_convolutional(conv_config(tmp_path, (4, 56, 56), convert_to_blocks=[1, 28, 28], apply_normalization=False))
