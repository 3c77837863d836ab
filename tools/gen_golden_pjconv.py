#!/usr/bin/env python3
"""Generate tests/golden/g19_pjconv.npz and g20_pjconv_cli.npz by IMPORTING the reference (authoring machine only).

Run:  python tools/gen_golden_pjconv.py <reference checkout>

Writes data only.  While generating it checks tests/pjconv_ref.py (the float64 restatement the tests use) against the live
reference PJ_Conv_AE and aborts if they disagree.  Same ReduceLROnPlateau(verbose=...) shim as tools/gen_golden.py.

Contents: seed, z, a batch of 16 frames; the reference's z, recon and loss; the full gradients of the four convolution tensors and
of every bias; fixed-index samples plus norms of the gradients of the four Linear weights; the same digests of the parameters after 3
Adam steps (lr 1e-3; the two 25,000-element convolution weights sampled too); per-tensor samples and sums of the seeded init.
g20: digests of two short runs of the reference CLI (train / compress / decompress) with model_name = "PJ_Conv_AE": run "norm" on 64
frames of 28 x 28 with apply_normalization, run "blocks" on 16 frames of 56 x 56 cut into 28 x 28 blocks without normalisation.  The
frames are np.random.default_rng(seed).random(shape) * 5 - 1 in float32 (the tests draw the same), the model is built under
torch.manual_seed(7).
"""
import os
import shutil
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")

import numpy as np  # noqa: E402
import torch  # noqa: E402

_RLROP = torch.optim.lr_scheduler.ReduceLROnPlateau


class _RLROPShim(_RLROP):
    def __init__(self, *a, verbose=None, **k):
        super().__init__(*a, **k)


torch.optim.lr_scheduler.ReduceLROnPlateau = _RLROPShim

SEED, Z, ROWS, LR = 19, 40, 16, 1e-3
LINEAR = ("encoder.4.weight", "encoder.5.weight", "decoder.0.weight", "decoder.2.weight")
N_SAMPLES = 256


def check(name, got, want, tol, l2=False):
    import pjconv_ref
    r = pjconv_ref.rel(got, want)
    if l2:      # Adam's first steps move every parameter by ~lr whatever the size of its gradient: elements whose float32 and float64
        # gradients sit at the 1e-8 eps scale take visibly different steps, so the parameters are compared in rel-L2
        r = float(np.linalg.norm(np.asarray(got, np.float64) - want) / np.linalg.norm(np.asarray(want, np.float64)))
    print(f"  {name}: rel {r:.3e} (tol {tol:.0e})")
    if not r <= tol:
        raise SystemExit(f"restatement disagrees with the reference: {name}")


def digest(prefix, sd, out, full_max=None):
    """full small tensors; samples + L2 norm of the Linear weights (and of every tensor above full_max elements)"""
    rng = np.random.default_rng(1234)
    for k, v in sd.items():
        a = v.detach().numpy().astype(np.float32).ravel()
        if k in LINEAR or (full_max is not None and a.size > full_max):
            idx = np.sort(rng.choice(a.size, N_SAMPLES, replace=False))
            out[f"{prefix}{k}.idx"] = idx.astype(np.int64)
            out[f"{prefix}{k}.sample"] = a[idx]
            out[f"{prefix}{k}.norm"] = np.float64(np.linalg.norm(a.astype(np.float64)))
        else:
            out[f"{prefix}{k}"] = a


def main(ref):
    sys.path.insert(0, ref)
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from baler.modules import models as ref_models
    from baler.modules import utils as ref_utils

    import pjconv_ref
    from baler_amd.modules import models

    torch.set_num_threads(8)
    out = {"seed": np.int64(SEED), "z_dim": np.int64(Z)}
    torch.manual_seed(SEED)
    model = ref_models.PJ_Conv_AE(784, Z)
    sd = model.state_dict()
    init = np.concatenate([v.detach().numpy().ravel() for v in sd.values()])
    print(f"PJ_Conv_AE(z={Z}): {init.size} parameters")
    assert init.size == 2504541 + 1001 * Z
    torch.manual_seed(SEED)
    mine = models.pj_conv_init(Z).numpy()
    if not np.array_equal(mine, init):
        raise SystemExit("models.pj_conv_init does not reproduce the reference's seeded init")
    out["keys"] = np.array(list(sd.keys()))
    out["shapes"] = np.array([list(t.shape) + [0] * (4 - t.dim()) for t in sd.values()])
    out["dtypes"] = np.array([str(t.dtype) for t in sd.values()])
    for k, v in sd.items():
        a = v.detach().numpy().ravel()
        out[f"init.{k}.head"] = a[:32].copy()
        out[f"init.{k}.sum"] = np.float64(a.astype(np.float64).sum())

    rng = np.random.default_rng(SEED)
    x = rng.random((ROWS, 1, 28, 28)).astype(np.float32)
    out["x"] = x.reshape(ROWS, 784)
    xt = torch.as_tensor(x)
    with torch.no_grad():
        z_ref = model.encode(xt).numpy()
        r_ref = model(xt).numpy()
    check("encode", pjconv_ref.encode(Z, init, x), z_ref, 2e-6)
    check("forward", pjconv_ref.forward(Z, init, x), r_ref.reshape(ROWS, 784), 2e-6)
    out["z"] = z_ref
    out["recon"] = r_ref.reshape(ROWS, 784)

    opt = torch.optim.Adam(model.parameters(), lr=LR)
    p, m, v = init.astype(np.float64), np.zeros(init.size), np.zeros(init.size)
    for step in (1, 2, 3):
        opt.zero_grad()
        recon = model(xt)
        loss, _, _ = ref_utils.mse_sum_loss_l1(model_children=list(model.children()), true_data=xt, reconstructed_data=recon,
                                            reg_param=0.001, validate=True)
        loss.backward()
        g_ref = np.concatenate([q.grad.numpy().ravel() for q in model.parameters()])
        l_me, g_me = pjconv_ref.fwd_bwd(Z, p, x)
        check(f"loss step {step}", l_me, loss.item(), 2e-6)
        check(f"gradient step {step}", g_me, g_ref, 1e-4)
        if step == 1:
            out["loss"] = np.float64(loss.item())
            digest("grad.", {k: q.grad for k, q in zip(sd.keys(), model.parameters())}, out)
        opt.step()
        pjconv_ref.adam_step(p, g_me, m, v, step, LR)
        check(f"params after step {step}", p, np.concatenate([q.detach().numpy().ravel() for q in model.parameters()]), 1e-5,
              l2=True)
    digest("p3.", model.state_dict(), out, full_max=4096)
    out["lr"] = np.float64(LR)
    np.savez_compressed(os.path.join(OUT, "g19_pjconv.npz"), **out)
    print("wrote g19_pjconv.npz", os.path.getsize(os.path.join(OUT, "g19_pjconv.npz")), "bytes")


CLI_BASE = dict(data_dimension="2", compression_ratio="20", apply_normalization="True", model_name='"PJ_Conv_AE"',
                model_type='"convolutional"', epochs="3", lr="0.001", batch_size="16", early_stopping="False", lr_scheduler="True",
                early_stopping_patience="100", min_delta="0", lr_scheduler_patience="50", custom_norm="False", reg_param="0.001",
                RHO="0.05", test_size="0", extra_compression="False", intermittent_model_saving="False",
                intermittent_saving_patience="100", mse_avg="False", mse_sum="True", emd="False", l1="True",
                activation_extraction="False", deterministic_algorithm="True", separate_model_saving="False",
                save_error_bounded_deltas="False", error_bounded_requirement="10", convert_to_blocks="False")
CLI_RUNS = {"norm": dict(n=64, hw=28, seed=1, cfg={}),
            "blocks": dict(n=16, hw=56, seed=2, cfg=dict(apply_normalization="False", convert_to_blocks="[1, 28, 28]", epochs="2"))}


def cli_frames(n, hw, seed):
    return (np.random.default_rng(seed).random((n, hw, hw)) * 5.0 - 1.0).astype(np.float32)


def gen_cli(ref):
    from baler import baler as ref_baler
    from baler.modules import helper as ref_helper
    from baler.modules import models as ref_models

    def factory(name):
        def make(n_features, z_dim):
            torch.manual_seed(7)
            return ref_models.PJ_Conv_AE(n_features, z_dim)
        return make
    ref_helper.model_init = factory
    out = {}
    for tag, run in CLI_RUNS.items():
        scratch = tempfile.mkdtemp(prefix="baler_golden_pjconv_")
        os.chdir(scratch)
        ws = os.path.join(scratch, "workspaces")
        proj = os.path.join(ws, "W", "P")
        for d in ("config", "output/compressed_output", "output/decompressed_output", "output/plotting", "output/training"):
            os.makedirs(os.path.join(proj, d), exist_ok=True)
        os.makedirs(os.path.join(ws, "W", "data"), exist_ok=True)
        for d in (ws, os.path.join(ws, "W"), proj, os.path.join(proj, "config")):
            open(os.path.join(d, "__init__.py"), "w").close()
        data = cli_frames(run["n"], run["hw"], run["seed"])
        np.savez(os.path.join(ws, "W", "data", "d.npz"), data=data, names=np.array(["frame"]))
        cfg = dict(CLI_BASE, input_path='"workspaces/W/data/d.npz"', **run["cfg"])
        with open(os.path.join(proj, "config", "P_config.py"), "w") as f:
            f.write("def set_config(c):\n" + "".join(f"    c.{k} = {v}\n" for k, v in cfg.items()))
        sys.path.insert(0, scratch)
        for k in [k for k in sys.modules if k == "workspaces" or k.startswith("workspaces.")]:
            del sys.modules[k]
        outp = os.path.join(proj, "output")
        for mode in ("train", "compress", "decompress"):
            sys.argv = ["baler", "--project", "W", "P", "--mode", mode]
            ref_baler.main()
        sys.path.remove(scratch)
        sd = torch.load(os.path.join(outp, "compressed_output", "model.pt"))
        flat = np.concatenate([v.numpy().ravel() for v in sd.values()])
        comp = np.load(os.path.join(outp, "compressed_output", "compressed.npz"))["data"]
        dec = np.load(os.path.join(outp, "decompressed_output", "decompressed.npz"))["data"]
        fl = np.load(os.path.join(outp, "training", "final_layer.npy"), allow_pickle=True)
        idx = np.sort(np.random.default_rng(20).choice(flat.size, size=1024, replace=False))
        out.update({f"{tag}.loss_data": np.load(os.path.join(outp, "training", "loss_data.npy")),
                    f"{tag}.final_sample_idx": idx, f"{tag}.final_sample": flat[idx],
                    f"{tag}.final_l2": np.float64(np.linalg.norm(flat.astype(np.float64))),
                    f"{tag}.compressed": comp, f"{tag}.compressed_dtype": np.array(str(comp.dtype)),
                    f"{tag}.decompressed_shape": np.array(dec.shape), f"{tag}.decompressed_dtype": np.array(str(dec.dtype)),
                    f"{tag}.decompressed_head": dec[:2], f"{tag}.decompressed_sum0": dec.astype(np.float64).sum(axis=0),
                    f"{tag}.final_layer": np.array(type(fl.item()).__name__), f"{tag}.keys": np.array(list(sd.keys()))})
        if tag == "norm":
            out["norm.normalization_features"] = np.load(os.path.join(outp, "training", "normalization_features.npy"))
        print(f"CLI run {tag}: compressed {comp.shape} {comp.dtype}, decompressed {dec.shape} {dec.dtype}, "
              f"final layer {type(fl.item()).__name__}")
        shutil.rmtree(scratch, ignore_errors=True)
    np.savez_compressed(os.path.join(OUT, "g20_pjconv_cli.npz"), **out)
    print("wrote g20_pjconv_cli.npz", os.path.getsize(os.path.join(OUT, "g20_pjconv_cli.npz")), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(os.path.abspath(sys.argv[1]))
    gen_cli(os.path.abspath(sys.argv[1]))
