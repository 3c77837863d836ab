#!/usr/bin/env python3
"""Generate tests/golden/g17_fpga.npz and g18_fpga_cli.npz by IMPORTING the reference (authoring machine only).

Run:  python tools/gen_golden_fpga.py <reference checkout>

Writes data only.  While generating it checks tests/fpga_ref.py (the NumPy restatement the tests use) against the live
reference FPGA_prototype_model and aborts if they disagree.  Same ReduceLROnPlateau(verbose=...) shim as tools/gen_golden.py.
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


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def check(name, got, want, tol):
    r = rel(got, want)
    print(f"  {name}: rel {r:.3e} (tol {tol:.0e})")
    if not r <= tol:
        raise SystemExit(f"restatement disagrees with the reference: {name}")


def flat_of(model):
    return np.concatenate([v.detach().numpy().ravel() for v in model.state_dict().values()])


def main(ref):
    scratch = tempfile.mkdtemp(prefix="baler_golden_fpga_")
    os.chdir(scratch)       # helper.py:25 writes next to the working directory
    sys.path.insert(0, ref)
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from baler import baler as ref_baler
    from baler.modules import models as ref_models
    from baler.modules import utils as ref_utils

    import fpga_ref
    from baler_amd import synth

    torch.set_num_threads(8)
    out = {}
    for (n, z, seed, rows) in ((24, 15, 17, 300), (7, 3, 171, 64)):
        d = fpga_ref.dims(n, z)
        torch.manual_seed(seed)
        model = ref_models.FPGA_prototype_model(n, z)
        sd = model.state_dict()
        init = flat_of(model)
        rng = np.random.default_rng(seed)
        cand = rng.random((rows * 3, n))
        x = cand[fpga_ref.off_the_kink(d, init, cand)][:rows]
        assert x.shape[0] == rows
        xt = torch.as_tensor(x)
        z_ref = model.encode(xt).detach().numpy()
        r_ref = model(xt).detach().numpy()
        d_ref = model.decode(torch.as_tensor(z_ref)).detach().numpy()
        print(f"FPGA_prototype_model({n}, {z}): {init.size} parameters")
        check("encode", fpga_ref.encode(d, init, x), z_ref, 1e-15)
        check("decode", fpga_ref.decode(d, init, z_ref), d_ref, 1e-15)
        check("forward", fpga_ref.forward(d, init, x), r_ref, 1e-15)
        opt = torch.optim.Adam(model.parameters(), lr=1e-2)
        p, m, v = init.copy(), np.zeros_like(init), np.zeros_like(init)
        snaps = {}
        for step in (1, 2, 3):
            opt.zero_grad()
            recon = model(xt)
            loss, _, _ = ref_utils.mse_sum_loss_l1(model_children=list(model.children()), true_data=xt, reconstructed_data=recon,
                                                reg_param=0.001, validate=True)
            loss.backward()
            g_ref = np.concatenate([q.grad.numpy().ravel() for q in model.parameters()])
            l_me, g_me = fpga_ref.fwd_bwd(d, p, x)
            check(f"loss step {step}", l_me, loss.item(), 1e-14)
            check(f"gradient step {step}", g_me, g_ref, 1e-13)
            if step == 1:
                snaps.update(loss=np.float64(loss.item()), grad=g_ref)
            opt.step()
            fpga_ref.adam_step(p, g_me, m, v, step, 1e-2)
            st = opt.state_dict()["state"]
            m_ref = np.concatenate([st[i]["exp_avg"].numpy().ravel() for i in range(len(st))])
            v_ref = np.concatenate([st[i]["exp_avg_sq"].numpy().ravel() for i in range(len(st))])
            check(f"params after step {step}", p, flat_of(model), 1e-12)
            if step in (1, 3):
                snaps.update({f"p{step}": flat_of(model), f"m{step}": m_ref, f"v{step}": v_ref})
        tag = "" if (n, z) == (24, 15) else "_7_3"
        out.update({f"init{tag}": init, f"x{tag}": x, f"z{tag}": z_ref, f"decoded{tag}": d_ref, f"recon{tag}": r_ref,
                    f"seed{tag}": np.int64(seed)})
        out.update({k + tag: v for k, v in snaps.items()})
        if not tag:
            out["keys"] = np.array(list(sd.keys()))
            out["shapes"] = np.array([list(t.shape) + [0] * (2 - t.dim()) for t in sd.values()])
            out["dtypes"] = np.array([str(t.dtype) for t in sd.values()])
    np.savez(os.path.join(OUT, "g17_fpga.npz"), **out)
    print("wrote g17_fpga.npz")

    # ---- g18: the reference CLI with model_name = "FPGA_prototype_model" on synth.cms_rows(10000)
    ws = os.path.join(scratch, "workspaces")
    shutil.copytree(os.path.join(REPO, "workspaces", "CMS_workspace"), os.path.join(ws, "CMS_workspace"))
    open(os.path.join(ws, "__init__.py"), "w").close()
    cfg = os.path.join(ws, "CMS_workspace", "CMS_project_v1", "config", "CMS_project_v1_config.py")
    src = open(cfg).read()
    src = src.replace('c.model_name = "AE"', 'c.model_name = "FPGA_prototype_model"')
    src = src.replace("c.activation_extraction = True", "c.activation_extraction = False")
    assert "FPGA_prototype_model" in src and "c.activation_extraction = False" in src
    open(cfg, "w").write(src)
    for dd in ("compressed_output", "decompressed_output", "plotting", "training"):
        os.makedirs(os.path.join(ws, "CMS_workspace", "CMS_project_v1", "output", dd), exist_ok=True)
    os.makedirs(os.path.join(ws, "CMS_workspace", "data"), exist_ok=True)
    raw = synth.cms_rows(10000)
    np.savez(os.path.join(ws, "CMS_workspace", "data", "example_CMS_data.npz"), data=raw, names=synth.CMS_NAMES)
    torch.manual_seed(18)
    init_model = ref_models.FPGA_prototype_model(24, 15)
    init_sd = {k: v.clone() for k, v in init_model.state_dict().items()}
    from baler.modules import helper as ref_helper

    def factory(n_features, z_dim):
        m = ref_models.FPGA_prototype_model(n_features, z_dim)
        m.load_state_dict(init_sd)
        return m

    ref_helper.model_init = lambda name: factory
    outp = os.path.join(ws, "CMS_workspace", "CMS_project_v1", "output")
    for mode in ("train", "compress", "decompress"):
        sys.argv = ["baler", "--project", "CMS_workspace", "CMS_project_v1", "--mode", mode]
        ref_baler.main()
    loss_data = np.load(os.path.join(outp, "training", "loss_data.npy"))
    norm_feats = np.load(os.path.join(outp, "training", "normalization_features.npy"))
    sd = torch.load(os.path.join(outp, "compressed_output", "model.pt"))
    final_flat = np.concatenate([v.numpy().ravel() for v in sd.values()])
    comp = np.load(os.path.join(outp, "compressed_output", "compressed.npz"))
    decomp = np.load(os.path.join(outp, "decompressed_output", "decompressed.npz"))
    idx = np.sort(np.random.default_rng(18).choice(final_flat.size, size=512, replace=False))
    np.savez(os.path.join(OUT, "g18_fpga_cli.npz"), init=flat_of(init_model), loss_data=loss_data,
             normalization_features=norm_feats, final_sample_idx=idx, final_sample=final_flat[idx],
             final_l2=np.float64(np.linalg.norm(final_flat)), keys=np.array(list(sd.keys())),
             compressed_head=comp["data"][:64], compressed_tail=comp["data"][-16:], compressed_colsum=comp["data"].sum(axis=0),
             compressed_shape=np.array(comp["data"].shape), compressed_nf=comp["normalization_features"], names=comp["names"],
             decompressed_head=decomp["data"][:64], decompressed_colsum=decomp["data"].sum(axis=0),
             decompressed_shape=np.array(decomp["data"].shape))
    print("wrote g18_fpga_cli.npz")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("BALER_REFERENCE", ""))
