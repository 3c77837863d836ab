"""The bf16 kernels of the 24-column autoencoder on MI355X (csrc/bf16.hip: encode / decode / forward + loss; csrc/bf16_train.hip: the
training pair) against the NumPy emulation of their arithmetic contract (tests/bf16_ref.py; the text: include/baler_amd.h), on the
same inputs, element by element -- not against the fp64 oracle at a statistical bar.

The rule and its inputs are those of tests/test_bf16_contract_host.py (inference_rule, training_rule, infer_case, train_case), where
every bar is derived from the distance between the emulation's own accumulation variants and from the emulation's error against the
oracle -- nothing is tuned on the kernels -- and where deliberately wrong emulations are shown to fail it.  Every distance is printed.

Also here: encode, decode and one training pass of the wide models 512-6, 625-7 and 2500-25 (csrc/fused.hip, csrc/generic.hip), and
BAMD_MODE_F16.  Two comparisons are held to the 1.5 x rule of tests/test_gpu_f16.py, row by row, instead of the exact-row count --
2500-25 at 33 and 129 rows, and binary16: test_bf16_contract_host.FALLBACK says why."""
import numpy as np
import pytest
import torch

import bf16_ref as br
from baler_amd import native
from oracle import c_oracle as orc
from test_bf16_contract_host import (CAP_MAX, EMU, F16_ZS, N_BIG, N_MAX, NS, TOL32, TRAIN_NS, TRAIN_OTHER_N, TRAIN_OTHER_ZS, TRAIN_ZS,
                                     WIDE_CASES, ZS, f16_case, infer_case, inference_rule, row_err, train_case, train_case_of_rows,
                                     training_rule, wide_case, wide_train_case)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _bf16_kernels_for_every_batch(monkeypatch):
    """BF16 handles train batches of <= 3072 rows on the fp32 small-batch kernels; these tests are about the bf16 kernels, at every size."""
    monkeypatch.setenv("BALER_AMD_BF16_SMALL_ROWS", "0")


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def host(t):
    return t.cpu().numpy().astype(np.float64)


def make_handle(dims, flat, path="bf16", mode="bf16"):
    h = native.Handle(dims, mode)
    p = dev(np.concatenate([flat, [0.0]]), torch.float32)
    h.load_params(p)
    assert h.path.startswith(path) and h.compute_mode == native.MODE_NAMES[mode]
    return h, p


def check_three(h, c, tag, x, zo, emu, ref_rows):
    """encode(x), decode(zo), forward(x) of the handle against the emulation's rows `emu`; the loss against the kernel's own
    reconstruction (float64 sum of (float32 recon - float32 x)^2 / 24)."""
    recon, loss = h.forward_loss(x)
    for op, got in (("encode", h.encode(x)), ("decode", h.decode(zo)), ("forward", recon)):
        inference_rule(f"{op} {tag}", host(got), emu[op], ref_rows[op], c["cap"][op])
    want = float(((host(recon.to(torch.float32)) - host(x.to(torch.float32))) ** 2).sum() / 24)
    assert abs(loss.item() - want) <= 1e-9 * want, f"loss {tag}: {loss.item()} vs {want} from the reconstruction"
    return loss.item()


@pytest.mark.parametrize("z", ZS)
def test_inference_is_the_emulation(z):
    c = infer_case(z)
    h, _ = make_handle(c["dims"], c["flat"])
    emu = c["emu"][EMU]
    for dt in (torch.float32, torch.float64):
        for n in NS:
            loss = check_three(h, c, f"z={z} n={n} {str(dt)[6:]}", dev(c["x"][:n], dt), dev(c["zo"][:n], dt),
                               {op: emu[op][:n] for op in emu if op != "loss"}, {op: c["ref"][op][:n] for op in c["ref"]})
    print(f"z={z}: loss {loss} against the emulation's {emu['loss']} ({abs(loss - emu['loss']) / emu['loss']:.1e})")
    assert abs(loss - emu["loss"]) <= TOL32 * emu["loss"]      # the 4100-row call; the emulation's variants are held to the same


@pytest.mark.parametrize("z", ZS)
def test_normalise_on_load_and_unnormalise_with_int_mask(z):
    """Raw rows normalised inside the encode (float64 arithmetic, one rounding to float32), the decode un-normalised in float64 and
    truncated on the int columns."""
    c = infer_case(z)
    h, _ = make_handle(c["dims"], c["flat"])
    n = 513
    feats = np.stack([np.linspace(-3, 3, 24), np.linspace(0.5, 40, 24)])
    raw = c["x"][:n] * feats[1] + feats[0]
    for dt in (torch.float64, torch.float32):
        rows = host(dev(raw, dt))
        xn = (rows - feats[0]) / feats[1]
        emu = br.encode(c["dims"], c["flat"], rows, br.ACCS[EMU], feats=feats)
        inference_rule(f"encode + normalise z={z} {str(dt)[6:]}", host(h.encode(dev(raw, dt), features=dev(feats))), emu,
                       orc.encode(c["dims"], c["flat"], xn), c["cap"]["encode"])
    mask = (np.arange(24) % 3 == 0).astype(np.uint8)
    zo = dev(c["zo"][:n])
    out = host(h.decode(zo, features=dev(feats), int_mask=torch.from_numpy(mask).cuda()))
    fl = mask == 0

    def back(t):
        return ((t - feats[0]) / feats[1])[:, fl]
    emu_out = br.decode(c["dims"], c["flat"], c["zo"][:n], br.ACCS[EMU], feats=feats, int_mask=mask)
    inference_rule(f"decode + un-normalise z={z} (float columns)", back(out), back(emu_out),
                   back(orc.renormalize(c["ro"][:n], feats[0], feats[1])), c["cap"]["decode"])
    # the int columns: what the kernel's own float32 reconstruction truncates to -- and the emulation's integers wherever the row is
    # exact and the emulation's value is clear of an integer by more than the row may be off
    plain = host(h.decode(dev(c["zo"][:n], torch.float32)))
    assert np.array_equal(out[:, ~fl], np.trunc(plain * feats[1] + feats[0])[:, ~fl])
    emu_plain = br.decode(c["dims"], c["flat"], c["zo"][:n], br.ACCS[EMU])
    norm = np.abs(emu_plain).max()
    exact = row_err(plain, emu_plain, norm) <= TOL32
    un = emu_plain.astype(np.float64) * feats[1] + feats[0]
    safe = exact[:, None] & (np.abs(un - np.round(un)) > 2 * TOL32 * norm * feats[1]) & ~fl[None, :]
    print(f"int columns z={z}: {safe.sum()} of {n * (~fl).sum()} values compared with the emulation's integers")
    assert safe.sum() > 0.9 * n * (~fl).sum() and np.array_equal(out[safe], emu_out[safe])


def test_second_grid_round_every_row():
    """131072 + 77 rows: more than one pass of the full grid.  The rows are those of the 4100-row case, repeated: the contract is
    row-local, so every row of the large call has its emulation."""
    c = infer_case(15)
    h, _ = make_handle(c["dims"], c["flat"])
    idx = np.arange(N_BIG) % N_MAX
    emu = c["emu"][EMU]
    check_three(h, c, f"n={N_BIG}", dev(c["x"][idx]), dev(c["zo"][idx]), {op: emu[op][idx] for op in emu if op != "loss"},
                {op: c["ref"][op][idx] for op in c["ref"]})


@pytest.mark.parametrize("F,Z,n", WIDE_CASES)
def test_wide_model_encode_and_decode(F, Z, n):
    """The wide models' encode and decode (csrc/fused.hip): en1 / de4 and, where test_bf16_contract_host.wide_paths says so, the
    narrow layers on the bf16 MFMA with the inference contract's roundings; the other narrow layers in exact fp32."""
    c = wide_case(F, Z, n)
    h, _ = make_handle(c["dims"], c["flat"], path="fused")
    for op, dt in (("encode32", torch.float32), ("encode64", torch.float64)):
        inference_rule(f"{F}-{Z} n={n} {op}", host(h.encode(dev(c["x"], dt))), c["emu"][op][EMU], c["ref"][op], c["cap"][op], c["fallback"])
    for dt in (torch.float32, torch.float64):
        inference_rule(f"{F}-{Z} n={n} decode {str(dt)[6:]}", host(h.decode(dev(c["zo"], dt))), c["emu"]["decode"][EMU], c["ref"]["decode"],
                       c["cap"]["decode"], c["fallback"])
    # raw rows: normalised in float64 into a float32 workspace, then the float32 rows' kernel
    feats = np.stack([np.linspace(-3, 3, F), np.linspace(0.5, 40, F)])
    raw = c["x"] * feats[1] + feats[0]
    emu = br.encode(c["dims"], c["flat"], raw, br.ACCS[EMU], feats=feats, fp32_layers=c["paths"]["encode32"])
    inference_rule(f"{F}-{Z} n={n} encode + normalise", host(h.encode(dev(raw), features=dev(feats))), emu,
                   orc.encode(c["dims"], c["flat"], (raw - feats[0]) / feats[1]), c["cap"]["encode32"], c["fallback"])


@pytest.mark.parametrize("F,Z,n", WIDE_CASES)
def test_wide_model_training_pass(F, Z, n, monkeypatch):
    """One training pass of a wide model on the bf16 launches (wide_bf16_train_fwd / _bwd_kernel, dw_wide_bf16_k / dw_short_bf16_k)
    against bf16_ref.wide_train_pass: float32 rows, the same rows as float64, and raw rows with features."""
    monkeypatch.setenv("BALER_AMD_WIDE_SMALL_ROWS", "0")      # (small batches run the float32 split launches by default)
    c = wide_train_case(F, Z, n)
    h, p = make_handle(c["dims"], c["flat"], path="fused")
    training_rule(f"{F}-{Z} n={n} float32 rows", *run_pass(h, p, dev(c["x"])), c)
    training_rule(f"{F}-{Z} n={n} float64 rows", *run_pass(h, p, dev(c["x"], torch.float64)), c)
    feats = np.stack([np.linspace(-3, 3, F), np.linspace(0.5, 40, F)])
    raw = c["x"].astype(np.float64) * feats[1] + feats[0]
    cc = train_case_of_rows(c["dims"], c["flat"], raw, feats, br.wide_train_pass)
    training_rule(f"{F}-{Z} n={n} features", *run_pass(h, p, dev(raw), dev(feats)), cc)


@pytest.mark.parametrize("z", F16_ZS)
def test_fp16_mode_row_by_row(z):
    """BAMD_MODE_F16 against test_f16_host.f16_chain on the rows of the bf16 case: the 1.5 x rule on the error against the oracle
    (test_bf16_contract_host.FALLBACK) and, beyond tests/test_gpu_f16.py, EVERY row within 1.5 x the emulation's worst row of the
    emulation; the share of rows that are not exact is printed."""
    c = f16_case(z)
    h, _ = make_handle(c["dims"], c["flat"], path="f16", mode="fp16")
    for dt in (torch.float32, torch.float64):
        for n in NS:
            x, zo = dev(c["x"][:n], dt), dev(c["zo"][:n], dt)
            for op, got in (("encode", h.encode(x)), ("decode", h.decode(zo)), ("forward", h.forward_loss(x)[0])):
                inference_rule(f"fp16 {op} z={z} n={n} {str(dt)[6:]}", host(got), c["emu"]["f32"][op][:n], c["ref"][op][:n], CAP_MAX, True)


def run_pass(h, p, x, features=None):
    g, g2 = torch.zeros_like(p), torch.zeros_like(p)
    h.fwd_bwd(x, g, features=features)
    h.fwd_bwd(x, g2, features=features)
    assert torch.equal(g, g2)                                   # fixed-order reductions: bitwise repeatable
    gh = host(g)
    return float(gh[-1]), gh[:-1]


@pytest.mark.parametrize("n", TRAIN_NS)
@pytest.mark.parametrize("z", TRAIN_ZS)
def test_training_pass_is_the_emulation(z, n):
    c = train_case(z, n)
    h, p = make_handle(c["dims"], c["flat"])
    training_rule(f"z={z} n={n}", *run_pass(h, p, dev(c["x"])), c)
    if n == 1000:
        # float32 rows, and raw rows normalised on load: each against the emulation of exactly those rows, with the variants, the oracle and the bars of those rows
        x32 = c["x"].astype(np.float32)
        feats = np.stack([np.linspace(-3, 3, 24), np.linspace(0.5, 40, 24)])
        raw = c["x"] * feats[1] + feats[0]
        for tag, rows, f in (("float32 rows", x32, None), ("features", raw, feats)):
            cc = train_case_of_rows(c["dims"], c["flat"], rows, f)
            training_rule(f"z={z} n={n} {tag}", *run_pass(h, p, dev(rows), None if f is None else dev(f)), cc)


@pytest.mark.parametrize("z", TRAIN_OTHER_ZS)
def test_training_pass_other_latents(z):
    c = train_case(z, TRAIN_OTHER_N, TRAIN_OTHER_N)
    h, p = make_handle(c["dims"], c["flat"])
    training_rule(f"z={z} n={TRAIN_OTHER_N}", *run_pass(h, p, dev(c["x"])), c)
