"""Guard-band tests: a call touches only the row block, codes and parameters it was given (tests/guard_bands.py).

Every case runs each call twice on ONE handle: on plain tensors, the way the rest of the suite calls the library (`plain`), and with
EVERY tensor argument -- inputs and outputs alike -- framed inside a larger poisoned arena, with lead = 0 (the block at the
allocation's own alignment) and lead = 3 rows (the block has only the alignment its row size gives it).  Then
  (a) the output guards still hold 0x5A and the input arenas (NaN guards) are unchanged, bit for bit;
  (b) every framed output equals `plain` bit for bit (all sums on these paths are fixed-order; colstats.hip, the one file with
      atomics, is held to the bar of tests/test_gpu_colstats.py on its sums);
  (c) at the case's largest row count the framed result meets the project's existing bar against oracle/c_oracle (fpga_ref /
      pjconv_ref for those families): rel() <= 1e-5 in fp32, 1e-11 in fp64 (on float64 output), rel-L2 <= 2e-2 for the narrow bf16
      kernels (training loss 2e-3) and 6e-3 (gradients 5e-3, loss 1e-3) for the wide bf16 ones -- the bars of tests/test_gpu_parity.py
      and tests/test_gpu_bf16_train.py.  16-bit codes are
      held to the identity of tests/test_gpu_latent16.py (the float32 codes rounded to nearest even) on top of that.  Parameters
      after Adam: rel-L2 at the mode's bar (see training_calls for bf16).  FPGA_prototype_model and PJ_Conv_AE have no reference for
      activation_means, and oracle/c_oracle has no latent term: bamd_fwd_bwd_latent is held to a NumPy restatement that the test first
      checks against oracle/c_oracle without one (rel-L2 as in tests/test_gpu_swae.py; on a BF16 handle, that family's gradient bar).
      Handle-free calls: the oracle or NumPy, bamd_swd the torch restatement and bars of tests/test_gpu_swae.py, bamd_column_moments /
      bamd_column_hist the NumPy references, bin edges and bars of tests/test_gpu_colstats.py.
Routings (ROUTES): the knobs of the README's table, set the way the suite's other tests set them, so that at these small row counts the
throughput pair (both role settings), the tail hand-off, the 4-row and 16-row small-batch chains, the bf16 training pair, the wide split
launches on 16-row tiles and on 64-row groups, the one-launch wide kernels, the chunked class pass, the three fp64 chains and the
chunked converting launch each see framed calls.  Every case prints family, h.path, compute mode, routing and row count.
Row counts: 129, then 17, then 1 on the same handle, so that every smaller call runs over workspaces the larger one left dirty.

The one combination some families refuse (decode with features into float32, SERVES_RENORM_F32 below) must be refused with framed
tensors too, with nothing written; any other NativeError fails the test.
No case can fault by construction: every stray access within 160 rows / 4096 bytes of a block stays inside its arena, and the guard
entries of index inputs are valid indices that point at a guard row."""
import numpy as np
import pytest
import torch

import fpga_ref
import guard_bands as gb
import pjconv_ref
from baler_amd import native
from baler_amd.modules import models
from oracle import c_oracle as orc
from oracle import deltas as odeltas
import test_gpu_colstats as cst
from test_gpu_latent16 import assert_same_bits as _same_bits_16_32_64
from test_gpu_parity import rel, rel_l2
from test_gpu_swae import _swd_ref

pytestmark = pytest.mark.gpu

LEADS = (0, 3)
ROWS = (129, 17, 1)
BIG = 256 * 64 + 65
F32, F64, F16, BF16 = torch.float32, torch.float64, torch.float16, torch.bfloat16
TOL = {"fp32": 1e-5, "fp64": 1e-11}


def assert_same_bits(a, b, what):
    """assert_same_bits of tests/test_gpu_latent16.py, and the same for the one-byte types (flags, masks)."""
    if a.element_size() == 1:
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), what
    else:
        _same_bits_16_32_64(a, b, what)


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def host(t):
    return t.detach().to(torch.float64).cpu().numpy()


class Frames:
    """The framed arguments of one call: inp() frames an input (NaN guards, snapshot kept), out() an output or in/out tensor
    (0x5A guards); check() is assertion (a)."""

    def __init__(self, lead, what):
        self.lead, self.what, self.ins, self.outs = lead, what, [], []

    def inp(self, t, fill=gb.NAN):
        if t is None:
            return None
        v, a = gb.framed(t, self.lead, None, fill)
        self.ins.append((a, a.clone()))
        return v

    def out(self, t, name):
        v, a = gb.framed(t, self.lead, None, gb.POISON)
        self.outs.append((a, t.shape[0], name))
        return v

    def check(self):
        torch.cuda.synchronize()
        for a, n, name in self.outs:
            gb.assert_guards_intact(a, self.lead, n, f"{self.what} lead={self.lead}: {name}")
        for a, snap in self.ins:
            gb.assert_inputs_untouched(a, snap, f"{self.what} lead={self.lead}")


def both(what, call, ins, outs, same=None, refusal=None):
    """Run `call(ins, outs)` on plain tensors and, per lead, on framed ones.  ins: dict name -> tensor or None; outs: dict name ->
    initial block (poisoned for a pure output, the starting value for an in/out tensor).  Assertions (a) and (b); returns the framed
    outputs of the last lead (dict).  refusal: None -- the library must serve the call (a NativeError fails the test); a string -- the
    library must refuse it, plain and framed alike, with that text in the message and nothing written; then None is returned."""
    plain = {k: v.clone() for k, v in outs.items()}
    if refusal is None:
        call(ins, plain)
    else:
        with pytest.raises(native.NativeError, match=refusal):
            call(ins, plain)
    got = None
    for lead in LEADS:
        fr = Frames(lead, what)
        fi = {k: fr.inp(v) for k, v in ins.items()}
        fo = {k: fr.out(v, k) for k, v in outs.items()}
        if refusal is not None:
            with pytest.raises(native.NativeError, match=refusal):
                call(fi, fo)
            fr.check()
            for k, v in outs.items():
                assert_same_bits(fo[k], v, f"{what} lead={lead}: {k} written by a refused call")
            continue
        call(fi, fo)
        fr.check()
        for k in outs:
            (same or assert_same_bits)(fo[k], plain[k], f"{what} lead={lead}: {k}")
        got = fo
    return got


# ---- raw calls for the entry points whose binding allocates its own output -----------------------------------------------------
def forward_loss_raw(h, x, feats, recon, loss):
    native._check(native.lib().bamd_forward_loss(h._h, native._ptr(x), native._dt(x), x.shape[0], native._ptr(feats), native._ptr(recon),
                                                 native._dt(recon), native._ptr(loss), h._s()), "bamd_forward_loss")


def activation_means_raw(h, x, feats, out):
    native._check(native.lib().bamd_activation_means(h._h, native._ptr(x), native._dt(x), x.shape[0], native._ptr(feats), native._ptr(out),
                                                     out.shape[1], h._s()), "bamd_activation_means")


def raw2(call_name, argv):
    native._check(getattr(native.lib(), call_name)(*argv), call_name)


# ---- references ------------------------------------------------------------------------------------------------------------------
def dense_fwd_bwd(dims, flat, x, lg=None, keep=None):
    """NumPy float64 fwd + bwd of the dense LeakyReLU(0.01) autoencoder with dL/dz += lg at the bottleneck (oracle/c_oracle has no
    latent term); checked against orc.fwd_bwd without one where it is used.  keep (a dict): receives "dz", dL/dz at the bottleneck."""
    L, lay, off = len(dims) - 1, [], 0
    for l in range(L):
        K, N = dims[l], dims[l + 1]
        lay.append((flat[off:off + K * N].reshape(N, K), flat[off + K * N:off + K * N + N]))
        off += K * N + N
    lin = (L // 2 - 1, L - 1)
    ys, pre = [x], []
    for l, (W, b) in enumerate(lay):
        a = ys[-1] @ W.T + b
        pre.append(a)
        ys.append(a if l in lin else np.where(a > 0, a, 0.01 * a))
    e = ys[-1] - x
    dz, g = 2.0 * e / dims[0], [None] * L
    for l in range(L - 1, -1, -1):
        if l not in lin:
            dz = dz * np.where(pre[l] > 0, 1.0, 0.01)
        if l == L // 2 - 1 and lg is not None:
            dz = dz + lg
        if l == L // 2 - 1 and keep is not None:
            keep["dz"] = dz.copy()
        g[l] = np.concatenate([(dz.T @ ys[l]).ravel(), dz.sum(0)])
        dz = dz @ lay[l][0]
    return float((e * e).sum() / dims[0]), np.concatenate(g)


class DenseRef:
    def __init__(self, dims, flat):
        self.dims, self.flat = dims, flat

    def rows(self, n, seed, margin=2e-5):
        """n uniform random rows whose LeakyReLU pre-activations all stay farther than `margin` from 0 (off_the_kink of
        tests/test_gpu_parity.py, for any layer count): the max-norm bars are held on rows clear of the kink."""
        d, x = self.dims, np.random.default_rng(seed).random((2 * n + 64, self.dims[0]))
        L, a, off, keep = len(d) - 1, x, 0, np.ones(x.shape[0], dtype=bool)
        for l in range(L):
            K, N = d[l], d[l + 1]
            a = a @ self.flat[off:off + K * N].reshape(N, K).T + self.flat[off + K * N:off + K * N + N]
            off += K * N + N
            if l not in (L // 2 - 1, L - 1):
                keep &= np.abs(a).min(axis=1) > margin
                a = np.where(a > 0, a, 0.01 * a)
        assert keep.sum() >= n
        return np.ascontiguousarray(x[keep][:n])

    def encode(self, x, flat=None):
        return orc.encode(self.dims, self.flat if flat is None else flat, x)

    def decode(self, z):
        return orc.decode(self.dims, self.flat, z)

    def fwd_bwd(self, x, lg=None, flat=None):
        flat = self.flat if flat is None else flat
        lo, go = orc.fwd_bwd(self.dims, flat, x)
        if lg is None:
            return lo, go
        l2, g2 = dense_fwd_bwd(self.dims, flat, x)
        assert rel(g2, go) < 1e-12 and abs(l2 - lo) < 1e-12 * lo, "the NumPy restatement disagrees with oracle/c_oracle"
        return dense_fwd_bwd(self.dims, flat, x, lg)

    def adam(self, p, g, m, v, t, lr):
        orc.adam_step(p, g, m, v, t, lr)

    def activation_means(self, x, max_nodes):
        return orc.activation_means(self.dims, self.flat, x, max_nodes)


class FpgaRef(DenseRef):
    def rows(self, n, seed):
        x = np.random.default_rng(seed).random((2 * n + 64, self.dims[0]))
        return np.ascontiguousarray(x[fpga_ref.off_the_kink(self.dims, self.flat, x)][:n])

    def encode(self, x, flat=None):
        return fpga_ref.encode(self.dims, self.flat if flat is None else flat, x)

    def decode(self, z):
        return fpga_ref.decode(self.dims, self.flat, z)

    def fwd_bwd(self, x, lg=None, flat=None):
        return fpga_ref.fwd_bwd(self.dims, self.flat if flat is None else flat, x, lg)

    def adam(self, p, g, m, v, t, lr):
        fpga_ref.adam_step(p, g, m, v, t, lr)

    activation_means = None


class PjRef:
    activation_means = None

    def __init__(self, z, flat):
        self.z, self.flat, self.dims = z, flat, [784, z, 784]

    def rows(self, n, seed):
        return np.random.default_rng(seed).random((n, 784))

    def encode(self, x, flat=None):
        return pjconv_ref.encode(self.z, self.flat if flat is None else flat, x)

    def decode(self, z):
        return pjconv_ref.decode(self.z, self.flat, z)

    def fwd_bwd(self, x, lg=None, flat=None):
        assert lg is None
        return pjconv_ref.fwd_bwd(self.z, self.flat if flat is None else flat, x)

    def adam(self, p, g, m, v, t, lr):
        pjconv_ref.adam_step(p, g, m, v, t, lr)


# ---- families and routings -------------------------------------------------------------------------------------------------------
PAIR = {"BALER_AMD_LATENCY_ROWS": "0", "BALER_AMD_TAIL_SPLIT": "0"}
ROUTES = {
    "default": {},
    "pair-roles0": dict(PAIR, BALER_AMD_TRAIN_ROLES="0"),
    "pair-roles1": dict(PAIR, BALER_AMD_TRAIN_ROLES="1"),
    "pair-tail-split": {"BALER_AMD_LATENCY_ROWS": "0"},
    "wide-small0": {"BALER_AMD_WIDE_SMALL_ROWS": "0"},
    "lat32-64": {"BALER_AMD_LAT32_ROWS": "64"},
    "class-chunk64": {"BALER_AMD_LATENCY_ROWS": "32", "BALER_AMD_CLASS_CHUNK_ROWS": "64"},
    "f64-qchain0": {"BALER_AMD_F64_QCHAIN_BLKS": "0"},
    "f64-regchain0": {"BALER_AMD_F64_REGCHAIN_BLKS": "0"},
    "f64-both0": {"BALER_AMD_F64_QCHAIN_BLKS": "0", "BALER_AMD_F64_REGCHAIN_BLKS": "0"},
    # a BF16 handle of the 24-column model trains batches of <= 3072 rows on the fp32 small-batch kernels: 0 sends every batch to
    # bf16_train_kernel (64-row workgroups, the dz hand-off between its two launches, reduce_tiles_k), as tests/test_gpu_bf16_train.py does
    "bf16-small0": {"BALER_AMD_BF16_SMALL_ROWS": "0"},
    # the split wide launches on 64-row groups (wide_small_in_kernel / wide_small_out_kernel; by default only above 512 rows)
    "wide-group64": {"BALER_AMD_WIDE_IN16_ROWS": "0", "BALER_AMD_WIDE_OUT16_ROWS": "0"},
    "lat4-0": {"BALER_AMD_LAT4_ROWS": "0"},           # lat2_chain_kernel on an exact instantiation (default: the 4-row chain)
    "mid-hybrid0": {"BALER_AMD_MID_HYBRID": "0"},     # 64..127 columns on the small-batch class alone, inference included
}
# name: (kind, F, Z, mode, handle env, inference routings, training routings)
INF_W = ("default", "lat32-64")
TR_F64 = ("default", "f64-qchain0", "f64-regchain0", "f64-both0")
FAMILIES = {
    "ae24-fp32": ("dense", 24, 15, "fp32", {}, ("default",), ("default", "pair-roles0", "pair-roles1", "lat4-0")),
    "ae24-fp64": ("dense", 24, 15, "fp64", {}, INF_W, TR_F64),
    "ae24-bf16": ("dense", 24, 15, "bf16", {}, ("default",), ("default", "bf16-small0")),
    "ae24z8-bf16": ("dense", 24, 8, "bf16", {}, ("default",), ("default", "bf16-small0")),
    "class40-fp32": ("dense", 40, 10, "fp32", {}, ("default",), ("default", "pair-roles0", "pair-roles1")),
    "class40-fp64": ("dense", 40, 10, "fp64", {}, INF_W, TR_F64),
    "class100-fp32": ("dense", 100, 12, "fp32", {}, ("default", "mid-hybrid0"), ("default", "class-chunk64", "mid-hybrid0")),
    "cfd625-fp32": ("dense", 625, 7, "fp32", {}, INF_W, ("default", "wide-small0", "wide-group64")),
    "cfd625-bf16": ("dense", 625, 7, "bf16", {}, INF_W, ("default", "wide-small0")),
    "cfd2500-fp32": ("dense", 2500, 25, "fp32", {}, INF_W, ("default", "wide-small0", "wide-group64")),
    "cfd2500-bf16": ("dense", 2500, 25, "bf16", {}, INF_W, ("default", "wide-small0")),
    "wide512-fp32": ("dense", 512, 6, "fp32", {}, INF_W, ("default", "wide-small0", "wide-group64")),
    "wideclass300-fp32": ("dense", 300, 20, "fp32", {}, INF_W, ("default", "wide-small0", "wide-group64")),
    "layerwise-ae24-fp32": ("dense", 24, 15, "fp32", {"BALER_AMD_FORCE_GENERIC": "1"}, ("default",), ("default",)),
    "layerwise-30-64-32-9": ("dims", [30, 64, 32, 9, 32, 64, 30], 9, "fp32", {}, ("default",), ("default",)),
    "fpga-fp32": ("fpga", 24, 15, "fp32", {}, INF_W, ("default",)),
    "fpga-fp64": ("fpga", 24, 15, "fp64", {}, INF_W, TR_F64),
    "pjconv-z10": ("pj", 784, 10, "fp32", {}, INF_W, ("default",)),
}
INFER_CASES = [pytest.param(f, r, id=f"{f}-{r}") for f, v in FAMILIES.items() for r in v[5]]
TRAIN_CASES = [pytest.param(f, r, id=f"{f}-{r}") for f, v in FAMILIES.items() for r in v[6]]


# The one combination any of these families refuses: bamd_decode that un-normalises (features) into a float32 output.  Where the
# dispatch decides it (a change of routing there moves a family between the two lists): served by the `decode` member of the
# register-chain Impl in fused.hip (infer_kernel / infer2_kernel: up to 64 columns, and 64..127 columns on the small-batch class,
# BALER_AMD_MID_HYBRID=0) and by bf16_decode (bf16.hip); refused, with the message below, by the two `decode` members of the wide-layer
# Impls in fused.hip (the fp32 and the bf16 wide kernels; 64..127 columns use them for inference by default), by generic_forward
# (generic.hip: the layer-wise path, and what fused64_infer hands this call to), by fpga_infer (fpga.hip) and by pj_decode (pjconv.hip).
# Every other NativeError fails the test.
RENORM_F32_REFUSAL = "decode with features needs a float64 output"
SERVES_RENORM_F32 = {("ae24-fp32", "default"), ("class40-fp32", "default"), ("class100-fp32", "mid-hybrid0"), ("ae24-bf16", "default"),
                     ("ae24z8-bf16", "default")}


def family(name, route, monkeypatch, spec=None):
    """spec: the FAMILIES entry of a family that another module defines (tests/test_gpu_streams.py)."""
    kind, F, Z, mode, env, _, _ = spec or FAMILIES[name]
    monkeypatch.setenv("BALER_AMD_QUIET", "1")
    for k, v in {**env, **ROUTES[route]}.items():
        monkeypatch.setenv(k, v)
    pdt = F64 if mode == "fp64" else F32
    if kind == "pj":
        torch.manual_seed(4)
        flat = models.pj_conv_init(Z).numpy().astype(np.float64)
        h, ref = native.Handle.pj_conv(Z, mode), PjRef(Z, flat)
    elif kind == "fpga":
        d, rng = fpga_ref.dims(F, Z), np.random.default_rng(17)
        flat = np.concatenate([np.concatenate([rng.uniform(-1, 1, d[l + 1] * d[l]) / np.sqrt(d[l]), rng.uniform(-1, 1, d[l + 1]) / np.sqrt(d[l])])
                               for l in range(6)])
        h, ref = native.Handle(d, mode, act="relu"), FpgaRef(d, flat)
    else:
        dims = F if kind == "dims" else orc.ae_dims(F, Z)
        flat = orc.formula_params(dims, 100 + dims[0] + Z)
        h, ref = native.Handle(dims, mode), DenseRef(dims, flat)
    flat = dev(np.concatenate([flat, [0.0]]), pdt)
    ref.flat = host(flat)[:-1]                     # the parameters as the handle holds them (float32 handles: rounded)
    h.load_params(flat)
    cmode = {native.MODE_F32: "fp32", native.MODE_F64: "fp64", native.MODE_BF16: "bf16", native.MODE_F16: "fp16",
             native.MODE_F16X3: "fp16x3"}[h.compute_mode]
    wide = h.dims[0] > 127 and kind == "dense"
    print(f"\n[guard bands] family={name} path={h.path} compute={cmode} routing={route} {ROUTES[route]} env={env}")
    return h, ref, flat, cmode, wide


def feats_of(F, seed=7):
    rng = np.random.default_rng(seed)
    f = np.stack([rng.normal(size=F) * 10, rng.uniform(0.5, 300.0, size=F)])
    return f, (rng.random(F) < 0.3).astype(np.uint8)


def bar_ok(cmode, wide, got, want, odt, what):
    """Assertion (c) for an inference result."""
    if cmode == "bf16":
        err, bar = rel_l2(got, want), (6e-3 if wide else 2e-2)
    elif cmode == "fp64":
        if odt != F64:
            return                                  # the fp64 bar is on float64 output; float32 output is covered bit for bit by (b)
        err, bar = rel(got, want), TOL["fp64"]
    else:
        err, bar = rel(got, want), TOL["fp32"]
    print(f"    oracle {what}: {err:.3e} (bar {bar:g})")
    assert err <= bar, what


# ---- encode / decode -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,route", INFER_CASES)
def test_encode_decode(name, route, monkeypatch):
    h, ref, _, cmode, wide = family(name, route, monkeypatch)
    F, Z = h.dims[0], h.z_dim
    fnp, mnp = feats_of(F)
    feats, mask = dev(fnp), dev(mnp)
    for n in ROWS:
        print(f"  rows={n}")
        x64 = ref.rows(n, 1000 + n)
        for xdt in (F32, F64):
            xn = dev(x64, xdt)
            xraw = dev(host(xn) * fnp[1] + fnp[0], xdt)
            for use_f in (False, True):
                xin = xraw if use_f else xn
                seen = host(xin)
                seen = (seen - fnp[0]) / fnp[1] if use_f else seen               # what the kernel computes on, in float64
                z32 = None
                for odt in (F32, F64, F16, BF16):
                    what = f"{name} {route} encode n={n} x={xdt} features={use_f} out={odt}"
                    got = both(what, lambda i, o: h.encode(i["x"], features=i["features"], out=o["z"]),
                               {"x": xin, "features": feats if use_f else None}, {"z": gb.poisoned((n, Z), odt, "cuda")})
                    if odt == F32:
                        z32 = got["z"]
                    if odt in (F16, BF16) and z32 is not None:
                        assert_same_bits(got["z"], z32.to(odt), what + ": not the rounded float32 codes")
                    elif n == ROWS[0]:
                        bar_ok(cmode, wide, host(got["z"]), ref.encode(seen), odt, what)
        z64 = ref.encode(x64)
        for cdt in (F32, F16, BF16):
            zc = dev(z64, cdt)
            want = ref.decode(host(zc)) if n == ROWS[0] else None
            for renorm in (False, True):
                for odt in (F32, F64):
                    what = f"{name} {route} decode n={n} codes={cdt} renorm={renorm} out={odt}"
                    got = both(what, lambda i, o: h.decode(i["z"], features=i["features"], int_mask=i["int_mask"], out=o["out"]),
                               {"z": zc, "features": feats if renorm else None, "int_mask": mask if renorm else None},
                               {"out": gb.poisoned((n, F), odt, "cuda")},
                               refusal=RENORM_F32_REFUSAL if renorm and odt == F32 and (name, route) not in SERVES_RENORM_F32 else None)
                    if got is None:
                        print(f"    refused as expected: {what}")
                        continue
                    if n == ROWS[0]:
                        o = host(got["out"])
                        if renorm:
                            keep = mnp == 0
                            assert np.array_equal(o[:, ~keep], np.trunc(o[:, ~keep])), what
                            bar_ok(cmode, wide, o[:, keep], (want * fnp[1] + fnp[0])[:, keep], odt, what)
                        else:
                            bar_ok(cmode, wide, o, want, odt, what)


# ---- the training entry points ---------------------------------------------------------------------------------------------------
def grad_ok(cmode, wide, n, g, lo, go, what, l2_only=False):
    g = host(g)
    if cmode == "bf16":
        gbar, lbar = ((5e-3 if n >= 33 else 1e-1), 1e-3) if wide else (2e-2, 2e-3)     # narrow: tests/test_gpu_bf16_train.py
        gerr = rel_l2(g[:-1], go)
    else:
        gbar = lbar = TOL[cmode]
        gerr = rel_l2(g[:-1], go) if l2_only else rel(g[:-1], go)
    lerr = abs(g[-1] - lo) / lo
    print(f"    oracle {what}: gradient {gerr:.3e} (bar {gbar:g}) loss {lerr:.3e} (bar {lbar:g})")
    assert gerr <= gbar and lerr <= lbar, what


def latent_share_ok(h, ref, xin, seen, lgd, g, what):
    """bamd_fwd_bwd_latent on a BF16 handle really adds latent_grad, once and unscaled.  Against the same call with a zero latent term
    (same kernels, same forward, so the same LeakyReLU signs):
      * the loss and every decoder tensor are the same bits (dL/dz enters behind them), every encoder tensor differs;
      * the bias gradient of the bottleneck layer is sum_rows dL/dz with nothing between it and the latent term, so the two calls
        differ there by sum_rows latent_grad, up to the rounding of each row's dL/dz to bfloat16 on the way into the weight-gradient
        product: unit roundoff 2^-9 per term, |error| <= 2^-9 sum_rows (|dz + lg| + |dz|) per column.  The bound is taken at 2^-8 with
        dz from the float64 reference (the handle's own dz differs from it by the bf16 forward, a few per cent; float32 accumulation
        of 129 terms is 2^-17 of that).  A dropped latent term misses it by |sum_rows lg|; the test first checks that this is more
        than 4 bounds in some column, which depends on the reference alone."""
    dims, L = ref.dims, len(ref.dims) - 1
    zero = torch.zeros_like(g)
    h.fwd_bwd_latent(xin, torch.zeros_like(lgd), zero)
    off = [0]
    for l in range(L):
        off += [off[-1] + dims[l] * dims[l + 1], off[-1] + dims[l] * dims[l + 1] + dims[l + 1]]      # W_l, b_l, W_l+1, ..
    enc = off[2 * (L // 2)]
    assert torch.equal(g[enc:], zero[enc:]), what + ": the latent term changed a decoder tensor or the loss"
    for t in range(2 * (L // 2)):
        assert not torch.equal(g[off[t]:off[t + 1]], zero[off[t]:off[t + 1]]), what + f": encoder tensor {t} ignores the latent term"
    lg, keep = host(lgd), {}
    dense_fwd_bwd(dims, ref.flat, seen, lg, keep)
    bound = 2.0 ** -8 * (np.abs(keep["dz"]).sum(0) + np.abs(keep["dz"] - lg).sum(0))
    assert (np.abs(lg.sum(0)) > 4 * bound).any(), what + ": the check has no power on these rows"
    d = (host(g) - host(zero))[off[2 * (L // 2) - 1]:enc]
    err = np.abs(d - lg.sum(0)) / bound
    print(f"    latent share {what}: bottleneck bias gradient off by at most {err.max():.3f} of its bf16 rounding bound")
    assert (err <= 1.0).all(), what + ": the latent term's share of the bottleneck bias gradient"


def training_calls(name, route, h, ref, flat, cmode, wide, n, x64, oracle, only_fwd_bwd=False):
    F, Z, np_ = h.dims[0], h.z_dim, h.nparams
    pdt = h.param_dtype
    fnp, _ = feats_of(F)
    feats = dev(fnp)
    tag = f"{name} {route} n={n}"
    pj = isinstance(ref, PjRef)
    lscale = 1.0 if pj else 1.0 / F                     # the loss is sum((r - x)^2) / n_features (PJ_Conv_AE: / 1 channel)
    for xdt in (F32, F64):
        xn = dev(x64, xdt)
        xraw = dev(host(xn) * fnp[1] + fnp[0], xdt)
        for use_f in (False, True):
            if only_fwd_bwd and use_f:
                continue
            xin, fe = (xraw, feats) if use_f else (xn, None)
            seen = (host(xin) - fnp[0]) / fnp[1] if use_f else host(xin)
            v = f"{tag} x={xdt} features={use_f}"
            got = both(v + " fwd_bwd", lambda i, o: h.fwd_bwd(i["x"], o["grads"], features=i["features"]),
                       {"x": xin, "features": fe}, {"grads": gb.poisoned((np_ + 1,), pdt, "cuda")})
            if oracle:
                lo, go = ref.fwd_bwd(seen)
                grad_ok(cmode, wide, n, got["grads"], lo, go, v + " fwd_bwd")
            if only_fwd_bwd:
                continue
            got = both(v + " forward_loss", lambda i, o: forward_loss_raw(h, i["x"], i["features"], o["recon"], o["loss_out"]),
                       {"x": xin, "features": fe}, {"recon": gb.poisoned((n, F), xdt, "cuda"), "loss_out": gb.poisoned((1,), F64, "cuda")})
            if oracle:
                z = ref.encode(seen)
                want = ref.decode(z)
                bar_ok(cmode, wide, host(got["recon"]), want, F64 if cmode != "fp64" else xdt, v + " forward_loss recon")
                lw, lg_ = float(((want - seen) ** 2).sum() * lscale), float(got["loss_out"].item())
                # bf16: BF16_TOL on the loss of the narrow inference kernels (test_bf16_* of tests/test_gpu_parity.py), 1e-3 wide
                lbar = (1e-3 if wide else 2e-2) if cmode == "bf16" else TOL[cmode]
                print(f"    oracle {v} forward_loss: loss {abs(lg_ - lw) / lw:.3e} (bar {lbar:g})")
                assert abs(lg_ - lw) <= lbar * lw
            if ref.activation_means is not None:
                got = both(v + " activation_means", lambda i, o: activation_means_raw(h, i["x"], i["features"], o["out"]),
                           {"x": xin, "features": fe}, {"out": gb.poisoned((len(h.dims) - 3, 200), F64, "cuda")})
                if oracle:
                    want = np.asarray(ref.activation_means(seen, 200), dtype=np.float64)
                    o = host(got["out"])
                    assert np.array_equal(np.isnan(o), np.isnan(want)), v + " activation_means: unused slots"
                    bar_ok(cmode, wide, np.nan_to_num(o), np.nan_to_num(want), F64, v + " activation_means")
    if only_fwd_bwd:
        return
    xin = dev(x64, F64 if cmode == "fp64" else F32)
    seen = host(xin)
    if not pj:
        # The latent term of tests/test_gpu_swae.py (0.01 N(0, 1) on AE(24, 15)) in the same proportion to dL/drecon = 2 e / F at every
        # width.  At a fixed 0.01 the encoder layers of a 2500-column model carry a third of the gradient norm instead of 2 %, and the
        # whole-vector bf16 bar (5e-3, set on fwd_bwd) does not follow for such a vector: LeakyReLU units within bf16 rounding of the
        # kink take the other slope (tools/bf16_kink_flips.py restates it in float64 NumPy: 7.9e-2 / 6.5e-2 / 6.7e-2 on en1 .. en3 from
        # the signs alone, which is what the wide bf16 kernels measure there; 2.3e-2 on the whole vector).
        # What then holds the latent term itself: in fp32 / fp64 the 1e-5 / 1e-11 bars do.  On a BF16 handle the encoder is ~2 % of
        # the norm, so the whole-vector bar would not notice a dropped or mis-scaled latent_grad; latent_share_ok below does.
        lg = np.random.default_rng(n).normal(size=(n, Z)) * (0.01 * 24 / F)
        lgd = dev(lg, pdt)
        got = both(tag + " fwd_bwd_latent", lambda i, o: h.fwd_bwd_latent(i["x"], i["latent_grad"], o["grads"]),
                   {"x": xin, "latent_grad": lgd}, {"grads": gb.poisoned((np_ + 1,), pdt, "cuda")})
        if oracle:      # rel-L2, as tests/test_gpu_swae.py holds it in fp32 / fp64; a BF16 handle: that family's gradient bar, as for fwd_bwd
            lo, go = ref.fwd_bwd(seen, host(lgd))
            grad_ok(cmode, wide, n, got["grads"], lo, go, tag + " fwd_bwd_latent", l2_only=True)
            if cmode == "bf16":
                latent_share_ok(h, ref, xin, seen, lgd, got["grads"], tag + " fwd_bwd_latent")
    # Adam on framed params / m / v, after gradients the handle made itself; then the one-call step and the one-call epoch.  Each call
    # starts from the case's parameters (reloaded: a step also refreshes the handle's packed weights).
    grads = torch.zeros(np_ + 1, dtype=pdt, device="cuda")
    h.fwd_bwd(xin, grads)
    zeros = torch.zeros_like(flat)

    def fresh(call):
        def run(i, o):
            h.load_params(flat)
            call(i, o)
        return run

    state = {"params": flat.clone(), "m": zeros.clone(), "v": zeros.clone(), "loss_accum": torch.full((1,), 0.25, dtype=F64, device="cuda")}
    got = both(tag + " adam_step", fresh(lambda i, o: h.adam_step(o["params"], i["grads"], o["m"], o["v"], 1, 1e-3, loss_accum=o["loss_accum"])),
               {"grads": grads}, state)
    step = both(tag + " train_step",
                fresh(lambda i, o: h.train_step(i["x"], o["params"], o["m"], o["v"], 1, 1e-3, loss_accum=o["loss_accum"], grads=o["grads"])),
                {"x": xin}, dict(state, grads=gb.poisoned((np_ + 1,), pdt, "cuda")))
    for k in ("params", "m", "v", "loss_accum"):
        assert_same_bits(step[k], got[k], f"{tag}: train_step {k} differs from fwd_bwd + adam_step")
    # Adam against the oracle's Adam.  fp32 / fp64: from the ORACLE's gradient, rel-L2 of the parameters at the mode's bar (as
    # __graft_entry__.smoke does).  bf16: the first Adam steps move every parameter by about lr whatever the size of its gradient, so
    # a sign that differs under bf16 rounding moves a parameter by 2 lr and no bar on the trajectory follows from the bf16 gradient
    # bar; the suite has none either.  There the gradient is held to its bar above and the oracle's Adam is fed the handle's OWN
    # gradient: the update itself is float32 arithmetic, held to the fp32 bar.
    pbar = TOL["fp32" if cmode == "bf16" else cmode]
    if oracle:
        lo, go = ref.fwd_bwd(seen)
        if cmode == "bf16":
            go = host(grads)[:-1]
        p, m, v_ = ref.flat.copy(), np.zeros(np_), np.zeros(np_)
        ref.adam(p, go, m, v_, 1, 1e-3)
        err = rel_l2(host(got["params"])[:-1], p)
        print(f"    oracle {tag} adam_step / train_step: params {err:.3e} (bar {pbar:g})")
        assert err <= pbar
    if n == ROWS[0]:
        ep = both(tag + " train_epoch bs=64",
                  fresh(lambda i, o: h.train_epoch(i["x"], 64, o["params"], o["m"], o["v"], 1, 1e-3, loss_accum=o["loss_accum"], grads=o["grads"])),
                  {"x": xin}, dict(state, grads=gb.poisoned((np_ + 1,), pdt, "cuda")))
        # the epoch is its three batches as single steps, bit for bit (64, 64 and 1 rows)
        loop = {k: t.clone() for k, t in dict(state, grads=gb.poisoned((np_ + 1,), pdt, "cuda")).items()}
        h.load_params(flat)
        for t, (a, b) in enumerate(((0, 64), (64, 128), (128, 129)), 1):
            h.train_step(xin[a:b], loop["params"], loop["m"], loop["v"], t, 1e-3, loss_accum=loop["loss_accum"], grads=loop["grads"])
        for k in loop:
            assert_same_bits(ep[k], loop[k], f"{tag}: train_epoch {k} differs from the per-step loop")
        if oracle and cmode != "bf16":
            p, m, v_ = ref.flat.copy(), np.zeros(np_), np.zeros(np_)
            for t, (a, b) in enumerate(((0, 64), (64, 128), (128, 129)), 1):
                _, go = ref.fwd_bwd(seen[a:b], flat=p)
                ref.adam(p, go, m, v_, t, 1e-3)
            err = rel_l2(host(ep["params"])[:-1], p)
            print(f"    oracle {tag} train_epoch: params {err:.3e} (bar {pbar:g})")
            assert err <= pbar
    h.load_params(flat)


@pytest.mark.parametrize("name,route", TRAIN_CASES)
def test_training_entry_points(name, route, monkeypatch):
    h, ref, flat, cmode, wide = family(name, route, monkeypatch)
    for n in ROWS:
        print(f"  rows={n}")
        training_calls(name, route, h, ref, flat, cmode, wide, n, ref.rows(n, 2000 + n), oracle=n == ROWS[0])


@pytest.mark.parametrize("route", ["pair-roles0", "pair-roles1", "pair-tail-split"])
def test_fwd_bwd_second_row_group(route, monkeypatch):
    """256 * 64 + 65 rows on the 24-column model: two workgroups of the throughput pair prefetch a second row group and every other
    one prefetches past the end; with BALER_AMD_TAIL_SPLIT at its default the remainder is handed to the small-batch kernels at
    x + n F.  Then the three small row counts over the workspaces this left."""
    h, ref, flat, cmode, wide = family("ae24-fp32", route, monkeypatch)
    for n in (BIG,) + ROWS:
        print(f"  rows={n}")
        x64 = np.random.default_rng(7).random((n, 24)) if n == BIG else ref.rows(n, 3000 + n)
        training_calls("ae24-fp32", route, h, ref, flat, cmode, wide, n, x64, oracle=n == BIG, only_fwd_bwd=True)


# ---- handle-free entry points ----------------------------------------------------------------------------------------------------
HF_SHAPES = [(129, 24), (17, 3), (1, 24)]


def _sums_close(a, b, what):
    """colstats.hip accumulates with atomics: extrema and counts are exact, sums are held to the fp64 bar of
    tests/test_gpu_colstats.py (1e-11, relative to the larger magnitude in the row: the sums here are of same-signed terms)."""
    a64, b64 = host(a), host(b)
    ex = list(native.MOMENT_MIN_ROWS) + list(native.MOMENT_MAX_ROWS) + [0]
    assert np.array_equal(a64[ex], b64[ex]), what
    sm = [r for r in native.MOMENT_SUM_ROWS if r != 0]
    assert (np.abs(a64[sm] - b64[sm]) <= 1e-11 * np.maximum(np.abs(b64[sm]), 1e-300)).all(), what


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,c", HF_SHAPES)
def test_handle_free_entry_points(n, c, dtype):
    print(f"\n[guard bands] handle-free n={n} columns={c} {dtype}")
    L, P, S = native.lib(), native._ptr, native._stream
    rng = np.random.default_rng(10 * n + c)
    xnp = rng.uniform(0.5, 2.0, size=(n, c))
    x = dev(xnp, dtype)
    r = dev(xnp * (1.0 + rng.normal(scale=0.08, size=xnp.shape)), dtype)
    code = native._dt(x)
    tag = f"handle-free n={n} c={c} {dtype}"
    xs = host(x)

    got = both(tag + " minmax", lambda i, o: raw2("bamd_minmax", (P(i["x"]), code, n, c, P(o["out"]), S(i["x"]))),
               {"x": x}, {"out": gb.poisoned((2, c), F64, "cuda")})
    assert np.array_equal(host(got["out"]), orc.find_minmax(xs)), tag + " minmax against the oracle"
    got = both(tag + " col_minmax", lambda i, o: raw2("bamd_col_minmax", (P(i["x"]), code, n, c, P(o["out"]), S(i["x"]))),
               {"x": x}, {"out": gb.poisoned((2, c), F64, "cuda")})
    assert np.array_equal(host(got["out"]), np.stack([xs.min(0), xs.max(0)])), tag + " col_minmax"

    fnp = np.stack([xs.min(0) - 0.5, xs.max(0) - xs.min(0) + 1.0])
    feats, mnp = dev(fnp), (rng.random(c) < 0.3).astype(np.uint8)
    for odt in (F32, F64):
        got = both(tag + f" normalize out={odt}",
                   lambda i, o: raw2("bamd_normalize", (P(i["x"]), code, n, c, P(i["features"]), P(o["out"]), native._dt(o["out"]), S(i["x"]))),
                   {"x": x, "features": feats}, {"out": gb.poisoned((n, c), odt, "cuda")})
        want = torch.from_numpy((xs - fnp[0]) / fnp[1]).to(odt).to(F64).numpy()
        assert np.array_equal(host(got["out"]), want), tag + " normalize against NumPy"
    for m in (None, dev(mnp)):
        got = both(tag + f" renormalize int_mask={m is not None}",
                   lambda i, o: raw2("bamd_renormalize", (P(i["x"]), code, n, c, P(i["features"]), P(i["int_mask"]), P(o["out"]), S(i["x"]))),
                   {"x": x, "features": feats, "int_mask": m}, {"out": gb.poisoned((n, c), F64, "cuda")})
        want = xs * fnp[1] + fnp[0]
        if m is not None:
            want[:, mnp != 0] = np.trunc(want[:, mnp != 0])
        assert np.array_equal(host(got["out"]), want), tag + " renormalize against NumPy"

    got = both(tag + " emd_rows", lambda i, o: raw2("bamd_emd_rows", (P(i["x"]), P(i["recon"]), code, n, c, P(o["out"]), S(i["x"]))),
               {"x": x, "recon": r}, {"out": gb.poisoned((1,), F64, "cuda")})
    want = orc.emd_rows(xs, host(r))
    assert abs(got["out"].item() - want) <= 1e-11 * abs(want), tag + " emd_rows against the oracle"

    prior, proj = dev(rng.normal(size=(n, c)), dtype), rng.normal(size=(4, c))
    proj = dev(proj / np.linalg.norm(proj, axis=1, keepdims=True), dtype)
    got = both(tag + " swd", lambda i, o: raw2("bamd_swd", (P(i["z"]), P(i["prior"]), P(i["proj"]), code, n, c, 4, 0.5, P(o["loss"]), P(o["dz"]), S(i["z"]))),
               {"z": x, "prior": prior, "proj": proj}, {"loss": gb.poisoned((1,), F64, "cuda"), "dz": gb.poisoned((n, c), dtype, "cuda")},
               refusal="2 <= n_rows" if n < 2 else None)      # (the kernel sorts a batch: one row is refused)
    if n >= 2:      # the torch restatement and the bars of tests/test_gpu_swae.py
        want_loss, want_dz = _swd_ref(xs, host(prior), host(proj), 0.5)
        tol = 1e-5 if dtype == F32 else 1e-12
        lerr, derr = abs(got["loss"].item() - want_loss) / want_loss, np.linalg.norm(host(got["dz"]) - want_dz) / np.linalg.norm(want_dz)
        print(f"    reference {tag} swd: loss {lerr:.3e} (bar {tol:g}) dz {derr:.3e} (bar {10 * tol:g})")
        assert lerr <= tol and derr <= 10 * tol, tag + " swd against the torch restatement"

    got = both(tag + " error_deltas",
               lambda i, o: raw2("bamd_error_deltas", (P(i["x"]), P(i["recon"]), code, n * c, 10.0, P(o["flags"]), P(o["deltas"]), S(i["x"]))),
               {"x": x, "recon": r}, {"flags": gb.poisoned((n, c), torch.uint8, "cuda"), "deltas": gb.poisoned((n, c), F16, "cuda")})
    npdt = np.float32 if dtype == F32 else np.float64
    want_d, (wr, wc) = odeltas.error_bounded_requirement(10, host(r).astype(npdt), xs.astype(npdt))
    gr, gc = np.nonzero(got["flags"].cpu().numpy())
    assert np.array_equal(gr, wr) and np.array_equal(gc, wc), tag + " error_deltas flags against the oracle"
    assert got["deltas"].cpu().numpy()[wr, wc].tobytes() == np.array(want_d, dtype=np.float16).tobytes(), tag + " error_deltas deltas"

    # apply_deltas: the guard entries of rows / cols are VALID indices that point at trail-guard row n + 5 of the framed table, and
    # the guard deltas are NaN: an over-read of the index lists damages that guard row instead of storing out of range
    k = max(1, (n * c) // 5)
    sel = rng.choice(n * c, size=k, replace=False)
    rows, cols = dev(sel // c, torch.int64), dev(sel % c, torch.int32)
    vals = dev(rng.normal(size=k), F16)
    table = x.clone()
    plain = table.clone()
    native.apply_deltas(plain, rows, cols, vals)
    want = x.cpu().numpy().copy()                                          # (the oracle subtracts in the table's own dtype)
    odeltas.apply_deltas(want, list(vals.cpu().numpy()), ((sel // c), (sel % c)))
    assert np.array_equal(plain.cpu().numpy(), want), tag + " apply_deltas against the oracle"
    for lead in LEADS:
        fr = Frames(lead, tag + " apply_deltas")
        out = fr.out(table, "out")
        native.apply_deltas(out, fr.inp(rows, fill=n + 5), fr.inp(cols, fill=0), fr.inp(vals))
        fr.check()
        assert_same_bits(out, plain, tag + f" apply_deltas lead={lead}")

    # bamd_column_moments / bamd_column_hist against NumPy: the references, edges and bars of tests/test_gpu_colstats.py
    npdt = np.float32 if dtype == F32 else np.float64
    bnp, anp = x.cpu().numpy(), r.cpu().numpy()
    ref, resid, resp, b_, a_ = cst.np_moments(bnp, anp, None)
    got = both(tag + " column_moments",
               lambda i, o: raw2("bamd_column_moments", (P(i["before"]), P(i["after"]), code, n, c, -1, 0.0, P(o["out"]), 0, S(i["before"]))),
               {"before": x, "after": r}, {"out": gb.poisoned((13, c), F64, "cuda")}, same=_sums_close)
    cst.check_exact(cst.raw_dict(got["out"]), ref, tag + " column_moments")
    worst = cst.check_sums(cst.raw_dict(got["out"]), ref, tag + " column_moments")
    print(f"    reference {tag} column_moments: worst sum error {worst:.3e} (bar {cst.TOL:g})")
    acc = both(tag + " column_moments accumulate",
               lambda i, o: raw2("bamd_column_moments", (P(i["before"]), P(i["after"]), code, n, c, -1, 0.0, P(o["out"]), 1, S(i["before"]))),
               {"before": x, "after": r}, {"out": got["out"].clone()}, same=_sums_close)
    assert np.array_equal(host(acc["out"])[0], 2 * host(got["out"])[0])
    twice = {k: (2 * v if k.endswith(("sum", "sumsq")) or k.startswith("abs_") or k == "count" else v) for k, v in ref.items()}
    cst.check_exact(cst.raw_dict(acc["out"]), twice, tag + " column_moments accumulate")
    cst.check_sums(cst.raw_dict(acc["out"]), twice, tag + " column_moments accumulate")
    e_val = cst.value_edges(ref, npdt)
    empty = lambda shape: gb.poisoned(shape, torch.int64, "cuda")        # noqa: E731
    n_er, n_ed, n_ev = len(cst.E_RESP), len(cst.E_RESID), e_val.shape[1]
    got = both(tag + " column_hist",
               lambda i, o: raw2("bamd_column_hist", (P(i["before"]), P(i["after"]), code, n, c, -1, 0.0, P(i["e_resp"]), n_er, P(o["resp"]), P(i["e_resid"]),
                                                      n_ed, P(o["resid"]), P(i["e_val"]), n_ev, P(o["before"]), P(o["after"]), 0, S(i["before"]))),
               {"before": x, "after": r, "e_resp": dev(cst.E_RESP), "e_resid": dev(cst.E_RESID), "e_val": dev(e_val)},
               {"resp": empty((c, n_er - 1)), "resid": empty((c, n_ed - 1)), "before": empty((c, n_ev - 1)), "after": empty((c, n_ev - 1))})
    cst.check_counts(got, cst.np_hists(resid, resp, b_, a_, e_val), tag + " column_hist")
    assert all(int(got[k].sum()) > 0 for k in ("resp", "resid")), tag + " column_hist: the bins caught nothing"
