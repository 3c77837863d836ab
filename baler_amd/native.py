"""ctypes binding of libbaler_amd.so (include/baler_amd.h).

PyTorch is used only as the owner of device memory and of the current HIP stream; every call
below passes raw device pointers (``tensor.data_ptr()``) across the C ABI.  There is NO CPU or
PyTorch fallback: if the library is missing, fails to load, or no gfx950 device is present, the
calls raise ``NativeError``.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BALER_AMD_LIB", os.path.join(_HERE, "libbaler_amd.so"))  # override: kernel A/B experiments

F32, F64 = 0, 1
F16, BF16 = 2, 3        # 16-bit latent codes: the z of bamd_encode / bamd_decode only (include/baler_amd.h, bamd_dtype)
U8 = 8                  # 8-bit latent codes (bamd_code8): the same two places; rint + clamp to [0, 255] on store, exact widening on load



def UB(bits):
    """Code kind of packed ``bits``-bit latent codes, bits = 1 .. 7 (bamd_codeb: BAMD_U1 = 0x101 .. BAMD_U7 = 0x107)."""
    if isinstance(bits, bool) or not isinstance(bits, int) or not 1 <= bits <= 7:
        raise NativeError(f"packed latent codes have 1 to 7 bits, got {bits!r}")
    return 0x100 | bits


def packed_row_bytes(z_dim, bits):
    """Bytes of one packed latent row: ceil(z_dim * bits / 8) (rows are byte-aligned)."""
    return (int(z_dim) * int(bits) + 7) // 8


MODE_F32, MODE_F64, MODE_BF16, MODE_F16 = 0, 1, 2, 3     # MODE_F16: binary16 inference of the 24-column AE, fp32 training
MODE_F16X3 = 5      # fp32 accuracy from three binary16 MFMA products per tile (24-column AE inference, fp32 training); 4 is not a mode
MODE_NAMES = {"fp32": MODE_F32, "f32": MODE_F32, "fp64": MODE_F64, "f64": MODE_F64, "bf16": MODE_BF16, "fp16": MODE_F16, "f16": MODE_F16,
              "fp16x3": MODE_F16X3, "f16x3": MODE_F16X3}
PATH_NAMES = {0: "generic", 1: "fused", 2: "bf16", 3: "fused-infer", 4: "f16", 5: "f16x3"}      # bamd_path
ACT_LEAKY_RELU, ACT_RELU = 0, 1
ACT_NAMES = {"leaky_relu": ACT_LEAKY_RELU, "relu": ACT_RELU}

# every symbol include/baler_amd.h declares (tests check that the library exports all of them)
SYMBOLS = (
    "bamd_abi_version", "bamd_last_error", "bamd_device_count", "bamd_create", "bamd_destroy",
    "bamd_param_count", "bamd_mode_of", "bamd_load_params", "bamd_minmax", "bamd_normalize",
    "bamd_renormalize", "bamd_encode", "bamd_decode", "bamd_forward_loss", "bamd_fwd_bwd",
    "bamd_adam_step", "bamd_train_step", "bamd_emd_rows", "bamd_activation_means",
    "bamd_error_deltas", "bamd_apply_deltas", "bamd_fwd_bwd_latent", "bamd_swd", "bamd_col_minmax", "bamd_path_of",
    "bamd_train_epoch", "bamd_comm_unique_id", "bamd_comm_init", "bamd_comm_attach", "bamd_comm_release", "bamd_comm_world",
    "bamd_allreduce_sum", "bamd_train_epoch_dp", "bamd_create_act", "bamd_act_of", "bamd_create_pjconv",
    "bamd_column_moments", "bamd_column_hist",
)
# the frame statistics of the 2-D report have a header of their own (include/baler_amd_frames.h)
FRAME_SYMBOLS = ("bamd_frame_stats", "bamd_pixel_moments")
PJ_FEATURES = 784      # PJ_Conv_AE: one 28 x 28 frame per row


class NativeError(RuntimeError):
    pass


class AdamHP(ctypes.Structure):
    _fields_ = [("step", ctypes.c_int64), ("lr", ctypes.c_double), ("beta1", ctypes.c_double),
                ("beta2", ctypes.c_double), ("eps", ctypes.c_double)]


_lib = None


def lib():
    """Load libbaler_amd.so (built in-tree by ``make -C baler_amd/csrc`` / ``__graft_entry__.build``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(f"{LIB_PATH} is missing: build it with `make -C baler_amd/csrc` "
                          "(there is no CPU fallback for the hot path)")
    try:
        L = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise NativeError(f"cannot load {LIB_PATH}: {e}") from e
    vp, i64, ci, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
    L.bamd_abi_version.restype = ci
    L.bamd_last_error.restype = ctypes.c_char_p
    L.bamd_device_count.restype = ci
    L.bamd_create.argtypes = [ctypes.POINTER(ci), ci, ci, ci, ctypes.POINTER(vp)]
    L.bamd_create_act.argtypes = [ctypes.POINTER(ci), ci, ci, ci, ci, ctypes.POINTER(vp)]
    L.bamd_act_of.argtypes = [vp]
    L.bamd_create_pjconv.argtypes = [ci, ci, ci, ctypes.POINTER(vp)]
    L.bamd_act_of.restype = ci
    L.bamd_destroy.argtypes = [vp]
    L.bamd_destroy.restype = None
    L.bamd_param_count.argtypes = [vp]
    L.bamd_param_count.restype = i64
    L.bamd_mode_of.argtypes = [vp]
    L.bamd_mode_of.restype = ci
    L.bamd_load_params.argtypes = [vp, vp, ci, vp]
    L.bamd_minmax.argtypes = [vp, ci, i64, ci, vp, vp]
    L.bamd_col_minmax.argtypes = [vp, ci, i64, ci, vp, vp]
    L.bamd_path_of.argtypes = [vp]
    L.bamd_normalize.argtypes = [vp, ci, i64, ci, vp, vp, ci, vp]
    L.bamd_renormalize.argtypes = [vp, ci, i64, ci, vp, vp, vp, vp]
    L.bamd_encode.argtypes = [vp, vp, ci, i64, vp, vp, ci, vp]
    L.bamd_decode.argtypes = [vp, vp, ci, i64, vp, vp, vp, ci, vp]
    L.bamd_forward_loss.argtypes = [vp, vp, ci, i64, vp, vp, ci, vp, vp]
    L.bamd_fwd_bwd.argtypes = [vp, vp, ci, i64, vp, vp, vp]
    L.bamd_adam_step.argtypes = [vp, vp, vp, vp, vp, ctypes.POINTER(AdamHP), vp, vp]
    L.bamd_train_step.argtypes = [vp, vp, ci, i64, vp, vp, vp, vp, vp, ctypes.POINTER(AdamHP), vp, vp]
    L.bamd_train_epoch.argtypes = [vp, vp, ci, i64, i64, vp, vp, vp, vp, vp, ctypes.POINTER(AdamHP), vp, ctypes.POINTER(i64), vp]
    L.bamd_comm_unique_id.argtypes = [vp]
    L.bamd_comm_init.argtypes = [vp, vp, ci, ci]
    L.bamd_comm_attach.argtypes = [vp, vp, ci]
    L.bamd_comm_release.argtypes = [vp]
    L.bamd_comm_world.argtypes = [vp]
    L.bamd_allreduce_sum.argtypes = [vp, vp, ci, i64, vp]
    L.bamd_train_epoch_dp.argtypes = [vp, vp, ci, ctypes.POINTER(i64), i64, vp, vp, vp, vp, vp, ctypes.POINTER(AdamHP), vp, vp]
    L.bamd_emd_rows.argtypes = [vp, vp, ci, i64, ci, vp, vp]
    L.bamd_activation_means.argtypes = [vp, vp, ci, i64, vp, vp, ci, vp]
    L.bamd_error_deltas.argtypes = [vp, vp, ci, i64, dbl, vp, vp, vp]
    L.bamd_fwd_bwd_latent.argtypes = [vp, vp, ci, i64, vp, vp, vp, vp]
    L.bamd_swd.argtypes = [vp, vp, vp, ci, i64, ci, ci, dbl, vp, vp, vp]
    L.bamd_apply_deltas.argtypes = [vp, ci, ci, vp, vp, vp, i64, vp]
    L.bamd_column_moments.argtypes = [vp, vp, ci, i64, ci, ci, dbl, vp, ci, vp]
    L.bamd_column_hist.argtypes = [vp, vp, ci, i64, ci, ci, dbl, vp, ci, vp, vp, ci, vp, vp, ci, vp, vp, ci, vp]
    L.bamd_frame_stats.argtypes = [vp, vp, ci, i64, i64, vp, vp, vp]
    L.bamd_pixel_moments.argtypes = [vp, vp, ci, i64, i64, vp, ci, vp]
    for name in SYMBOLS + FRAME_SYMBOLS:
        getattr(L, name)
    _lib = L
    return L


def _check(rc, what):
    if rc != 0:
        msg = lib().bamd_last_error().decode(errors="replace")
        raise NativeError(f"{what} failed (status {rc}): {msg}")


def _dt(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float64:
        return F64
    raise NativeError(f"unsupported tensor dtype {t.dtype}")


def _dt_latent(t):
    """dtype code of a latent tensor: float32 / float64 as everywhere, or the 16-bit / 8-bit code types of bamd_encode / bamd_decode."""
    if t.dtype == torch.float16:
        return F16
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.uint8:
        return U8
    return _dt(t)


def _dev_tensor(t):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise NativeError("expected a CUDA/HIP tensor (the hot path has no CPU fallback)")
    if not t.is_contiguous():
        raise NativeError("expected a contiguous tensor")
    return t


def _stream(t=None):
    """The current stream OF THE TENSOR'S DEVICE (not of whichever device happens to be current: a stream handle of
    cuda:0 is not valid for buffers and a handle that live on cuda:1)."""
    dev = t.device if t is not None else None
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _same_device(what, first, *others):
    for t in others:
        if t is not None and t.device != first.device:
            raise NativeError(f"{what}: tensors live on different devices ({first.device} vs {t.device})")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def require_gpu():
    n = lib().bamd_device_count()
    if n <= 0 or not torch.cuda.is_available():
        raise NativeError("no MI355X (gfx950) device visible: the baler_amd hot path has no CPU fallback")
    return n


def comm_unique_id():
    """128 bytes identifying a new RCCL communicator (ncclGetUniqueId); rank 0 creates it and sends it to the other ranks."""
    buf = ctypes.create_string_buffer(128)
    _check(lib().bamd_comm_unique_id(buf), "bamd_comm_unique_id")
    return buf.raw


# ---- handle-free kernels --------------------------------------------------------------------------
def minmax(x):
    """data_processing.find_minmax on device: x (n, c) f32/f64 -> (2, c) f64 [min ; max-min]."""
    x = _dev_tensor(x)
    n, c = x.shape
    out = torch.empty((2, c), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().bamd_minmax(_ptr(x), _dt(x), n, c, _ptr(out), _stream(x)), "bamd_minmax")
    return out


def col_minmax(x):
    """Raw column extrema of this rank's rows: x (n, c) f32/f64 -> (2, c) f64 [min ; max] (bamd_col_minmax); the
    data-parallel form of find_minmax all-reduces row 0 with MIN and row 1 with MAX and takes range = max - min."""
    x = _dev_tensor(x)
    n, c = x.shape
    out = torch.empty((2, c), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().bamd_col_minmax(_ptr(x), _dt(x), n, c, _ptr(out), _stream(x)), "bamd_col_minmax")
    return out


def normalize(x, features, out_dtype=torch.float64):
    x = _dev_tensor(x)
    features = _dev_tensor(features)
    n, c = x.shape
    _same_device("normalize", x, features)
    out = torch.empty((n, c), dtype=out_dtype, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().bamd_normalize(_ptr(x), _dt(x), n, c, _ptr(features), _ptr(out), _dt(out), _stream(x)),
               "bamd_normalize")
    return out


def renormalize(x, features, int_mask=None):
    x = _dev_tensor(x)
    n, c = x.shape
    _same_device("renormalize", x, features, int_mask)
    out = torch.empty((n, c), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().bamd_renormalize(_ptr(x), _dt(x), n, c, _ptr(features), _ptr(int_mask), _ptr(out),
                                      _stream(x)), "bamd_renormalize")
    return out


def emd_rows(x, recon):
    """Sum over rows of the 1-D Wasserstein distance between the row's columns of x and recon (bamd_emd_rows): x, recon (n, c)
    f32/f64 with c <= 4096 -> float64[1]; a wider table raises NativeError.  Exact sort, differences in float64, fixed-order sums
    (bitwise repeatable, whatever BALER_AMD_EMD_WGS says).  A NaN in either table gives NaN; +-inf sort as values."""
    x = _dev_tensor(x)
    recon = _dev_tensor(recon)
    if x.dtype != recon.dtype or x.shape != recon.shape:
        raise NativeError("emd_rows: x and recon must have the same dtype and shape")
    _same_device("emd_rows", x, recon)
    out = torch.empty(1, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().bamd_emd_rows(_ptr(x), _ptr(recon), _dt(x), x.shape[0], x.shape[1], _ptr(out), _stream(x)),
               "bamd_emd_rows")
    return out


def swd(z, prior, proj, reg_weight):
    """utils.compute_swd forward + backward: -> (loss float64[1], dz like z).  z, prior (n, d); proj (s, d) unit rows.
    A stable sort: NaN last, ties by row.  A NaN in z gives a NaN loss and NaN in that row of dz alone (include/baler_amd.h)."""
    z, prior, proj = _dev_tensor(z), _dev_tensor(prior), _dev_tensor(proj)
    if not (z.dtype == prior.dtype == proj.dtype) or z.shape != prior.shape or proj.shape[1] != z.shape[1]:
        raise NativeError("swd: z/prior (n, d) and proj (s, d) must share dtype and latent size")
    _same_device("swd", z, prior, proj)
    loss = torch.empty(1, dtype=torch.float64, device=z.device)
    dz = torch.empty_like(z)
    with torch.cuda.device(z.device):
        _check(lib().bamd_swd(_ptr(z), _ptr(prior), _ptr(proj), _dt(z), z.shape[0], z.shape[1], proj.shape[0],
                              float(reg_weight), _ptr(loss), _ptr(dz), _stream(z)), "bamd_swd")
    return loss, dz


def error_deltas(x, recon, bound):
    """helper.save_error_bounded_requirement for a whole table: -> (flags uint8 (n, c), deltas float16 (n, c))."""
    x = _dev_tensor(x)
    recon = _dev_tensor(recon)
    if x.dtype != recon.dtype or x.shape != recon.shape:
        raise NativeError("error_deltas: x and recon must have the same dtype and shape")
    _same_device("error_deltas", x, recon)
    flags = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    deltas = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().bamd_error_deltas(_ptr(x), _ptr(recon), _dt(x), x.numel(), float(bound), _ptr(flags), _ptr(deltas),
                                       _stream(x)), "bamd_error_deltas")
    return flags, deltas


def apply_deltas(out, rows, cols, deltas):
    """out[rows[i], cols[i]] -= deltas[i] in place (rows int64, cols int32, deltas float16; device tensors)."""
    out = _dev_tensor(out)
    rows, cols, deltas = _dev_tensor(rows), _dev_tensor(cols), _dev_tensor(deltas)
    if rows.dtype != torch.int64 or cols.dtype != torch.int32 or deltas.dtype != torch.float16:
        raise NativeError("apply_deltas: rows int64, cols int32, deltas float16 expected")
    if not (rows.numel() == cols.numel() == deltas.numel()):
        raise NativeError("apply_deltas: rows, cols and deltas must have the same length")
    _same_device("apply_deltas", out, rows, cols, deltas)
    with torch.cuda.device(out.device):
        _check(lib().bamd_apply_deltas(_ptr(out), _dt(out), out.shape[1], _ptr(rows), _ptr(cols), _ptr(deltas),
                                       rows.numel(), _stream(out)), "bamd_apply_deltas")
    return out


# rows of bamd_column_moments' (13, n_cols) output (include/baler_amd.h)
MOMENT_ROWS = ("count", "resid_sum", "resid_sumsq", "resid_min", "resid_max", "resp_sum", "resp_sumsq",
               "before_min", "before_max", "after_min", "after_max", "sum_min", "sum_max")
MOMENT_SUM_ROWS, MOMENT_MIN_ROWS, MOMENT_MAX_ROWS = (0, 1, 2, 5, 6), (3, 7, 9, 11), (4, 8, 10, 12)


def _table_pair(what, before, after):
    before, after = _dev_tensor(before), _dev_tensor(after)
    if before.dtype != after.dtype or before.shape != after.shape or before.dim() != 2:
        raise NativeError(f"{what}: before and after must be two (n, c) tables of one dtype and shape")
    _same_device(what, before, after)
    return before, after


def _cut_args(cut):
    """cut = (column, value) or None -> the (cut_col, cut) pair of the C ABI."""
    return (-1, 0.0) if cut is None else (int(cut[0]), float(cut[1]))


def moments_summary(raw):
    """The (13, c) sums / extrema of bamd_column_moments (tensor or array) -> dict of float64 numpy arrays of length c: count,
    resid_mean, resid_rms, resid_min, resid_max, resp_mean, resp_rms, before_min, ..., sum_max (plotting.py:143-147, 203-234:
    mean = sum / count, RMS = sqrt(sum of squares / count))."""
    import numpy as np
    r = raw.detach().cpu().numpy() if isinstance(raw, torch.Tensor) else np.asarray(raw)
    d = dict(zip(MOMENT_ROWS, r))
    with np.errstate(all="ignore"):
        out = {"count": d["count"].astype(np.int64),
               "resid_mean": d["resid_sum"] / d["count"], "resid_rms": np.sqrt(d["resid_sumsq"] / d["count"]),
               "resid_min": d["resid_min"], "resid_max": d["resid_max"],
               "resp_mean": d["resp_sum"] / d["count"], "resp_rms": np.sqrt(d["resp_sumsq"] / d["count"])}
    for k in MOMENT_ROWS[7:]:
        out[k] = d[k]
    return out


def column_moments_raw(before, after, cut=None, out=None):
    """bamd_column_moments: -> the (13, c) float64 device tensor of sums and extrema (rows: MOMENT_ROWS).  With ``out`` (the
    result of an earlier call) this call's rows are ADDED to it: a table can be fed in row chunks."""
    before, after = _table_pair("column_moments", before, after)
    n, c = before.shape
    accumulate = out is not None
    if out is None:
        out = torch.empty((13, c), dtype=torch.float64, device=before.device)
    elif tuple(out.shape) != (13, c) or out.dtype != torch.float64:
        raise NativeError("column_moments: out must be a (13, n_cols) float64 tensor")
    _same_device("column_moments", before, _dev_tensor(out))
    cut_col, cut_val = _cut_args(cut)
    with torch.cuda.device(before.device):
        _check(lib().bamd_column_moments(_ptr(before), _ptr(after), _dt(before), n, c, cut_col, cut_val, _ptr(out),
                                         int(accumulate), _stream(before)), "bamd_column_moments")
    return out


def column_moments(before, after, cut=None, out=None):
    """Per-column residual / response statistics of plotting.plot_1D (see moments_summary) of two device tables; cut = (column,
    value) drops the rows with before[:, column] < value.  ``out``: as in column_moments_raw (the summary is then of all rows so far)."""
    return moments_summary(column_moments_raw(before, after, cut, out))


def column_hist(before, after, edges_resp=None, edges_resid=None, edges_val=None, cut=None, out=None):
    """bamd_column_hist: np.histogram with explicit bins of the response, the residual, ``before`` and ``after`` of every column.
    edges_resp (n_er,), edges_resid (n_ed,), edges_val (c, n_ev): float64 device tensors, or None to skip that histogram.
    edges_resid may also be (c, n_ed): one edge array per column, which need not be evenly spaced and may begin with -inf and
    end with +inf (the C ABI's n_ed < 0; baler_amd/colbox.py selects order statistics with it).
    -> dict of int64 device tensors "resp" (c, n_er - 1), "resid" (c, n_ed - 1), "before" and "after" (c, n_ev - 1) for the
    histograms asked for.  ``out`` (such a dict from an earlier call): the counts of this call's rows are added to it."""
    before, after = _table_pair("column_hist", before, after)
    n, c = before.shape
    accumulate = out is not None
    res = dict(out) if accumulate else {}
    ptr, cnt, sign = {}, {}, {"resid": 1}
    for key, e, names in (("resp", edges_resp, ("resp",)), ("resid", edges_resid, ("resid",)), ("val", edges_val, ("before", "after"))):
        if e is None:
            ptr[key], cnt[key] = None, 0
            continue
        e = _dev_tensor(e)
        want_dim = (2,) if key == "val" else ((1, 2) if key == "resid" else (1,))
        if e.dtype != torch.float64 or e.dim() not in want_dim or (e.dim() == 2 and e.shape[0] != c):
            raise NativeError(f"column_hist: edges_{key} must be float64 of shape " +
                              {"val": "(n_cols, n_edges)", "resid": "(n_edges,) or (n_cols, n_edges)", "resp": "(n_edges,)"}[key])
        _same_device("column_hist", before, e)
        ptr[key], cnt[key] = e, int(e.shape[-1])
        sign[key] = -1 if key == "resid" and e.dim() == 2 else 1       # n_ed < 0: per-column residual edges
        for nm in names:
            if not accumulate:
                res[nm] = torch.empty((c, max(cnt[key] - 1, 0)), dtype=torch.int64, device=before.device)
            elif nm not in res or tuple(res[nm].shape) != (c, cnt[key] - 1) or res[nm].dtype != torch.int64:
                raise NativeError(f"column_hist: out[{nm!r}] must be an int64 tensor of shape (n_cols, n_edges - 1)")
    cut_col, cut_val = _cut_args(cut)
    with torch.cuda.device(before.device):
        _check(lib().bamd_column_hist(_ptr(before), _ptr(after), _dt(before), n, c, cut_col, cut_val,
                                      _ptr(ptr["resp"]), cnt["resp"], _ptr(res.get("resp")),
                                      _ptr(ptr["resid"]), sign["resid"] * cnt["resid"], _ptr(res.get("resid")),
                                      _ptr(ptr["val"]), cnt["val"], _ptr(res.get("before")), _ptr(res.get("after")),
                                      int(accumulate), _stream(before)), "bamd_column_hist")
    return res


# ---- frame statistics: the report mode for 2-D data (include/baler_amd_frames.h) ---------------------------------------------------
# rows of bamd_frame_stats' (10, n_frames) output and of bamd_pixel_moments' (5, frame_elems) output
FRAME_ROWS = ("before_min", "before_max", "after_min", "after_max", "diff_min", "diff_max", "diff_sum", "diff_sumsq",
              "before_sumsq", "nan_count")
PIXEL_ROWS = ("diff_sum", "diff_sumsq", "diff_min", "diff_max", "nan_count")
PIXEL_SUM_ROWS, PIXEL_MIN_ROWS, PIXEL_MAX_ROWS = (0, 1, 4), (2,), (3,)


def _frame_pair(what, before, after):
    """Two device tensors (n, ...) of one dtype and shape, at least 2-D -> their (n, F) views (the checks of _table_pair)."""
    before, after = _dev_tensor(before), _dev_tensor(after)
    if before.dtype != after.dtype or before.shape != after.shape or before.dim() < 2:
        raise NativeError(f"{what}: before and after must be two (n, ...) tables of frames of one dtype and shape")
    _same_device(what, before, after)
    f = 1
    for d in before.shape[1:]:
        f *= int(d)
    if f < 1:
        raise NativeError(f"{what}: frames without elements")
    return before.reshape(before.shape[0], f), after.reshape(after.shape[0], f)


def frame_stats(before, after, diff=None):
    """bamd_frame_stats: -> the (10, n) float64 device tensor of per-frame extrema and sums (rows: FRAME_ROWS) of two device tensors
    (n, ...), d = before - after.  ``diff``: a tensor like ``before`` that receives d bit for bit.  A frame's ten values do not
    depend on n, on its index or on how the table was cut into calls."""
    before, after = _frame_pair("frame_stats", before, after)
    n, f = before.shape
    if diff is not None:
        diff = _dev_tensor(diff)
        if diff.dtype != before.dtype or diff.numel() != before.numel() or (n and diff.shape[0] != n):
            raise NativeError("frame_stats: diff must be a tensor of before's dtype and shape")
        _same_device("frame_stats", before, diff)
    out = torch.empty((len(FRAME_ROWS), n), dtype=torch.float64, device=before.device)
    if n == 0:
        return out
    with torch.cuda.device(before.device):
        _check(lib().bamd_frame_stats(_ptr(before), _ptr(after), _dt(before), n, f, _ptr(out), _ptr(diff), _stream(before)),
               "bamd_frame_stats")
    return out


def frame_summary(raw, frame_elems, dtype=None):
    """The (10, n) rows of bamd_frame_stats (tensor or array) of frames of ``frame_elems`` = F elements -> dict of numpy arrays of
    length n.  vmin / vmax: the colour scale of plotting.plot_2D's three panels (plotting.py:417-418), min / max over both tiles,
    NaN where the frame holds a NaN (np.amin / np.amax propagate it), cast to the table's ``dtype`` (numpy dtype; default float64);
    diff_min, diff_max, diff_mean = sum / F and diff_rms = sqrt(sum of squares / F) of d = before - after; rel_l2 = sqrt(sum d^2 /
    sum before^2); psnr = 20 log10((max - min of before) / diff_rms); nan_count (int64).  Zero denominators give inf / NaN."""
    import numpy as np
    r = raw.detach().cpu().numpy() if isinstance(raw, torch.Tensor) else np.asarray(raw)
    d = dict(zip(FRAME_ROWS, np.asarray(r, dtype=np.float64)))
    f = float(frame_elems)
    dt = np.dtype(np.float64 if dtype is None else dtype)
    has_nan = d["nan_count"] != 0
    with np.errstate(all="ignore"):
        rms = np.sqrt(d["diff_sumsq"] / f)
        out = {"vmin": np.where(has_nan, np.nan, np.minimum(d["before_min"], d["after_min"])).astype(dt),
               "vmax": np.where(has_nan, np.nan, np.maximum(d["before_max"], d["after_max"])).astype(dt),
               "diff_min": d["diff_min"], "diff_max": d["diff_max"],
               "diff_mean": d["diff_sum"] / f, "diff_rms": rms,
               "rel_l2": np.sqrt(d["diff_sumsq"] / d["before_sumsq"]),
               "psnr": 20.0 * np.log10((d["before_max"] - d["before_min"]) / rms),
               "nan_count": d["nan_count"].astype(np.int64)}
    return out


def pixel_moments_raw(before, after, out=None):
    """bamd_pixel_moments: -> the (5, F) float64 device tensor of per-pixel sums, extrema and NaN counts over the frames (rows:
    PIXEL_ROWS) of two device tensors (n, ...), d = before - after.  With ``out`` (the result of an earlier call) this call's frames
    are ADDED to it: a table can be fed in frame chunks."""
    before, after = _frame_pair("pixel_moments", before, after)
    n, f = before.shape
    accumulate = out is not None
    if out is None:
        out = torch.empty((len(PIXEL_ROWS), f), dtype=torch.float64, device=before.device)
    elif tuple(out.shape) != (len(PIXEL_ROWS), f) or out.dtype != torch.float64:
        raise NativeError("pixel_moments: out must be a (5, frame_elems) float64 tensor")
    _same_device("pixel_moments", before, _dev_tensor(out))
    with torch.cuda.device(before.device):
        _check(lib().bamd_pixel_moments(_ptr(before), _ptr(after), _dt(before), n, f, _ptr(out), int(accumulate), _stream(before)),
               "bamd_pixel_moments")
    return out


def pixel_summary(raw, n_frames):
    """The (5, F) rows of bamd_pixel_moments over ``n_frames`` frames (tensor or array) -> dict of numpy arrays of length F:
    pixel_diff_mean = sum / m and pixel_diff_rms = sqrt(sum of squares / m) with m = n_frames - nan_count (a pixel that is NaN in
    every frame: NaN), pixel_diff_min, pixel_diff_max, pixel_nan_count (int64).  A NaN among a pixel's values makes its sums NaN, as
    in numpy; the count says how many frames are behind it."""
    import numpy as np
    r = raw.detach().cpu().numpy() if isinstance(raw, torch.Tensor) else np.asarray(raw)
    d = dict(zip(PIXEL_ROWS, np.asarray(r, dtype=np.float64)))
    m = float(n_frames) - d["nan_count"]
    with np.errstate(all="ignore"):
        m = np.where(m > 0, m, np.nan)
        return {"pixel_diff_mean": d["diff_sum"] / m, "pixel_diff_rms": np.sqrt(d["diff_sumsq"] / m),
                "pixel_diff_min": d["diff_min"], "pixel_diff_max": d["diff_max"],
                "pixel_nan_count": d["nan_count"].astype(np.int64)}


# ---- model handle ---------------------------------------------------------------------------------
class Handle:
    """Owns a bamd_handle*; parameters and optimiser state stay in caller-owned torch tensors."""

    def __init__(self, dims, mode="fp32", device=None, act="leaky_relu"):
        require_gpu()
        self.dims = [int(d) for d in dims]
        self.mode = MODE_NAMES[mode] if isinstance(mode, str) else int(mode)
        act_code = ACT_NAMES[act] if isinstance(act, str) else int(act)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        arr = (ctypes.c_int * len(self.dims))(*self.dims)
        h = ctypes.c_void_p()
        _check(lib().bamd_create_act(arr, len(self.dims) - 1, act_code, self.mode, self.device.index, ctypes.byref(h)),
               "bamd_create_act")
        self._h = h
        self.nparams = int(lib().bamd_param_count(h))
        self.param_dtype = torch.float64 if self.mode == MODE_F64 else torch.float32
        # the mode the library computes in: "bf16" / "fp16" / "fp16x3" asked of a shape without such kernels is served in float32 (notice on stderr)
        self.compute_mode = int(lib().bamd_mode_of(h))

    @classmethod
    def pj_conv(cls, z_dim, mode="fp32", device=None):
        """Handle of PJ_Conv_AE (bamd_create_pjconv): rows of 784 values (one 28 x 28 frame each) in and out, latent z_dim
        (1..2450); every row-based method works unchanged.  "bf16" / "fp16" / "fp16x3" compute in float32 (notice on stderr), "fp64" is refused."""
        require_gpu()
        self = cls.__new__(cls)
        self.dims = [PJ_FEATURES, int(z_dim), PJ_FEATURES]
        self.mode = MODE_NAMES[mode] if isinstance(mode, str) else int(mode)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        h = ctypes.c_void_p()
        _check(lib().bamd_create_pjconv(int(z_dim), self.mode, self.device.index, ctypes.byref(h)), "bamd_create_pjconv")
        self._h = h
        self.nparams = int(lib().bamd_param_count(h))
        self.param_dtype = torch.float32
        self.compute_mode = int(lib().bamd_mode_of(h))
        return self

    @property
    def act(self):
        """The activation the handle computes with: "leaky_relu" or "relu" (bamd_act_of)."""
        return {ACT_LEAKY_RELU: "leaky_relu", ACT_RELU: "relu"}[int(lib().bamd_act_of(self._h))]

    def close(self):
        if getattr(self, "_h", None):
            lib().bamd_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _s(self):
        """Current torch stream of THE HANDLE'S device (the library makes that device current for the call)."""
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _mine(self, *tensors):
        for t in tensors:
            if t is not None and t.device != self.device:
                raise NativeError(f"tensor on {t.device} passed to a handle that lives on {self.device}")

    @property
    def z_dim(self):
        return self.dims[(len(self.dims) - 1) // 2]

    @property
    def path(self):
        """"fused" | "bf16" | "f16" | "f16x3" | "generic" | "fused-infer" (fused encode / decode / validation, layer-wise training): which
        kernels serve this shape's throughput calls (bamd_path_of)."""
        return PATH_NAMES[int(lib().bamd_path_of(self._h))]

    def load_params(self, flat):
        flat = _dev_tensor(flat)
        self._mine(flat)
        if flat.numel() < self.nparams:
            raise NativeError("parameter vector too short")
        _check(lib().bamd_load_params(self._h, _ptr(flat), _dt(flat), self._s()), "bamd_load_params")

    def _out(self, out, rows, cols, dtype, device):
        """Caller-provided output (a contiguous row block of a preallocated result) or a fresh tensor."""
        if out is None:
            return torch.empty((rows, cols), dtype=dtype, device=device)
        _dev_tensor(out)
        self._mine(out)
        if tuple(out.shape) != (rows, cols):
            raise NativeError(f"out has shape {tuple(out.shape)}, expected {(rows, cols)}")
        return out

    def encode(self, x, features=None, out_dtype=None, out=None, code_bits=None):
        """z = encode(x).  out_dtype (or the dtype of ``out``): float32 / float64, or torch.float16 / torch.bfloat16 for 16-bit
        codes -- the round-to-nearest-even conversion of the float32 codes, made on the device by bamd_encode (inside the encode kernel
        for the fp32 register chain, bf16.hip and the layer-wise path; one conversion launch behind a float32 workspace otherwise).
        torch.uint8: 8-bit codes, q = clamp(rint(float32 code), 0, 255) -- workspace and conversion launch for every family; the
        parameters are expected to carry the latent scale (baler_amd.latent8.fold).
        code_bits = b (1 .. 7) with torch.uint8: packed b-bit codes, q = clamp(rint(float32 code), 0, 2**b - 1); the result is
        (n, ceil(z_dim * b / 8)) bytes, each row a little-endian bit string of its codes (baler_amd.latent8.pack_rows).  Without
        code_bits a uint8 output means one byte per code."""
        x = _dev_tensor(x)
        self._mine(x, features)
        if code_bits is None:
            out = self._out(out, x.shape[0], self.z_dim, out_dtype or x.dtype, x.device)
            code = _dt_latent(out)
        else:
            code = UB(code_bits)
            if (out_dtype or torch.uint8) != torch.uint8 or (out is not None and out.dtype != torch.uint8):
                raise NativeError("packed latent codes (code_bits) are written to a uint8 tensor")
            out = self._out(out, x.shape[0], packed_row_bytes(self.z_dim, code_bits), torch.uint8, x.device)
        _check(lib().bamd_encode(self._h, _ptr(x), _dt(x), x.shape[0], _ptr(features), _ptr(out), code,
                                 self._s()), "bamd_encode")
        return out

    def decode(self, z, features=None, int_mask=None, out_dtype=None, out=None, code_bits=None):
        """out = decode(z).  z may hold float16 / bfloat16 / uint8 codes: they are widened exactly, the result is that of the widened
        float32 codes bit for bit (default output dtype then: float32).  code_bits = b (1 .. 7): z holds packed rows of b-bit
        codes, uint8 (n, ceil(z_dim * b / 8)), unpacked the same way."""
        z = _dev_tensor(z)
        self._mine(z, features, int_mask)
        code = _dt_latent(z)
        if code_bits is not None:
            code = UB(code_bits)
            if z.dtype != torch.uint8 or z.dim() != 2 or z.shape[1] != packed_row_bytes(self.z_dim, code_bits):
                raise NativeError(f"z: packed {code_bits}-bit codes of {self.z_dim} columns are uint8 (n_rows, "
                                  f"{packed_row_bytes(self.z_dim, code_bits)}), got {z.dtype} {tuple(z.shape)}")
        default = z.dtype if z.dtype in (torch.float32, torch.float64) else torch.float32
        out = self._out(out, z.shape[0], self.dims[-1], out_dtype or default, z.device)
        _check(lib().bamd_decode(self._h, _ptr(z), code, z.shape[0], _ptr(features), _ptr(int_mask),
                                 _ptr(out), _dt(out), self._s()), "bamd_decode")
        return out

    def forward_loss(self, x, features=None, want_recon=True, loss_out=None):
        x = _dev_tensor(x)
        self._mine(x, features, loss_out)
        recon = torch.empty_like(x) if want_recon else None
        loss = loss_out if loss_out is not None else torch.empty(1, dtype=torch.float64, device=x.device)
        _check(lib().bamd_forward_loss(self._h, _ptr(x), _dt(x), x.shape[0], _ptr(features), _ptr(recon),
                                       _dt(recon) if recon is not None else F32, _ptr(loss), self._s()),
               "bamd_forward_loss")
        return recon, loss

    def fwd_bwd(self, x, grads, features=None):
        x = _dev_tensor(x)
        grads = _dev_tensor(grads)
        self._mine(x, grads, features)
        if grads.dtype != self.param_dtype or grads.numel() < self.nparams + 1:
            raise NativeError("grads must hold param_count+1 elements of the handle's parameter type")
        _check(lib().bamd_fwd_bwd(self._h, _ptr(x), _dt(x), x.shape[0], _ptr(features), _ptr(grads), self._s()),
               "bamd_fwd_bwd")

    def fwd_bwd_latent(self, x, latent_grad, grads, features=None):
        """fwd_bwd with dL/dz of a latent regulariser (n, z_dim; handle parameter type) injected at the bottleneck."""
        x = _dev_tensor(x)
        grads = _dev_tensor(grads)
        latent_grad = _dev_tensor(latent_grad)
        self._mine(x, grads, latent_grad, features)
        if grads.dtype != self.param_dtype or grads.numel() < self.nparams + 1:
            raise NativeError("grads must hold param_count+1 elements of the handle's parameter type")
        if latent_grad.dtype != self.param_dtype or tuple(latent_grad.shape) != (x.shape[0], self.z_dim):
            raise NativeError("latent_grad must be (n_rows, z_dim) of the handle's parameter type")
        _check(lib().bamd_fwd_bwd_latent(self._h, _ptr(x), _dt(x), x.shape[0], _ptr(features), _ptr(latent_grad),
                                         _ptr(grads), self._s()), "bamd_fwd_bwd_latent")

    def adam_step(self, params, grads, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, loss_accum=None):
        self._mine(params, grads, m, v, loss_accum)
        for t in (params, grads, m, v):
            _dev_tensor(t)
            if t.dtype != self.param_dtype:
                raise NativeError("optimizer tensors must have the handle's parameter type")
        hp = AdamHP(int(step), float(lr), float(beta1), float(beta2), float(eps))
        _check(lib().bamd_adam_step(self._h, _ptr(params), _ptr(grads), _ptr(m), _ptr(v), ctypes.byref(hp),
                                    _ptr(loss_accum), self._s()), "bamd_adam_step")

    def train_step(self, x, params, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, loss_accum=None, grads=None,
                   features=None):
        """fwd + loss + bwd + Adam of one batch in one call (= fwd_bwd then adam_step; no all-reduce in between)."""
        x = _dev_tensor(x)
        self._mine(x, params, m, v, grads, loss_accum, features)
        for t in (params, m, v):
            _dev_tensor(t)
            if t.dtype != self.param_dtype:
                raise NativeError("optimizer tensors must have the handle's parameter type")
        if grads is not None and (grads.dtype != self.param_dtype or grads.numel() < self.nparams + 1):
            raise NativeError("grads must hold param_count+1 elements of the handle's parameter type")
        hp = AdamHP(int(step), float(lr), float(beta1), float(beta2), float(eps))
        _check(lib().bamd_train_step(self._h, _ptr(x), _dt(x), x.shape[0], _ptr(features), _ptr(params), _ptr(grads),
                                     _ptr(m), _ptr(v), ctypes.byref(hp), _ptr(loss_accum), self._s()), "bamd_train_step")

    def train_epoch(self, x, batch_size, params, m, v, first_step, lr, beta1=0.9, beta2=0.999, eps=1e-8, loss_accum=None,
                    grads=None, features=None):
        """One epoch of sequential batches over the resident rows `x` in ONE native call (bamd_train_epoch: the batch loop runs
        inside the library, every batch as train_step).  `first_step` = Adam's t of the first batch.  Returns the number of steps."""
        x = _dev_tensor(x)
        self._mine(x, params, m, v, grads, loss_accum, features)
        for t in (params, m, v):
            _dev_tensor(t)
            if t.dtype != self.param_dtype:
                raise NativeError("optimizer tensors must have the handle's parameter type")
        if grads is not None and (grads.dtype != self.param_dtype or grads.numel() < self.nparams + 1):
            raise NativeError("grads must hold param_count+1 elements of the handle's parameter type")
        hp = AdamHP(int(first_step), float(lr), float(beta1), float(beta2), float(eps))
        steps = ctypes.c_int64(0)
        _check(lib().bamd_train_epoch(self._h, _ptr(x), _dt(x), x.shape[0], int(batch_size), _ptr(features), _ptr(params),
                                      _ptr(grads), _ptr(m), _ptr(v), ctypes.byref(hp), _ptr(loss_accum), ctypes.byref(steps),
                                      self._s()), "bamd_train_epoch")
        return int(steps.value)

    # ---- data-parallel training inside the library (RCCL resolved at run time by the library) -----------------------------
    def comm_init(self, unique_id, rank, world):
        """Collective: ncclCommInitRank(world, unique_id, rank) on the handle's device; afterwards train_step / train_epoch_dp run
        fwd_bwd -> ncclAllReduce(sum) -> Adam inside the library.  `unique_id`: the 128 bytes of comm_unique_id() of rank 0."""
        if len(unique_id) != 128:
            raise NativeError("unique_id must be the 128 bytes of comm_unique_id()")
        buf = (ctypes.c_char * 128).from_buffer_copy(bytes(unique_id))
        with torch.cuda.device(self.device):
            _check(lib().bamd_comm_init(self._h, buf, int(rank), int(world)), "bamd_comm_init")

    def comm_attach(self, comm, world=0):
        """Use a communicator the CALLER made (an ncclComm_t as an integer address, from the same RCCL the library resolves); the
        handle never destroys it.  world <= 0: ask ncclCommCount."""
        _check(lib().bamd_comm_attach(self._h, ctypes.c_void_p(int(comm)), int(world)), "bamd_comm_attach")

    def comm_release(self):
        """Detach the communicator (ncclCommDestroy only if comm_init made it); the handle trains single-process again."""
        _check(lib().bamd_comm_release(self._h), "bamd_comm_release")

    @property
    def comm_world(self):
        """Ranks of the communicator attached to this handle (0: none, the handle trains single-process)."""
        return int(lib().bamd_comm_world(self._h))

    def allreduce_sum(self, t):
        """In-place SUM all-reduce of a float32 / float64 tensor over the handle's communicator, on the current stream."""
        t = _dev_tensor(t)
        self._mine(t)
        _check(lib().bamd_allreduce_sum(self._h, _ptr(t), _dt(t), t.numel(), self._s()), "bamd_allreduce_sum")
        return t

    def train_epoch_dp(self, x, batch_rows, params, m, v, first_step, lr, beta1=0.9, beta2=0.999, eps=1e-8, loss_accum=None,
                       grads=None, features=None):
        """One epoch of the data-parallel batch loop in ONE native call: `x` = this rank's rows of every global batch back to back,
        batch_rows[i] = its rows of global batch i (bamd_train_epoch_dp).  Returns the number of steps."""
        x = _dev_tensor(x)
        self._mine(x, params, m, v, grads, loss_accum, features)
        for t in (params, m, v):
            _dev_tensor(t)
            if t.dtype != self.param_dtype:
                raise NativeError("optimizer tensors must have the handle's parameter type")
        if grads is not None and (grads.dtype != self.param_dtype or grads.numel() < self.nparams + 1):
            raise NativeError("grads must hold param_count+1 elements of the handle's parameter type")
        counts = [int(c) for c in batch_rows]
        if sum(counts) != x.shape[0] or any(c < 0 for c in counts):
            raise NativeError("batch_rows must be non-negative and sum to the number of rows of x")
        arr = (ctypes.c_int64 * len(counts))(*counts)
        hp = AdamHP(int(first_step), float(lr), float(beta1), float(beta2), float(eps))
        _check(lib().bamd_train_epoch_dp(self._h, _ptr(x), _dt(x), arr, len(counts), _ptr(features), _ptr(params), _ptr(grads),
                                         _ptr(m), _ptr(v), ctypes.byref(hp), _ptr(loss_accum), self._s()), "bamd_train_epoch_dp")
        return len(counts)

    def activation_means(self, x, features=None, max_nodes=200):
        x = _dev_tensor(x)
        self._mine(x, features)
        out = torch.empty((len(self.dims) - 3, max_nodes), dtype=torch.float64, device=x.device)
        _check(lib().bamd_activation_means(self._h, _ptr(x), _dt(x), x.shape[0], _ptr(features), _ptr(out),
                                           max_nodes, self._s()), "bamd_activation_means")
        return out
