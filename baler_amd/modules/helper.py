"""Facade of the CLI modes (mirror of ``baler/modules/helper.py`` for train/compress/decompress).

Same function names, argument meaning and return shapes as the reference so ``baler_amd.baler`` reads
like ``baler.baler``; the loops inside ``compress`` / ``decompress`` are replaced by ONE native call
per large row block with a pre-allocated output (the reference grows a numpy array by
``np.concatenate`` per 512-row batch, helper.py:608-611,720-723 -- quadratic copying).
"""
import argparse
import importlib
import os
import sys
from dataclasses import dataclass
from math import ceil

import numpy as np
import torch

sys.path.append(os.getcwd())

from .. import colbox
from .. import dist as bdist
from .. import hostio
from .. import latent8
from .. import native
from . import data_processing, training

# rows per native encode/decode call when streaming a dataset through the device
ROW_BLOCK = 1 << 22


def get_arguments(argv=None):
    """reference helper.py:34-101: --mode / --project WORKSPACE PROJECT / --verbose, then
    ``workspaces.<W>.<P>.config.<P>_config.set_config(Config)``."""
    parser = argparse.ArgumentParser(
        prog="baler_amd",
        description="MI355X-native train/compress/decompress path of Baler (same CLI as `baler`).",
        formatter_class=argparse.RawTextHelpFormatter)
    parser.add_argument("--mode", type=str, required=True,
                        help="newProject, train, compress, decompress, report, info")
    parser.add_argument("--project", type=str, required=True, nargs=2, metavar=("WORKSPACE", "PROJECT"),
                        help="Specifies workspace and project, e.g. --project CMS_workspace CMS_project_v1")
    parser.add_argument("--verbose", dest="verbose", action="store_true", help="Verbose mode")
    parser.set_defaults(verbose=False)
    args = parser.parse_args(argv)

    workspace_name, project_name = args.project
    config_path = f"workspaces.{workspace_name}.{project_name}.config.{project_name}_config"
    if args.mode == "newProject":
        config = None
    else:
        config = Config
        importlib.import_module(config_path).set_config(config)
    return config, args.mode, workspace_name, project_name, args.verbose


def create_new_project(workspace_name: str, project_name: str, verbose: bool = False,
                       base_path: str = "workspaces") -> None:
    """reference helper.py:104-147: directory tree + default config."""
    workspace_path = os.path.join(base_path, workspace_name)
    project_path = os.path.join(base_path, workspace_name, project_name)
    if os.path.exists(project_path):
        print(f"The workspace and project ({project_path}) already exists.")
        return
    os.makedirs(project_path)
    required = [
        os.path.join(workspace_path, "data"),
        os.path.join(project_path, "config"),
        os.path.join(project_path, "output", "compressed_output"),
        os.path.join(project_path, "output", "decompressed_output"),
        os.path.join(project_path, "output", "plotting"),
        os.path.join(project_path, "output", "training"),
    ]
    if verbose:
        print(f"Creating project {project_name} in workspace {workspace_name}...")
    for d in required:
        if verbose:
            print(f"Creating directory {d}...")
        os.makedirs(d, exist_ok=True)
    with open(os.path.join(project_path, "config", f"{project_name}_config.py"), "w") as f:
        f.write(create_default_config(workspace_name, project_name))


@dataclass
class Config:
    """Mutable configuration holder: ``set_config(c)`` assigns attributes onto the CLASS, exactly as the
    reference does (helper.py:92-93,150-179), so config modules are interchangeable."""
    input_path: str
    compression_ratio: float
    epochs: int
    early_stopping: bool
    lr_scheduler: bool
    lr_scheduler_patience: int
    min_delta: int
    model_name: str
    custom_norm: bool
    lr: float
    batch_size: int
    test_size: float
    data_dimension: int


def create_default_config(workspace_name: str, project_name: str) -> str:
    """Default project config with the reference's keys (helper.py:182-232)."""
    lines = [
        ("input_path", f'"workspaces/{workspace_name}/data/{project_name}_data.npz"'),
        ("data_dimension", "1"), ("compression_ratio", "2.0"), ("apply_normalization", "True"),
        ("model_name", '"AE"'), ("model_type", '"dense"'), ("epochs", "5"), ("lr", "0.001"),
        ("batch_size", "512"), ("early_stopping", "True"), ("lr_scheduler", "True"),
        ("early_stopping_patience", "100"), ("min_delta", "0"), ("lr_scheduler_patience", "50"),
        ("custom_norm", "False"), ("reg_param", "0.001"), ("RHO", "0.05"), ("test_size", "0"),
        ("extra_compression", "False"), ("intermittent_model_saving", "False"),
        ("intermittent_saving_patience", "100"), ("mse_avg", "False"), ("mse_sum", "True"),
        ("emd", "False"), ("l1", "True"), ("activation_extraction", "False"),
        ("deterministic_algorithm", "True"), ("separate_model_saving", "False"),
        ("save_error_bounded_deltas", "False"), ("error_bounded_requirement", "10"),
        ("convert_to_blocks", "False"),
    ]
    body = "\n".join(f"    c.{k:<30} = {v}" for k, v in lines)
    notes = ("    # --mode report with data_dimension = 2 is opt-in (per-frame and per-pixel statistics, output/plotting/frame_stats.npz):\n"
             "    # c.report_frames = True; c.report_diff = True also stores the difference images; c.report_chunk_rows = frames per device chunk\n")
    return f"\n# === Configuration options ===\n\ndef set_config(c):\n{body}\n{notes}"


def model_init(model_name: str):
    return data_processing.initialise_model(model_name)


def numpy_to_tensor(data):
    return torch.from_numpy(data)


def get_device():
    """reference helper.py:425-439 returns "cuda:0" or "cpu"; here the device is the rank's GPU and a
    missing GPU is an error (no CPU fallback for the hot path)."""
    native.require_gpu()
    return torch.device("cuda", torch.cuda.current_device())


def detacher(tensor):
    return tensor.cpu().detach().numpy()


def normalize(data, custom_norm):
    """reference helper.py:261-274 (per-column min-max over axis 0; identity if custom_norm)."""
    return data_processing.normalize(data, custom_norm)


def renormalize(data, true_min_list, feature_range_list, int_mask=None):
    return data_processing.renormalize_func(data, true_min_list, feature_range_list, int_mask)


def npz_array_shape(path, key):
    """Shape of one array of an .npz archive from its .npy header (np.load(path)[key].shape reads the whole array)."""
    import zipfile
    with zipfile.ZipFile(path) as zf, zf.open(key + ".npy") as f:
        version = np.lib.format.read_magic(f)
        header = np.lib.format.read_array_header_1_0(f) if version == (1, 0) else np.lib.format.read_array_header_2_0(f)
        return tuple(header[0])


def _open_table(path, convert_to_blocks=None):
    """-> (host view of the table -- a memory map when the archive stores it uncompressed --, original shape)."""
    src = hostio.open_npz_array(path, "data")
    original_shape = tuple(src.shape)
    if convert_to_blocks:
        print("Converted Dataset to Blocks of Size - ", convert_to_blocks, " from original ", original_shape)
        src = src.reshape(-1, convert_to_blocks[1], convert_to_blocks[2])   # data_processing.py:26-34 (a view)
    return src, original_shape


def _load_to_device(path, plan=None, convert_to_blocks=None):
    """Rows `plan` (default: all) of the archive's table -> device tensor, streamed through pinned staging."""
    src, original_shape = _open_table(path, convert_to_blocks)
    return hostio.upload_rows(src, plan, get_device()), original_shape


def _minmax_features(local, world):
    """find_minmax (data_processing.py:113-130) of a row-sharded table: per-rank column extrema, MIN / MAX all-reduce,
    range = max - min -- bit-identical to the single-process reduction.  -> (2, prod(shape[1:])) float64, device."""
    flat = local.reshape(local.shape[0], -1)
    if world == 1:
        return native.minmax(flat)
    if flat.shape[0] > 0:
        mm = native.col_minmax(flat)
    else:      # a rank without rows: neutral elements
        mm = torch.stack([torch.full((flat.shape[1],), float("inf"), dtype=torch.float64, device=flat.device),
                          torch.full((flat.shape[1],), float("-inf"), dtype=torch.float64, device=flat.device)])
    bdist.allreduce_minmax(mm)
    return torch.stack([mm[0], mm[1] - mm[0]])


def process(input_path, custom_norm, test_size, apply_normalization, convert_to_blocks, verbose, batch_size=None):
    """reference helper.py:277-319.  Returns (train_set, test_set, normalization_features, original_shape); the
    features are a numpy array as in the reference, the two sets live on the DEVICE (the dataset crosses PCIe once,
    through pinned double-buffered staging).

    Under ``torch.distributed`` with ``batch_size`` given (the GLOBAL batch, dist.global_batch) every rank reads from
    the file, uploads and normalises ONLY the rows it trains on -- its slice of every global batch (SURVEY.md section
    8(e)) -- and the sets are ``training.ShardedRows``; the column min/max comes from one MIN/MAX all-reduce."""
    rank, world = bdist.rank_world()
    src, original_shape = _open_table(input_path, convert_to_blocks)
    if verbose:
        print("Original Dataset Shape - ", tuple(original_shape))
    n = src.shape[0]
    sharded = world > 1 and batch_size is not None
    if not sharded:
        data = hostio.upload_rows(src, None, get_device())
        feats = _minmax_features(data, 1).reshape((2,) + tuple(data.shape[1:]))
        train_plan = test_plan = None
    else:
        if not test_size:
            train_plan = test_plan = hostio.RowPlan.cyclic(n, batch_size, rank, world)
            data = hostio.upload_rows(src, train_plan, get_device())
            feats = _minmax_features(data, world)               # the ranks' shards tile the table
        else:
            tr_idx, te_idx = data_processing.split_indices(n, test_size, random_state=1)
            train_plan = hostio.RowPlan.cyclic(n, batch_size, rank, world, index=tr_idx)
            test_plan = hostio.RowPlan.cyclic(n, batch_size, rank, world, index=te_idx)
            # min/max is over the WHOLE table (helper.py:300-303 runs before the split): a contiguous 1/N slice per
            # rank, streamed through the device once and dropped
            probe = hostio.upload_rows(src, hostio.RowPlan.contiguous(n, rank, world), get_device())
            feats = _minmax_features(probe, world)
            del probe
            data = None
        feats = feats.reshape((2,) + tuple(src.shape[1:]))
    normalization_features = feats.cpu().numpy()

    def norm(t):
        if not (apply_normalization and not custom_norm) or t.shape[0] == 0:
            return t
        flat = t.reshape(t.shape[0], -1)
        return native.normalize(flat.contiguous(), feats.reshape(2, -1).contiguous(), torch.float64).reshape(t.shape)

    if apply_normalization:
        print("Normalizing the data...")
    if not sharded:
        data = norm(data)
        if not test_size:
            return data, data, normalization_features, original_shape
        train_set, test_set = data_processing.split(data, test_size=test_size, random_state=1)
        return train_set, test_set, normalization_features, original_shape

    def shard(plan, local):
        return training.ShardedRows(norm(local), plan.n_global, plan.local_spans, batch_size, rank, world)

    if not test_size:
        train_set = shard(train_plan, data)
        return train_set, train_set, normalization_features, original_shape
    train_set = shard(train_plan, hostio.upload_rows(src, train_plan, get_device()))
    test_set = shard(test_plan, hostio.upload_rows(src, test_plan, get_device()))
    return train_set, test_set, normalization_features, original_shape


def train(model, number_of_columns, train_set, test_set, project_path, config):
    return training.train(model, number_of_columns, train_set, test_set, project_path, config)


def model_saver(model, model_path):
    return data_processing.save_model(model, model_path)


CONV_MODELS = ("PJ_Conv_AE",)


def is_convolutional(config):
    return config.data_dimension == 2 and getattr(config, "model_type", None) != "dense"


def check_convolutional(config):
    """The convolutional configurations baler_amd runs: PJ_Conv_AE (reference models.py:668-715) on 28 x 28 frames (after
    convert_to_blocks) in float32.  Everything else raises here, before the data reaches the GPU."""
    name = config.model_name
    if name not in CONV_MODELS:
        raise NotImplementedError(
            f"convolutional model {name!r} is out of scope: baler_amd runs PJ_Conv_AE only (Conv_AE / Conv_AE_GDN crash on the "
            "shipped data, Conv_AE_3D hard-codes a view, TransformerAE has no encode / decode)")
    shape = npz_array_shape(config.input_path, "data")
    blocks = getattr(config, "convert_to_blocks", None)
    frame = (blocks[1], blocks[2]) if blocks else tuple(shape[1:])
    if tuple(frame) != (28, 28):
        raise NotImplementedError(f"PJ_Conv_AE runs on 28 x 28 frames only (its Linear(2450, 500) fixes the size); got {tuple(frame)}")
    from . import models
    if models._DEFAULT_MODE in ("fp64", "f64"):
        raise NotImplementedError("PJ_Conv_AE computes in float32 only (the reference model is float32); fp64 mode is not supported")
    if getattr(config, "custom_loss_function", None) == "loss_function_swae":
        raise NotImplementedError("the sliced-Wasserstein loss is not supported for PJ_Conv_AE")
    if getattr(config, "save_error_bounded_deltas", False):
        raise NotImplementedError("error-bounded deltas are not supported for PJ_Conv_AE")
    if blocks and getattr(config, "apply_normalization", False):
        raise NotImplementedError(
            "convert_to_blocks with apply_normalization is not supported for PJ_Conv_AE: the reference itself fails in decompress "
            "(operands could not be broadcast together with shapes (16,1,56,56) (28,28))")


def save_final_layer(training_path):
    """training.py:344-346: np.save of np.array(model.get_final_layer_dims()), the decoder's last child -- nn.LeakyReLU(0.2) -- as a
    0-d object array, which the reference's decompress loads (helper.py:650-653).  Written for that reader; nothing here reads it."""
    np.save(os.path.join(training_path, "final_layer.npy"), np.array(torch.nn.LeakyReLU(0.2), dtype=object))


def load_conv_model(config, model_path, z_dim, part=None):
    """PJ_Conv_AE from model.pt, or (separate_model_saving) from encoder.pt / decoder.pt.  The reference loads the prefix-free keys
    of those files with load_state_dict(strict=False) (data_processing.py:108) into a model whose keys carry the encoder. /
    decoder. prefix, so it loads nothing; here the trained half is actually loaded."""
    from . import models
    model = models.PJ_Conv_AE(784, z_dim)
    model.to(get_device())
    sd = torch.load(str(model_path), map_location="cpu")
    if part is None:
        model.load_state_dict(sd, strict=False)
    else:
        model.load_part_state_dict(part, sd)
    return model


def _derive_sizes(config, data_shape, names_len):
    """n_features / latent size exactly as helper.compress derives them (helper.py:505-535)."""
    if config.data_dimension == 1:
        number_of_columns = names_len
        config.latent_space_size = ceil(number_of_columns / config.compression_ratio)
        config.number_of_columns = number_of_columns
        return number_of_columns
    if config.data_dimension == 2:
        if is_convolutional(config):
            # reference baler.py:128-134: the latent size comes from the ORIGINAL frame, even when convert_to_blocks cuts it
            original = npz_array_shape(config.input_path, "data")
            config.number_of_columns = original[2]
            config.latent_space_size = ceil((original[1] * original[2]) / config.compression_ratio)
            return 784
        number_of_rows = data_shape[1]
        config.number_of_columns = data_shape[2]
        config.latent_space_size = ceil((number_of_rows * config.number_of_columns) / config.compression_ratio)
        return number_of_rows * config.number_of_columns
    raise NameError("Data dimension can only be 1 or 2. Got config.data_dimension = "
                    + str(config.data_dimension))


def latent_dtype_of(config):
    """config.latent_dtype -> None | "float16" | "bfloat16" | "uint8" | "uint1" .. "uint7" (hostio.parse_latent_dtype; anything
    else: ValueError)."""
    return hostio.parse_latent_dtype(getattr(config, "latent_dtype", None))


def _check_float16_range(h, flat, feats, out, world):
    """config.latent_dtype = "float16": a latent beyond +-65504 is stored as +-inf and decodes to garbage.  Before anything leaves the
    device: count the inf codes (one accumulation on the device, one read); only if there are any, encode the affected row blocks once
    more at float32 and count those whose float32 latent is finite; refuse to go on if there are any.  Every rank takes part (the
    counts are summed over the ranks) and every rank raises."""
    n_inf = torch.isinf(out).sum().to(torch.float64).reshape(1)
    if world > 1:
        bdist.allreduce_sum(n_inf)
    if int(n_inf.item()) == 0:
        return
    bad = torch.zeros(1, dtype=torch.float64, device=out.device)
    for s in range(0, out.shape[0], ROW_BLOCK):
        e = min(s + ROW_BLOCK, out.shape[0])
        z32 = h.encode(flat[s:e], features=feats, out_dtype=torch.float32)
        bad += (torch.isinf(out[s:e]) & torch.isfinite(z32)).sum()
    if world > 1:
        bdist.allreduce_sum(bad)
    count = int(bad.item())
    if count:
        raise ValueError(f"latent_dtype = \"float16\": {count} latent codes of this model are finite but beyond the float16 range "
                         "(|z| > 65504) and would be stored as +-inf; no archive is written.  Use latent_dtype = \"bfloat16\" "
                         "(float32's range at 8 bits of precision) or leave latent_dtype unset.")


def _calibrate_latent8(h, flat, feats, world, name="uint8"):
    """config.latent_dtype = "uint8" (or "uint1" .. "uint7": ``name``, for the message), first pass: the extrema of every latent column over ALL rows -> (2, z) float64 numpy
    [min ; range].  Per ROW_BLOCK one float32 encode and one bamd_col_minmax; the blocks' 2 x z doubles are combined on the device,
    the ranks' with one MIN and one MAX all-reduce (exact in any order, so every rank count gives the same scale).  A non-finite
    extremum (a NaN or inf latent: bamd_col_minmax propagates NaN) raises ValueError on every rank, before anything is written."""
    z = h.z_dim
    mm = torch.stack([torch.full((z,), float("inf"), dtype=torch.float64, device=flat.device),
                      torch.full((z,), float("-inf"), dtype=torch.float64, device=flat.device)])      # a rank without rows: neutral
    for s in range(0, flat.shape[0], ROW_BLOCK):
        e = min(s + ROW_BLOCK, flat.shape[0])
        blk = native.col_minmax(h.encode(flat[s:e], features=feats, out_dtype=torch.float32))
        nan = torch.isnan(blk).any(dim=0) | torch.isnan(mm).any(dim=0)
        mm = torch.stack([torch.minimum(mm[0], blk[0]), torch.maximum(mm[1], blk[1])])
        mm[:, nan] = float("nan")
    if world > 1:
        bdist.allreduce_minmax(mm)
    mm = mm.cpu().numpy()
    with np.errstate(all="ignore"):
        scale = np.stack([mm[0], mm[1] - mm[0]])
    if not (np.isfinite(mm).all() and np.isfinite(scale).all()):
        bad = int((~(np.isfinite(mm) & np.isfinite(scale)).all(axis=0)).sum())
        raise ValueError(f"latent_dtype = \"{name}\": {bad} of {z} latent columns have a non-finite minimum or maximum over this table "
                         "(a NaN or inf row, or a model that overflows on it), so there is no scale for the codes; no archive is "
                         "written.  Use latent_dtype = \"float16\" / \"bfloat16\" or leave latent_dtype unset.")
    return scale


def _check_fp16_mode_range(h, rows_in, rows_out, world, what):
    """The fp16 and fp16x3 compute modes (BAMD_MODE_F16 / BAMD_MODE_F16X3: binary16 layer inputs, include/baler_amd.h): a value beyond
    +-65504 inside the chain turns every output of ITS row non-finite.  Count, on the device, the rows whose input is entirely finite
    but whose output is not (rows that came in with NaN / inf pass through as in every mode) and refuse to go on if there are any.
    Every rank takes part and every rank raises.  Handles that compute in another mode are not checked."""
    if h.compute_mode not in (native.MODE_F16, native.MODE_F16X3):
        return
    bad = (torch.isfinite(rows_in).all(dim=1) & ~torch.isfinite(rows_out).all(dim=1)).sum().to(torch.float64).reshape(1)
    if world > 1:
        bdist.allreduce_sum(bad)
    count = int(bad.item())
    if count:
        name = "fp16" if h.compute_mode == native.MODE_F16 else "fp16x3"
        raise ValueError(f"BALER_AMD_MODE={name}: {count} rows with finite input left the float16 range (|value| > 65504) inside the "
                         f"model and {what} to non-finite values; nothing is written.  Use the bf16 mode (BALER_AMD_MODE=bf16: "
                         "float32's range at 8 bits of precision) or the fp32 mode (BALER_AMD_MODE=fp32) for this model and data.")


def compress(model_path, config):
    """reference helper.py:473-616.  Returns (compressed ndarray, batches, deltas, indices); the last three are
    empty lists unless ``config.save_error_bounded_deltas`` (then: batch numbers, one float16 array per batch and
    one ``(rows, cols)`` tuple per batch, helper.py:589-606).  The input is re-normalised with ITS OWN min/max
    (helper.py:500-504).  With ``torch.distributed`` every rank reads, uploads and encodes only its contiguous row
    range (no data-path collective; the min/max of the sharded table is one MIN/MAX all-reduce of 2 x C doubles) and
    the latent codes are gathered GPU to GPU onto rank 0, which alone returns them (other ranks: 0 rows).

    Pipeline per rank: file -> pinned staging -> HBM (double buffered), column min/max, then per ROW_BLOCK one
    ``bamd_encode`` with the normalisation fused into the load (evaluated in float64 on the UNCAST source values, as
    the reference normalises before it casts, helper.py:500-504,560-563), the download of block k overlapping the
    encode of block k+1.

    ``config.latent_dtype`` = "float16" / "bfloat16": the latent buffer has that dtype -- bamd_encode rounds the codes on the device, so
    the gather, the download and the archive move 2 bytes per code; float16 codes come back as a numpy float16 array, bfloat16 codes
    as their uint16 bit patterns (hostio.latent_to_archive).  The deltas side channel is computed from decode() of the ROUNDED codes,
    which is what decompress will decode.

    ``config.latent_dtype`` = "uint8": two passes.  The first finds the extrema of every latent column (_calibrate_latent8); the map
    of [min, min + range] onto [0, 255] is then folded into the last encoder and the first decoder layer of THIS RUN's copy of the
    parameters (baler_amd.latent8; model.pt is not touched), and the second pass encodes to bytes: 1 byte per code.  The scale is
    left in ``config.latent_scale`` for the archive; the deltas come from decode() of the bytes on the folded handle.

    ``config.latent_dtype`` = "uint1" .. "uint7": the same two passes with 2**b - 1 in the place of 255; the second pass writes
    packed rows of ceil(z * b / 8) bytes (bamd_codeb; baler_amd.latent8.pack_rows states the layout), which every later step
    -- row blocks, the gather, the archive -- moves as plain byte rows."""
    want_deltas = bool(getattr(config, "save_error_bounded_deltas", False))
    latent_dtype = latent_dtype_of(config)          # (a bad value fails here, before any GPU work)
    rank, world = bdist.rank_world()
    src, original_shape = _open_table(config.input_path, getattr(config, "convert_to_blocks", None) or None)
    names = np.load(config.input_path)["names"]
    n_features = _derive_sizes(config, src.shape, len(names))
    n_total = src.shape[0]
    plan = hostio.RowPlan.contiguous(n_total, rank, world)
    flat = hostio.upload_rows(src, plan, get_device())
    flat = flat.reshape(flat.shape[0], -1)
    feats = None
    if config.apply_normalization and not config.custom_norm:
        print("Normalizing...")
        feats = _minmax_features(flat, world)
    # reference: 1-D tables stay float64, 2-D ones become float32 AFTER normalisation (helper.py:560-563)
    work_dtype = torch.float32 if config.data_dimension == 2 else flat.dtype
    if feats is None and flat.dtype != work_dtype:
        flat = flat.to(work_dtype)

    if is_convolutional(config):
        model = load_conv_model(config, model_path, config.latent_space_size,
                                "encoder" if getattr(config, "separate_model_saving", False) else None)
    else:
        model = data_processing.load_model(data_processing.initialise_model(config.model_name), model_path,
                                           n_features=n_features, z_dim=config.latent_space_size)
    model.eval()
    h = model.handle()
    n_local = flat.shape[0]
    bits = hostio.latent_bits(latent_dtype)      # None | 8 ("uint8") | 1 .. 7 (packed rows)
    packed = bits if bits is not None and bits < 8 else None
    if bits is not None:
        # the affine map of the codes goes INTO the model of this run (model.pt stays as it is): from here on h emits the latent in
        # code units [0, 2**bits - 1], and decodes them.  config.latent_scale: what perform_compression writes next to the codes.
        config.latent_scale = _calibrate_latent8(h, flat, feats, world, latent_dtype)
        model.load_flat(latent8.fold(model, config.latent_scale[0], config.latent_scale[1], latent8.levels(bits)))
        h = model.handle()
    width = config.latent_space_size if packed is None else hostio.packed_row_bytes(config.latent_space_size, packed)
    out = torch.empty((n_local, width), dtype=hostio.LATENT_DTYPES.get(latent_dtype, work_dtype), device=flat.device)
    if want_deltas:
        flags = torch.empty((n_local, n_features), dtype=torch.uint8, device=flat.device)
        deltas = torch.empty((n_local, n_features), dtype=torch.float16, device=flat.device)
    ready = []
    for s in range(0, n_local, ROW_BLOCK):
        e = min(s + ROW_BLOCK, n_local)
        if not want_deltas:
            h.encode(flat[s:e], features=feats, out=out[s:e], code_bits=packed)
        else:
            # the side channel compares decode(encode(x)) with the NORMALISED input (helper.py:589-606)
            xn = native.normalize(flat[s:e], feats, out_dtype=work_dtype) if feats is not None else flat[s:e]
            h.encode(xn, out=out[s:e], code_bits=packed)
            flags[s:e], deltas[s:e] = native.error_deltas(xn, h.decode(out[s:e], out_dtype=xn.dtype, code_bits=packed),
                                                          config.error_bounded_requirement)
        ev = torch.cuda.Event()
        ev.record()
        ready.append((e, ev))
    if latent_dtype == "float16":       # before the gather and the download: an overflowing run fails without moving the codes
        _check_float16_range(h, flat, feats, out, world)
    checked = out
    if bits is not None and h.compute_mode in (native.MODE_F16, native.MODE_F16X3):
        # a byte (or a packed code) cannot show a non-finite latent (NaN is stored as 0): the fp16 modes' range check reads the folded handle's float32
        # latent instead -- a tiny range makes a large folded weight, which can leave the float16 range where the plain model did not
        checked = torch.empty((n_local, config.latent_space_size), dtype=torch.float32, device=out.device)
        for s in range(0, n_local, ROW_BLOCK):
            e = min(s + ROW_BLOCK, n_local)
            h.encode(flat[s:e], features=feats, out=checked[s:e])
    _check_fp16_mode_range(h, flat, checked, world, "encode")
    # bfloat16 codes travel as a float16-typed view: a 2-byte carrier every collective and numpy know; no copy interprets it
    compressed = _gather_rows(out.view(torch.float16) if latent_dtype == "bfloat16" else out, n_total, world, ready)
    if latent_dtype == "bfloat16":
        compressed = compressed.view(np.uint16)
    if not want_deltas:
        return compressed, [], [], []
    flags = _gather_rows(flags, n_total, world)
    deltas = _gather_rows(deltas, n_total, world)
    if rank != 0:
        return compressed, [], [], []
    return (compressed,) + split_deltas(flags, deltas, config.batch_size)


def save_error_bounded_requirement(config, decoded_output, data_batch):
    """reference helper.py:442-470 for ONE batch of host arrays (kept for callers of the reference function; the
    compress path evaluates the whole table at once): -> (list of float16 deltas, (rows, cols))."""
    dev = get_device()
    x = torch.as_tensor(np.ascontiguousarray(data_batch), device=dev)
    r = torch.as_tensor(np.ascontiguousarray(decoded_output), device=dev).to(x.dtype)
    flags, deltas = native.error_deltas(x, r, config.error_bounded_requirement)
    rows, cols = np.nonzero(flags.cpu().numpy())
    return list(deltas.cpu().numpy()[rows, cols]), (rows, cols)


def split_deltas(flags, deltas, batch_size):
    """Dense (flags, float16 deltas) of the whole table -> the reference's per-batch side channel
    (helper.py:589-606): batch numbers, flagged deltas (row-major, as ``np.where`` orders them) and
    ``(rows, cols)`` with rows counted inside the batch.  Every batch is listed, flagged or not."""
    batches, out_deltas, out_index = [], [], []
    for idx, s in enumerate(range(0, flags.shape[0], batch_size)):
        rows, cols = np.nonzero(flags[s:s + batch_size])
        batches.append(idx)
        out_deltas.append(np.ascontiguousarray(deltas[s:s + batch_size][rows, cols]))
        out_index.append((rows, cols))
    print("Total Deltas Found - ", int(sum(len(d) for d in out_deltas)))
    return batches, out_deltas, out_index


def save_deltas(comp_dir, batches, deltas, index):
    """baler.py:316-338: the two gzip'd ``np.save`` object arrays the reference's decompress reads back
    (``compressed_deltas.npz.gz``: one entry per batch; ``compressed_batch_index_metadata.npz.gz``:
    ``[batch numbers, (rows, cols) per batch]``).  Entries are float16 ARRAYS where the reference stored Python
    lists of float16 scalars -- the consumer indexes them the same way (helper.py:708-718)."""
    import gzip
    d_arr = np.empty(len(batches), dtype=object)
    i_arr = np.empty((2, len(batches)), dtype=object)
    for k, b in enumerate(batches):
        d_arr[k] = deltas[k]
        i_arr[0, k] = b
        i_arr[1, k] = index[k]
    with gzip.GzipFile(os.path.join(comp_dir, "compressed_deltas.npz.gz"), "w") as f:
        np.save(file=f, arr=d_arr)
    with gzip.GzipFile(os.path.join(comp_dir, "compressed_batch_index_metadata.npz.gz"), "w") as f:
        np.save(file=f, arr=i_arr)


def load_deltas(input_path_deltas, input_batch_index, batch_size):
    """Side channel files -> flat (global rows int64, cols int32, deltas float16) host arrays (helper.py:655-665)."""
    import gzip
    loaded_deltas = np.load(gzip.GzipFile(input_path_deltas, "r"), allow_pickle=True)
    loaded_index = np.load(gzip.GzipFile(input_batch_index, "r"), allow_pickle=True)
    rows, cols, vals = [], [], []
    for k, b in enumerate(loaded_index[0]):
        r, c = loaded_index[1][k]
        rows.append(np.asarray(r, dtype=np.int64) + int(b) * batch_size)
        cols.append(np.asarray(c, dtype=np.int32))
        vals.append(np.asarray(loaded_deltas[k], dtype=np.float16).reshape(-1))
    if not rows:
        return np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float16)
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)


def _gather_rows(local, n_total, world, ready=None):
    """Per-rank row shards (contiguous ranges in rank order) -> ONE host array on rank 0; other ranks get a 0-row
    array (only rank 0 writes artefacts).  Multi-rank: one device-to-device gather onto rank 0 (dist.gather_rows, RCCL
    over xGMI), then a single pinned, double-buffered download -- nothing is pickled and no rank but 0 touches PCIe.
    ``ready``: per-block completion events of the producer (single rank: the download of block k overlaps block k+1)."""
    if world == 1:
        return hostio.download_rows(local, ready=ready)
    full = bdist.gather_rows(local, n_total, dst=0)
    if full is None:
        return np.empty((0,) + tuple(local.shape[1:]), dtype=hostio.NP_OF_TORCH[local.dtype])
    return hostio.download_rows(full)


def decompress(model_path, input_path, input_path_deltas, input_batch_index, model_name, config,
               output_path, original_shape, renorm=None):
    """reference helper.py:619-733.  Returns (decompressed ndarray, names, normalization_features).  With
    ``config.save_error_bounded_deltas`` the stored float16 deltas are subtracted from the decoder output of
    their batch (helper.py:708-718), on the device, before un-normalisation.

    ``renorm`` (not in the reference signature; optional): ``(features (2, C) float64, int_mask or None)``.  When
    given, the un-normalisation ``x*range + min`` and the truncation of the "int" columns that the reference applies
    afterwards on the host (baler.py:410-435) run on the device -- fused into the decode kernel's store when there are
    no deltas -- so the decompressed table crosses PCIe once (float64) instead of three times."""
    loaded = np.load(input_path)
    data = hostio.open_npz_array(input_path, "data")     # memory-mapped when stored: a rank reads only its rows
    names = loaded["names"]
    normalization_features = loaded["normalization_features"]
    # 16-bit codes are recognised from the ARCHIVE (data.dtype / its latent_dtype key), never from the config
    data, code_dtype = hostio.latent_from_archive(data, loaded.files, lambda k: loaded[k])
    latent_scale = hostio.latent_scale_from_archive(data, loaded.files, lambda k: loaded[k])      # 8-bit and packed codes only (else None)
    bits = hostio.latent_bits(str(loaded["latent_dtype"])) if latent_scale is not None else None
    packed = bits if bits is not None and bits < 8 else None      # packed rows: data is (N, ceil(z * bits / 8)) bytes
    latent_space_size = data.shape[1] if packed is None else latent_scale.shape[1]
    model_dict = torch.load(str(model_path), map_location="cpu")
    number_of_columns = len(model_dict[list(model_dict.keys())[-1]])  # len(de4.bias), helper.py:668-674

    if is_convolutional(config):
        number_of_columns = 784          # one 28 x 28 frame per row
        model = load_conv_model(config, model_path, latent_space_size,
                                "decoder" if getattr(config, "separate_model_saving", False) else None)
    else:
        model = data_processing.load_model(data_processing.initialise_model(config.model_name), model_path,
                                           n_features=number_of_columns, z_dim=latent_space_size)
    model.eval()
    if latent_scale is not None:      # 8-bit codes: this run's copy of the parameters decodes code units (model.pt is not touched)
        model.load_flat(latent8.fold(model, latent_scale[0], latent_scale[1], latent8.levels(bits)))
    h = model.handle()
    rank, world = bdist.rank_world()
    n_total = data.shape[0]
    lo, hi = bdist.shard_rows(n_total, rank, world)
    # this rank's latent rows only, through pinned double-buffered staging
    z = hostio.upload_rows(data, hostio.RowPlan.contiguous(n_total, rank, world), get_device(), keep_half=code_dtype is not None)
    if code_dtype is not None:
        z = z.view(code_dtype)
    # what the decoder writes without the fused epilogue: the codes' own dtype, or the working precision compress() had for 16-bit codes
    plain_dtype = z.dtype if code_dtype is None else (torch.float32 if config.data_dimension == 2 else torch.float64)
    want_deltas = bool(getattr(config, "save_error_bounded_deltas", False))
    r_feats = r_mask = None
    if renorm is not None:
        r_feats = torch.as_tensor(np.asarray(renorm[0], dtype=np.float64).reshape(2, -1), device=z.device).contiguous()
        if renorm[1] is not None:
            r_mask = torch.as_tensor(np.asarray(renorm[1], dtype=np.uint8), device=z.device).contiguous()
    fuse = renorm is not None and not want_deltas
    out = torch.empty((hi - lo, number_of_columns), dtype=torch.float64 if fuse else plain_dtype, device=z.device)
    ready = []
    for s in range(0, hi - lo, ROW_BLOCK):
        e = min(s + ROW_BLOCK, hi - lo)
        if fuse:
            h.decode(z[s:e], features=r_feats, int_mask=r_mask, out=out[s:e], code_bits=packed)
        else:
            h.decode(z[s:e], out=out[s:e], code_bits=packed)
        ev = torch.cuda.Event()
        ev.record()
        ready.append((e, ev))
    _check_fp16_mode_range(h, z, out, world, "decode")
    if want_deltas:
        ready = None
        rows, cols, vals = load_deltas(input_path_deltas, input_batch_index, config.batch_size)
        mine = (rows >= lo) & (rows < hi)                     # this rank's row shard
        dev = out.device
        native.apply_deltas(out, torch.from_numpy(rows[mine] - lo).to(dev), torch.from_numpy(cols[mine]).to(dev),
                            torch.from_numpy(vals[mine]).to(dev))
        print("Total Deltas Added - ", int(len(rows)))
        if renorm is not None:
            out = native.renormalize(out, r_feats, r_mask)
    decompressed = _gather_rows(out, n_total, world, ready)
    if rank != 0:
        return decompressed, names, normalization_features
    if is_convolutional(config):
        decompressed = decompressed.reshape((len(decompressed), 1, 28, 28))     # what PJ_Conv_AE.decode returns
    if config.data_dimension == 2 and getattr(config, "model_type", None) == "dense":
        blocks = getattr(config, "convert_to_blocks", None)
        if blocks:
            # rows are blocks here, not frames.  The reference reshapes with the FRAME shape (helper.py:728-731) and so
            # raises ValueError for its own exafel1/exafel2 configs (dense model + convert_to_blocks); the caller
            # (perform_decompression, baler.py:394-408) folds the blocks back into frames.
            decompressed = decompressed.reshape((len(decompressed), blocks[1], blocks[2]))
        else:
            decompressed = decompressed.reshape((len(decompressed), original_shape[1], original_shape[2]))
    return decompressed, names, normalization_features


# ---- --mode report: the data path of plotting.plot_1D ----------------------------------------------------------------------------
REPORT_CUT = (3, 1e-6)      # plotting.py:118: get_index_to_cut(3, 1e-6, before), hard-coded in the reference


def report_response_edges():
    return np.arange(-20, 20, 0.1)          # plotting.py:194


def report_residual_edges():
    return np.arange(-1, 1, 0.01)           # plotting.py:217


def report_value_edges(x_min, x_max):
    """plotting.py:146-153 with x_min / x_max = the extrema of before + after of one column (scalars of the table's dtype)."""
    x_diff = abs(x_max - x_min)
    return np.linspace(x_min - 0.1 * x_diff, x_max + 0.1 * x_diff, 200)


def report_cut(config, n_cols):
    """The row cut of the report: config.report_cut = (column, value) or None when the config sets it; else the reference's
    (3, 1e-6) for tables of more than 3 columns (the reference indexes column 3 unconditionally) and no cut for narrower ones."""
    if hasattr(config, "report_cut"):
        cut = config.report_cut
        if cut is None:
            return None
        col, value = int(cut[0]), float(cut[1])
        if not 0 <= col < n_cols:
            raise ValueError(f"report_cut column {col} is outside the table's {n_cols} columns")
        return col, value
    return REPORT_CUT if n_cols > 3 else None


def report_kernel_cut(cut, dtype):
    """The cut as the kernels take it.  numpy compares a float32 column with the Python float in float32 (plotting.py:72), the
    kernels compare as float64: the threshold rounded to the table's dtype makes the two agree on every row."""
    return None if cut is None else (int(cut[0]), float(np.dtype(dtype).type(cut[1])))


def report_chunk_rows(config, row_bytes):
    """Rows per device chunk of the report: config.report_chunk_rows, else what fills one of hostio's staging buffers."""
    rows = getattr(config, "report_chunk_rows", None)
    return max(1, int(rows)) if rows else max(1, hostio.CHUNK_BYTES // max(1, row_bytes))


def check_report(config):
    if config.data_dimension != 1:
        raise NotImplementedError("--mode report serves data_dimension = 1 (plotting.plot_1D); plotting.plot_2D has no native "
                                  "path: run the reference's plot mode on the artefacts, or set c.report_frames = True for the "
                                  "per-frame and per-pixel statistics behind its pages (helper.frame_report)")


def column_report(config, output_path, verbose=False):
    """The data path of plotting.plot_1D (plotting.py:101-239) on the device: per column the mean / RMS of the residual
    after - before and of the response (after - before) / before * 100, the residual's extrema, and the response, residual,
    before and after histograms with the reference's bins.  Both tables stream through the GPU in row chunks, twice: moments,
    then -- the value bins come from the before + after extrema -- histograms; the tables never have to fit on the device.
    Under data parallelism each rank takes a contiguous row slice; sums and counts are SUM-, extrema MIN- / MAX-all-reduced.
    config.report_box (default True) adds the box-and-whisker statistics of the residual (box_q1, box_med, box_q3, box_whislo,
    box_whishi, box_edge: matplotlib's boxplot_stats, plotting.py:76-98) by exact selection, a few more sweeps; the chunks stay on the
    device across them when the rank's two slices fit in config.report_box_resident_mb (default 1024) MB, else they stream again.
    Returns the dict that rank 0 also writes to output/plotting/column_stats.npz."""
    check_report(config)
    device = get_device()
    rank, world = bdist.rank_world()
    before = hostio.open_npz_array(config.input_path, "data")
    after = hostio.open_npz_array(os.path.join(output_path, "decompressed_output", "decompressed.npz"), "data")
    names = np.load(config.input_path)["names"]
    if before.ndim != 2 or before.shape != after.shape:
        raise ValueError(f"report: input {before.shape} and decompressed {after.shape} must be two tables of one shape")
    n, c = before.shape
    cut = report_cut(config, c)
    t_dtype, h_dtype = hostio._device_dtype(np.result_type(before.dtype, after.dtype))
    shown_cut, cut = cut, report_kernel_cut(cut, h_dtype)
    lo, hi = bdist.shard_rows(n, rank, world)
    chunk = report_chunk_rows(config, 2 * c * np.dtype(h_dtype).itemsize)

    def chunks():
        for a in range(lo, hi, chunk):
            plan = hostio.RowPlan("range", n, lo=a, hi=min(a + chunk, hi), count=min(a + chunk, hi) - a)
            b_dev, a_dev = hostio.upload_rows(before, plan, device), hostio.upload_rows(after, plan, device)
            yield b_dev.to(t_dtype), a_dev.to(t_dtype)      # (a no-op unless the two archives differ in dtype)

    # sweep 1: moments
    empty = torch.empty((0, c), dtype=t_dtype, device=device)
    raw = native.column_moments_raw(empty, empty, cut)           # the neutral elements (a rank may own no rows)
    for b_dev, a_dev in chunks():
        native.column_moments_raw(b_dev, a_dev, cut, out=raw)
    if world > 1:
        import torch.distributed as td
        for rows, op in ((native.MOMENT_SUM_ROWS, td.ReduceOp.SUM), (native.MOMENT_MIN_ROWS, td.ReduceOp.MIN),
                         (native.MOMENT_MAX_ROWS, td.ReduceOp.MAX)):
            part = raw[list(rows)].contiguous()
            td.all_reduce(part, op=op)
            raw[list(rows)] = part
    stats = native.moments_summary(raw)

    # the reference's bins, built by the very numpy calls it uses
    e_resp, e_resid = report_response_edges(), report_residual_edges()
    with np.errstate(invalid="ignore"):      # a column without kept values: NaN edges, nothing is counted
        e_val = np.stack([np.asarray(report_value_edges(h_dtype(stats["sum_min"][k]), h_dtype(stats["sum_max"][k])), dtype=np.float64)
                          for k in range(c)])
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).to(device)   # noqa: E731
    d_resp, d_resid, d_val = dev(e_resp), dev(e_resid), dev(e_val)

    # sweep 2: histograms
    counts = native.column_hist(empty, empty, d_resp, d_resid, d_val, cut)    # zeros
    for b_dev, a_dev in chunks():
        native.column_hist(b_dev, a_dev, d_resp, d_resid, d_val, cut, out=counts)
    if world > 1:
        for t in counts.values():
            bdist.allreduce_sum(t)
    result = {"names": names, "cut": np.array(shown_cut if shown_cut is not None else (-1, 0.0), dtype=np.float64)}
    result.update(stats)
    result.update(edges_response=e_resp, edges_residual=e_resid, edges_value=e_val,
                  counts_response=counts["resp"].cpu().numpy(), counts_residual=counts["resid"].cpu().numpy(),
                  counts_before=counts["before"].cpu().numpy(), counts_after=counts["after"].cpu().numpy())

    # the box-and-whisker page (plotting.py:76-98): exact order statistics of the residual by bracket descent (colbox.py); every
    # round is one more sweep of bamd_column_hist with per-column edges, its int64 counts SUM-all-reduced
    box = None
    if getattr(config, "report_box", True):
        mine = 2 * (hi - lo) * c * np.dtype(h_dtype).itemsize
        resident = list(chunks()) if mine <= float(getattr(config, "report_box_resident_mb", 1024)) * 2 ** 20 else None

        def hist(edges):
            d_edges = dev(edges)
            got = native.column_hist(empty, empty, edges_resid=d_edges, cut=cut)
            for b_dev, a_dev in (resident if resident is not None else chunks()):
                native.column_hist(b_dev, a_dev, edges_resid=d_edges, cut=cut, out=got)
            if world > 1:
                bdist.allreduce_sum(got["resid"])
            return got["resid"].cpu().numpy()

        box, box_info = colbox.box_stats(stats["count"], stats["resid_min"], stats["resid_max"], hist, h_dtype)
        result.update(box)
    if rank == 0:
        os.makedirs(os.path.join(output_path, "plotting"), exist_ok=True)
        np.savez(os.path.join(output_path, "plotting", "column_stats.npz"), **result)
        print("=== Column report ===")
        for k in range(c):
            print(f"{str(names[k]).split('.')[-1]}: residual mean {stats['resid_mean'][k]:.6g} RMS {stats['resid_rms'][k]:.6g} "
                  f"min {stats['resid_min'][k]:.6g} max {stats['resid_max'][k]:.6g}; response mean {stats['resp_mean'][k]:.4g} % "
                  f"RMS {stats['resp_rms'][k]:.4g} %")
        if box is not None:
            print(f"=== Box and whisker === ({box_info['rounds']} sweeps, {'resident' if resident is not None else 'streamed'}; "
                  f"x axis half-width {float(box['box_edge']):.6g})")
            for k in range(c):
                print(f"{str(names[k]).split('.')[-1]}: q1 {box['box_q1'][k]:.6g} median {box['box_med'][k]:.6g} q3 {box['box_q3'][k]:.6g} "
                      f"whiskers {box['box_whislo'][k]:.6g} .. {box['box_whishi'][k]:.6g}")
    return result


# ---- --mode report for 2-D data: the data path of plotting.plot_2D, opt-in with config.report_frames -------------------------------
def report_frames_on(config):
    return config.data_dimension == 2 and bool(getattr(config, "report_frames", False))


def _frame_tables(config, output_path):
    """The two host arrays of the 2-D report (memory maps where the archives store them), `after` viewed in `before`'s shape; every
    shape refusal, before any GPU work."""
    if config.data_dimension != 2:
        raise ValueError(f"frame_report serves data_dimension = 2, not {config.data_dimension} (1-D data: column_report)")
    before = hostio.open_npz_array(config.input_path, "data")
    after = hostio.open_npz_array(os.path.join(output_path, "decompressed_output", "decompressed.npz"), "data")
    ok = before.ndim >= 2 and after.ndim >= 1 and before.shape[0] == after.shape[0]
    elems = int(np.prod(before.shape[1:])) if before.ndim >= 2 else 0
    if not ok or elems < 1 or after.size != before.shape[0] * elems:
        raise ValueError(f"report: input {tuple(before.shape)} must be frames (n, ...) and decompressed {tuple(after.shape)} must hold as "
                         "many frames of as many elements each")
    # PJ_Conv_AE writes (N, 1, 28, 28), a block run may leave blocks or flat rows: plot_2D reshapes too (plotting.py:388-391)
    return before, after.reshape(before.shape)


def frame_report(config, output_path, verbose=False):
    """The data path of plotting.plot_2D (plotting.py:370-437) on the device, for every frame: the colour scale vmin / vmax of its
    three panels and the difference image d = before - after behind the third, plus per-frame error figures (diff_min, diff_max,
    diff_mean, diff_rms, rel_l2, psnr, nan_count: native.frame_summary) and the per-pixel error map over all frames
    (pixel_diff_mean, pixel_diff_rms, pixel_diff_min, pixel_diff_max, pixel_nan_count in the frame's shape: native.pixel_summary).
    Both tables stream through the GPU once, in chunks of config.report_chunk_rows frames (default: what fills one of hostio's
    staging buffers, at least one frame -- a frame larger than a staging buffer grows the buffer); per chunk one bamd_frame_stats
    and one bamd_pixel_moments call.  Under data parallelism each rank takes a contiguous slice of the frames: the per-frame rows
    are gathered in rank order (never summed: a frame's values are the bits one rank computed), the pixel sums and counts are SUM-,
    the pixel extrema MIN- / MAX-all-reduced.  config.report_diff = True (default False) also stores `diff`, every difference image.
    Returns the dict that rank 0 also writes to output/plotting/frame_stats.npz."""
    before, after = _frame_tables(config, output_path)
    device = get_device()
    rank, world = bdist.rank_world()
    n, shape = before.shape[0], tuple(before.shape[1:])
    elems = int(np.prod(shape))
    t_dtype, h_dtype = hostio._device_dtype(np.result_type(before.dtype, after.dtype))
    lo, hi = bdist.shard_rows(n, rank, world)
    chunk = report_chunk_rows(config, 2 * elems * np.dtype(h_dtype).itemsize)
    want_diff = bool(getattr(config, "report_diff", False))

    raw = torch.empty((len(native.FRAME_ROWS), hi - lo), dtype=torch.float64, device=device)
    empty = torch.empty((0, elems), dtype=t_dtype, device=device)
    acc = native.pixel_moments_raw(empty, empty)               # the neutral elements (a rank may own no frames)
    diff = torch.empty((hi - lo, elems), dtype=t_dtype, device=device) if want_diff else None
    for a in range(lo, hi, chunk):
        e = min(a + chunk, hi)
        plan = hostio.RowPlan("range", n, lo=a, hi=e, count=e - a)
        b_dev = hostio.upload_rows(before, plan, device).to(t_dtype).reshape(e - a, elems)
        a_dev = hostio.upload_rows(after, plan, device).to(t_dtype).reshape(e - a, elems)      # (.to: a no-op unless the archives differ in dtype)
        raw[:, a - lo:e - lo] = native.frame_stats(b_dev, a_dev, diff[a - lo:e - lo] if want_diff else None)
        native.pixel_moments_raw(b_dev, a_dev, out=acc)
    rows = raw.t().contiguous()                                # (n_local, 10): frames are rows, as gather_rows wants them
    if world > 1:
        import torch.distributed as td
        rows = bdist.gather_rows(rows, n, dst=0)
        for idx, op in ((native.PIXEL_SUM_ROWS, td.ReduceOp.SUM), (native.PIXEL_MIN_ROWS, td.ReduceOp.MIN),
                        (native.PIXEL_MAX_ROWS, td.ReduceOp.MAX)):
            part = acc[list(idx)].contiguous()
            td.all_reduce(part, op=op)
            acc[list(idx)] = part
    diff_host = _gather_rows(diff, n, world) if want_diff else None
    if rank != 0:
        return None
    per_frame = native.frame_summary(rows.t(), elems, h_dtype)
    per_pixel = {k: v.reshape(shape) for k, v in native.pixel_summary(acc, n).items()}
    sums = rows.cpu().numpy()
    sumsq, before_sumsq = (float(np.cumsum(sums[:, k])[-1]) if n else 0.0 for k in (7, 8))      # in frame order
    with np.errstate(all="ignore"):
        totals = {"table_diff_rms": np.float64(np.sqrt(np.float64(sumsq) / np.float64(n * elems))),
                  "table_rel_l2": np.float64(np.sqrt(np.float64(sumsq) / np.float64(before_sumsq)))}
    result = {"shape": np.array((n,) + shape, dtype=np.int64)}
    result.update(per_frame)
    result.update(per_pixel)
    result.update(totals)
    if want_diff:
        result["diff"] = diff_host.reshape((n,) + shape)
    os.makedirs(os.path.join(output_path, "plotting"), exist_ok=True)
    np.savez(os.path.join(output_path, "plotting", "frame_stats.npz"), **result)
    print("=== Frame report ===")
    print(f"{n} frames of {' x '.join(str(d) for d in shape)}: difference RMS {totals['table_diff_rms']:.6g}, relative L2 error "
          f"{totals['table_rel_l2']:.6g}, {int(per_frame['nan_count'].sum())} NaN elements")
    with np.errstate(invalid="ignore"):
        worst = np.argsort(-np.nan_to_num(per_frame["diff_rms"], nan=np.inf), kind="stable")[:5]
    for k in worst:
        print(f"frame {int(k)}: difference RMS {per_frame['diff_rms'][k]:.6g} min {per_frame['diff_min'][k]:.6g} max "
              f"{per_frame['diff_max'][k]:.6g}; colour scale {per_frame['vmin'][k]:.6g} .. {per_frame['vmax'][k]:.6g}; PSNR "
              f"{per_frame['psnr'][k]:.4g} dB")
    return result
