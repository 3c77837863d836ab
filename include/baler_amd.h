/*
 * baler_amd.h -- C ABI of libbaler_amd.so, the MI355X (gfx950) hot path of Baler's dense
 * autoencoder: train (forward + sum-of-squares loss + backward + Adam), encode (compress) and
 * decode (decompress), plus the per-column min-max (un)normalisation either side of it.
 *
 * The reference (baler-collaboration/baler @ 2024_10_08) has NO native/FFI boundary for this path:
 * the path sits behind Python call surfaces.  Each entry point below names
 * the reference interface it replaces (file:line, relative to the reference checkout); the Python
 * binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *  - every function returns 0 on success or a negative bamd_status; no exceptions cross the ABI;
 *    bamd_last_error() returns a message for the calling thread's last failure;
 *  - the CALLER owns every device buffer passed in (dataset, params, grads, Adam m/v, outputs);
 *    the library borrows the pointers for the duration of the call and owns only its handle
 *    (layer descriptor, MFMA-fragment-packed weight copy, partial-gradient slabs, activation
 *    workspace);
 *  - every pointer argument needs the alignment of its element type and nothing more (a row block of a larger allocation
 *    is a valid argument), and a call reads and writes nothing outside the rows, codes and parameters it was given;
 *  - all work is enqueued asynchronously on the hipStream_t passed as `stream` (void*; NULL =
 *    the default stream); nothing synchronises the host, with ONE exception: a call that has to make or grow device memory of the
 *    library's own -- the create calls (no stream: they allocate and fill their index maps with blocking copies), the first call
 *    that needs a workspace of the handle, the first handle-free call on a stream (scratch is per device and stream), and a call with
 *    more rows than any before it -- allocates, and freeing the smaller buffer waits for the device; a repeated call of a size already
 *    seen never waits (tests/test_gpu_streams.py holds stream order and the absence of a host wait for such calls);
 *  - one handle per (model, device); a handle is not thread-safe, and it is SINGLE-STREAM: the library re-packs its
 *    weight fragments lazily, on the stream of the first call that needs them after an optimiser step, so calls on one
 *    handle must be issued on one stream (or the caller orders its streams with events around every call);
 *  - parameter vectors are FLAT in Baler's state-dict order: for each layer l, W_l[out][in]
 *    row-major then b_l[out] (models.py:128-136; the key order of model.pt);
 *  - rows are independent: multi-GPU = one process and one handle per GPU, rows sharded by the
 *    caller; the only exchange is a SUM all-reduce of the flat gradient buffer between
 *    bamd_fwd_bwd() and bamd_adam_step() (done by the caller with RCCL).
 */
#ifndef BALER_AMD_H
#define BALER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BAMD_ABI_VERSION 1

typedef struct bamd_handle bamd_handle;

typedef enum bamd_status {
    BAMD_OK = 0,
    BAMD_ERR_INVALID = -1,     /* bad argument (null pointer, unsupported dtype/shape ...) */
    BAMD_ERR_NO_DEVICE = -2,   /* no HIP device / wrong architecture */
    BAMD_ERR_HIP = -3,         /* a HIP runtime call failed; see bamd_last_error() */
    BAMD_ERR_ALLOC = -4,       /* device allocation failed */
    BAMD_ERR_UNSUPPORTED = -5  /* feature not available in this compute mode */
} bamd_status;

/* element type of a caller buffer.  BAMD_F16 (IEEE binary16) and BAMD_BF16 (bfloat16) are STORAGE types of latent codes and are
 * legal in exactly two places: z_dtype of bamd_encode (the output) and z_dtype of bamd_decode (the input).  Every other dtype
 * argument of every function (x_dtype, out_dtype, recon_dtype, bamd_load_params, the normalisation / statistics / deltas / swd
 * entry points, bamd_allreduce_sum, the training calls) returns BAMD_ERR_INVALID for them, with a message that names the
 * argument, before anything is written to a caller buffer.
 * Rounding: a 16-bit code is the IEEE round-to-nearest-even conversion of the value the same handle would have stored as FLOAT32
 * (a BAMD_MODE_F64 handle rounds its float64 latent to float32 first, then to 16 bits: t.to(float32).to(float16 / bfloat16)).  NaN
 * stays NaN, +-inf stays +-inf, a float16 overflow gives +-inf (no saturation), float16 subnormals are produced, not flushed.
 * Widening a code on bamd_decode is exact: the result equals bamd_decode of the widened float32 codes bit for bit. */
typedef enum bamd_dtype { BAMD_F32 = 0, BAMD_F64 = 1, BAMD_F16 = 2, BAMD_BF16 = 3 } bamd_dtype;

/* 8-bit latent codes: a CODE KIND, not an element type -- no table can have it, so it is not a member of the enum above.
 * BAMD_U8 is legal in exactly two places: z_dtype of bamd_encode (the output) and z_dtype of bamd_decode (the input); the buffer
 * is (n_rows, z_dim) bytes, row-major, unpadded.  Every other dtype argument of every entry point returns BAMD_ERR_INVALID for
 * it, with a message that names the argument, before anything is launched or written.
 * Store: let v be the value the same handle would have stored as BAMD_F32 (a BAMD_MODE_F64 handle rounds its float64 latent to
 * float32 first).  The code is q = (uint8) min(max(rint(v), 0), 255), rint being round-half-to-even in float32 (rintf).  NaN
 * gives 0, -inf gives 0, +inf gives 255.
 * Load: float32(q) is exact; a decode of BAMD_U8 codes equals the decode of their float32 widening bit for bit, the fused
 * un-normalise and int-truncation epilogue included.
 * The library knows nothing about a scale: a caller that wants a latent in [0, 255] folds its per-column affine map into the
 * last encoder layer and the first decoder layer of the parameters it loads (baler_amd/latent8.py does).  For every family the
 * codes pass through the handle's float32 latent workspace and one row-conversion launch; no encode or decode kernel changes. */
typedef enum bamd_code8 { BAMD_U8 = 8 } bamd_code8;

/* Packed sub-byte latent codes, b = 1 .. 7 bits each: a third code kind, numbered 0x100 | b (BAMD_UB(b)); "code = bits" would
 * collide with values that stay refused.  Legal exactly where BAMD_U8 is -- z_dtype of the encode entry point (output) and of
 * the decode entry point (input); every other dtype argument of every entry point returns BAMD_ERR_INVALID for them, naming the
 * argument, before anything is launched or written.  0x100, 0x108 and 0x109 name nothing and are refused as well.
 * Store: v as for BAMD_U8; q = (unsigned) min(max(rint(v), 0), 2^b - 1), round-half-to-even in float32; NaN and -inf give 0,
 * +inf gives 2^b - 1 (for b = 8 this would be the BAMD_U8 rule).
 * Layout: the buffer is (n_rows, S) bytes, row-major, S = ceil(z_dim * b / 8).  Code k of a row occupies bits [k b, (k + 1) b)
 * of that row's bit string; bit i of a row is bit (i mod 8) of the row's byte (i div 8) -- least-significant bit first, the
 * order of numpy's packbits(bitorder="little").  The unused high bits of a row's last byte are written as zero and ignored on
 * load.  Rows are byte-aligned on purpose: row chunks, rank slices and row plans stay plain byte ranges (a chunk that starts at
 * row r starts at byte r * S); the cost is at most 7 bits per row.
 * Load: float32(q), exact; a decode of packed codes equals the decode of their float32 widening bit for bit, the fused
 * un-normalise and int-truncation epilogue included.  As for BAMD_U8 the library knows no scale, every family goes through the
 * float32 latent workspace and one row-conversion launch, and no encode or decode kernel changes. */
typedef enum bamd_codeb {
    BAMD_U1 = 0x101, BAMD_U2 = 0x102, BAMD_U3 = 0x103, BAMD_U4 = 0x104, BAMD_U5 = 0x105, BAMD_U6 = 0x106, BAMD_U7 = 0x107
} bamd_codeb;
#define BAMD_UB(bits) (0x100 | (bits))      /* bits = 1 .. 7 */

/* arithmetic the Linear layers run in.  F32 = v_mfma_f32_16x16x4_f32 (exact fp32, the parity mode:
 * outputs within 1e-5 rel. of the fp64 reference).  F64 = v_mfma_f64_16x16x4_f64 (long-horizon
 * training parity).  BF16 = v_mfma_f32_16x16x32_bf16 with fp32 accumulation: a THROUGHPUT mode with its own 2e-2 bar.
 * Inference (bamd_encode / bamd_decode / bamd_forward_loss): weights rounded from the fp32 master copy and kept in LDS,
 * 4-5x the F32 rate (measured 2e-3 encode, 6e-3 decode).  Training (bamd_fwd_bwd / bamd_train_step): bf16 weights,
 * activations and gradients through the chain, fp32 accumulation and fp32 partial gradients; params / m / v / grads stay
 * FLOAT (the caller's fp32 master copy and Adam state); bamd_adam_step re-rounds the bf16 fragments.  3.3x the F32 training
 * rate; one-step gradients within ~5e-3 rel-L2 of the fp64 reference; batches of <= 3072 rows run on the F32 small-batch
 * kernels instead (exact fp32, and faster there: 18 vs 34 us per 512-row step).  Available for the 24-column AE (every fused latent
 * size) and for the wide models CFD_dense_AE(2500, 25), CFD_dense_AE(625, 7) and the 512-column model: their two wide layers on
 * the bf16 MFMA in bamd_encode / bamd_decode (HBM-bound) and in the training pass (forward of en1 / de4, de4's input-gradient
 * product AND the weight gradients of those two wide layers: operands rounded to bfloat16, float32 accumulation and float32
 * partial sums; only the six narrow layers, the loss, the masks and the narrow layers' weight gradients stay fp32 on the
 * activations the pass stores -- dL/drecon as bfloat16 where both of its readers take it that way: one-step gradients within
 * ~1e-3 rel-L2, which is the rounding of those wide operands; BALER_AMD_BF16_WIDE_TRAIN=0: the F32 launches); validation of such a handle runs
 * in fp32; any OTHER shape asked for in BAMD_MODE_BF16 is created as a float32 handle (run-time-width fused classes or the layer-wise
 * kernels, whatever serves the shape in BAMD_MODE_F32) with a notice on stderr -- bamd_mode_of() then returns BAMD_MODE_F32.  bamd_activation_means of a BF16 handle runs on the fp32
 * layer-wise kernels.
 * BF16 arithmetic, of the 24-column AE and of the wide models (tests/bf16_ref.py is this paragraph as NumPy; the kernels are held
 * to it element by element, tests/test_gpu_bf16_contract.py).  Every rounding to bfloat16 is to nearest even; the order of an
 * fp32 sum is not part of the contract.
 *   Inference.  Weights: bfloat16, rounded from the fp32 master copy when they are packed.  Biases: fp32 -- the start value of
 *   the fp32 accumulator.  Rows: float64 (float32 rows widened; normalised as (x - min) / range in float64 when features are
 *   given) -> ONE rounding to float32 -> bfloat16.  Per layer a = b + sum_k W[., k] h[k] in fp32; an activated layer hands
 *   bfloat16(max(a, a * 0.01f)) on: LeakyReLU on the fp32 accumulator with the fp32 slope, then one rounding per layer input.
 *   The latent and the reconstruction stay fp32.  bamd_forward_loss is bamd_encode then bamd_decode: the fp32 latent is rounded
 *   to bfloat16 by the decoder's loader (as float / BAMD_F16 codes are; BAMD_BF16 codes enter exactly); its loss is the float64
 *   sum of (fp32 reconstruction - fp32 row)^2 / n_features.  Un-normalisation: float64(reconstruction) * range + min, two
 *   float64 roundings, trunc() on the int columns, then the output dtype.
 *   Training (batches above the small-batch threshold).  Weights AND biases: bfloat16 -- the bias is input column K of the
 *   packed weights and meets a ones column of the layer's input image, so it is one more bfloat16 x bfloat16 product of the
 *   fp32 sum (inference keeps it fp32: the two differ by the bias's rounding, 1e-3 to 2.5e-3 rel-L2 of an encode /
 *   decode).  Every layer input is
 *   a bfloat16 image, the latent included; the forward pass is otherwise the inference one.  e = fp32 reconstruction - fp32 row
 *   (not the row's bfloat16 image); loss = float64 sum of e^2 / n_features; dL/drecon = e * (2.0f / n_features) in fp32, rounded
 *   to bfloat16.  Backward: dX_l = dZ_l W_l with the forward's bfloat16 weights and fp32 sums; dZ_{l-1} = bfloat16(dX_l) where
 *   the STORED bfloat16 activation is >= 0 and bfloat16(dX_l * 0.01f) where its sign bit is set (the derivative is taken from
 *   the activation, not the pre-activation; no mask below the latent); [dW_l | db_l] = dZ_l^T [X_l | 1]: bfloat16 x bfloat16
 *   products, fp32 sums over the batch in a fixed order (bitwise repeatable).  Gradients and loss are stored as FLOAT.
 *   Wide models, bamd_encode / bamd_decode.  en1 and de4 follow the inference contract above (operands rounded to bfloat16, the
 *   fp32 bias as start value, LeakyReLU on the fp32 accumulator).  The six narrow layers follow it too in bamd_decode and in
 *   bamd_encode of FLOAT32 rows whose length is a multiple of 16 bytes and at least 192 columns (2500 and 512 columns; raw rows
 *   with features are normalised in float64 into a float32 workspace first and then take this path); in every other bamd_encode
 *   (FLOAT64 rows, 625 columns) the narrow layers run in exact fp32 on the fp32 master weights and their inputs are not
 *   rounded.  With features, bamd_decode un-normalises the float32 reconstruction with bamd_renormalize's arithmetic.
 *   bamd_forward_loss runs in fp32.
 *   Wide models, training (batches above BALER_AMD_WIDE_SMALL_ROWS, default 8192; smaller ones run the F32 launches).  Rows:
 *   float32 (FLOAT64 and raw rows: float64 -> one rounding to float32).  Forward: en1 and de4 round their input (the row; the
 *   fp32 activation y7) and their weights to bfloat16, fp32 bias as start value, fp32 sums; the SIX narrow layers -- which
 *   inference runs on the bf16 MFMA where the line above says so -- run in exact fp32 on the fp32 master weights; every
 *   activation is stored in fp32 and never rounded.  e = fp32 reconstruction - fp32 row; loss = float64 sum of e^2 /
 *   n_features; dL/drecon = e * (2.0f / n_features), and THIS is the one bfloat16 gradient: stored as bfloat16 when n_features
 *   is a multiple of 4 (BALER_AMD_BF16_DZ16=0: fp32) and rounded to bfloat16 by both of its readers either way.  Backward:
 *   de4's input-gradient product is bfloat16(dL/drecon) x bfloat16(W) with fp32 sums; the masks are y > 0 ? 1 : 0.01f on the
 *   stored fp32 activations; layers de3 .. en2 and every dZ below de4 are exact fp32.  Weight gradients: [dW | db] of de4 =
 *   bfloat16(dL/drecon)^T [bfloat16(y7) | 1] and of en1 = bfloat16(dZ)^T [bfloat16(row) | 1], fp32 sums in a fixed order --
 *   in passes of at least 128 rows; in a smaller pass these two products, like the narrow layers', are exact fp32 on the
 *   UNROUNDED fp32 dL/drecon, dZ, rows and y7.  The six narrow layers' gradients are exact fp32 from the fp32 dZ and
 *   activations always.  All biases are fp32 throughout.
 * F16 = v_mfma_f32_16x16x32_f16 with fp32 accumulation: the second THROUGHPUT mode, for INFERENCE only -- the MFMA rate and operand
 * layout of BF16 with IEEE binary16's 11 significant bits instead of 8 (measured against the fp64 reference: about one eighth of the
 * BF16 error).  It serves bamd_encode, bamd_decode and bamd_forward_loss of the 24-column AE at every fused latent size (15, 12, 10,
 * 8, 6, 5, 4, 3, 2).  Arithmetic: weights are rounded to nearest even from the fp32 master copy to binary16 when they are packed;
 * layer inputs are binary16 (rows, normalised in float64 first; latent codes on decode; activations); biases and accumulation are
 * fp32; after every activated layer the fp32 accumulator is rounded to binary16 (nearest even, NO clamp) and LeakyReLU is
 * max(h, h * s) in binary16, s = the binary16 nearest to 0.01; the two un-activated outputs (latent, reconstruction) stay fp32 and
 * go through the epilogues of the BF16 mode (un-normalise + int truncation, loss partials, every z_dtype).  On bamd_decode BAMD_F16
 * codes are binary16 already and enter the chain WITHOUT a rounding (BAMD_BF16 / float codes are rounded to binary16).
 * Range: data normalised to [0, 1] and the activations of a trained model (largest seen: 6.9) are far inside binary16's range
 * (65504).  A value that leaves it becomes +-inf, and every output of THAT ROW becomes non-finite (inf or NaN); no other row is
 * affected (rows are MFMA columns, they never mix).  Callers that cannot rule this out check their outputs, as
 * baler_amd's compress / decompress do, and fall back to BAMD_MODE_BF16 or BAMD_MODE_F32.
 * Everything else on an F16 handle is exact fp32: bamd_fwd_bwd, bamd_train_step, bamd_train_epoch(_dp) and bamd_adam_step run the
 * kernels a BAMD_MODE_F32 handle of the same shape runs, at every batch size, with bit-identical results (params / m / v / grads
 * are FLOAT); the binary16 fragments are re-rounded lazily after an optimiser step or bamd_load_params; bamd_activation_means runs
 * on the fp32 layer-wise kernels.  Any shape without F16 kernels (other column counts, the wide models, BAMD_ACT_RELU handles,
 * PJ_Conv_AE) is created as a float32 handle with one notice on stderr, and bamd_mode_of() returns BAMD_MODE_F32.
 * F16X3 = three v_mfma_f32_16x16x32_f16 products per tile with fp32 accumulation: a PARITY mode for INFERENCE -- the accuracy of F32
 * (the measurements are in DESIGN.md section 15) on the binary16 MFMA.  It serves
 * bamd_encode, bamd_decode and bamd_forward_loss of the 24-column AE at every fused latent size (15, 12, 10, 8, 6, 5, 4, 3, 2).
 * (Its value is 5: 4 is not a mode and stays refused as "unknown mode".)  Arithmetic:
 *   Split.  An fp32 value a becomes two binary16 values: hi = binary16(a), round to nearest even, NO clamp; lo = binary16((a - hi) *
 *   2^11).  a - hi is exact in fp32 and the scale is a power of two, so lo does not depend on the instructions that compute it.
 *   Weights are split from the fp32 master copy when they are packed.  Biases stay fp32.
 *   Layer.  main = b + sum hi_w * hi_h (the bias is the start value); corr = sum (lo_w * hi_h + hi_w * lo_h); both are fp32
 *   accumulators of the MFMA, whose summation order is unspecified; a = main + corr * 2^-11 in fp32, rounded once (corr * 2^-11 is
 *   exact).  The lo * lo product (2^-22 of the result) is not computed.
 *   Activated layers.  LeakyReLU is max(a, a * 0.01f) on the fp32 value; the value is split AFTER the activation (the order of the
 *   BF16 kernels, not of the F16 mode).
 *   Rows are normalised in float64 when features are given, rounded ONCE to float32, then split.  Latent codes on bamd_decode:
 *   float32 / float64 codes are rounded to float32, then split; BAMD_F16 and BAMD_BF16 codes widen exactly to float32 and are split
 *   like any float32 value -- a binary16 code (and a bfloat16 code inside binary16's normal range) has lo = 0 --, so decoding 16-bit
 *   codes and decoding their float32 widening give the same bits.  bamd_forward_loss is the encode, then the decode of the UNROUNDED
 *   fp32 latent.  The latent and the reconstruction stay fp32 and go through the epilogues of the BF16 mode (un-normalise + int
 *   truncation, loss partials, every z_dtype).  Results are bitwise repeatable.
 *   Range: binary16's.  A value whose hi part lies beyond 65504 (a row element, a latent code, an activation) becomes +-inf and
 *   every output of THAT ROW becomes non-finite; no other row changes.  A WEIGHT beyond 65504 does that to every row.  baler_amd's
 *   compress / decompress count such rows on the device and refuse before writing, as in the F16 mode.
 * Everything else on an F16X3 handle is exact fp32, as on an F16 handle: the training calls, bamd_adam_step and
 * bamd_activation_means run the launches of a BAMD_MODE_F32 handle bit for bit; the split fragments are re-made lazily after an
 * optimiser step or bamd_load_params.  Any shape without F16X3 kernels (other column counts, the wide models, BAMD_ACT_RELU handles,
 * PJ_Conv_AE) is created as a float32 handle with one notice on stderr, and bamd_mode_of() returns BAMD_MODE_F32. */
typedef enum bamd_mode { BAMD_MODE_F32 = 0, BAMD_MODE_F64 = 1, BAMD_MODE_BF16 = 2, BAMD_MODE_F16 = 3, BAMD_MODE_F16X3 = 5 } bamd_mode;

/* Adam hyper-parameters of one step (torch.optim.Adam defaults are beta1=.9 beta2=.999 eps=1e-8). */
typedef struct bamd_adam {
    int64_t step;   /* t AFTER the increment (first step = 1) */
    double lr;      /* current learning rate (host-side ReduceLROnPlateau feeds this) */
    double beta1, beta2, eps;
} bamd_adam;

int bamd_abi_version(void);
const char *bamd_last_error(void);
/* number of visible HIP devices, or a negative bamd_status */
int bamd_device_count(void);

/* ---- model handle ------------------------------------------------------------------------------
 * Replaces: models.AE.__init__ / models.CFD_dense_AE.__init__ (models.py:122-139, 192-209) and
 * data_processing.initialise_model/load_model (data_processing.py:76-110).
 * dims has n_layers+1 entries (n_features, 200, 100, 50, z, 50, 100, 200, n_features for the
 * reference topologies; any even n_layers >= 2 is accepted).  LeakyReLU(0.01) follows every layer
 * except the last encoder layer and the last decoder layer (models.py:141-152). */
int bamd_create(const int *dims, int n_layers, int mode, int device, bamd_handle **out);
void bamd_destroy(bamd_handle *h);

/* activation that follows every layer except the last encoder layer and the last decoder layer */
typedef enum bamd_act {
    BAMD_ACT_LEAKY_RELU = 0,   /* F.leaky_relu(0.01): AE / CFD_dense_AE (models.py:141-152) */
    BAMD_ACT_RELU = 1          /* nn.ReLU: FPGA_prototype_model (models.py:410-463) */
} bamd_act;
/* The create call above with the activation as an argument; the create call is exactly this one with BAMD_ACT_LEAKY_RELU.
 * Replaces: models.FPGA_prototype_model.__init__ (models.py:410-427) and data_processing.initialise_model / load_model
 * (data_processing.py:76-110) for that model, whose dims are (n_features, 20, 10, z, 10, 20, n_features) with ReLU after en1, en2,
 * de1 and de2.  ReLU follows torch: relu(nan) = nan, relu(-inf) = 0, and the backward pass lets the gradient through where the
 * layer's output is > 0 (threshold_backward; an exact-zero pre-activation gets a zero gradient).  A BAMD_ACT_RELU handle runs on the
 * fused FPGA_prototype_model kernels (fpga.hip) for n_features <= 64 and z <= 32 in BAMD_MODE_F32 / BAMD_MODE_F64, and on the
 * layer-wise kernels for every other shape; the LeakyReLU kernel families never serve it.  In BAMD_MODE_BF16 / BAMD_MODE_F16 / BAMD_MODE_F16X3 it is created as a
 * float32 handle with a notice on stderr.  The activation-means diagnostic returns BAMD_ERR_UNSUPPORTED for it (the reference model
 * has no activation hooks either, training.py:287). */
int bamd_create_act(const int *dims, int n_layers, int act, int mode, int device, bamd_handle **out);
int bamd_act_of(const bamd_handle *h);     /* the handle's bamd_act, or BAMD_ERR_INVALID for a null handle */

/* PJ_Conv_AE, the reference's convolutional autoencoder for 28 x 28 frames.  Replaces: models.PJ_Conv_AE.__init__ / encode / decode /
 * forward (models.py:668-715) and data_processing.initialise_model / load_model (data_processing.py:76-110) for that model:
 *   encoder.0 Conv2d(1, 20, 5, stride 2, pad 2) 28x28 -> 14x14, LeakyReLU(0.2); encoder.2 Conv2d(20, 50, 5, 2, 2) -> 7x7; flatten;
 *   encoder.4 Linear(2450, 500); encoder.5 Linear(500, z);  decoder.0 Linear(z, 500), LeakyReLU(0.2); decoder.2 Linear(500, 2450);
 *   decoder.4 ConvTranspose2d(50, 20, 5, 2, 2, output_padding 1) -> 14x14; decoder.5 ConvTranspose2d(20, 1, 5, 2, 2, 1) -> 28x28,
 *   LeakyReLU(0.2).
 * An image is ONE ROW of 784 values (NCHW (N, 1, 28, 28) is row-major (N, 784)), so every row-based call below takes rows of 784
 * values with the usual signature; features / renorm are per pixel, (2, 784) float64.  The flat parameter vector is the state-dict
 * order of the reference (per tensor weight row-major then bias; ConvTranspose2d weights are (in, out, kh, kw)): 2504541 + 1001 z
 * parameters.  The loss of bamd_forward_loss / bamd_fwd_bwd is utils.mse_sum_loss_l1(validate=True) (utils.py:176-211) of the
 * reference's 2-D path, whose divisor is true_data.shape[1] = the channel count, 1: the PLAIN sum of squared errors, not divided by 784.
 * Arithmetic: v_mfma_f32_16x16x4_f32 (exact fp32) implicit GEMMs, fixed-order weight-gradient sums: bitwise repeatable.
 * z_dim: 1 .. 2450 (else BAMD_ERR_INVALID).  mode: BAMD_MODE_F32; BAMD_MODE_BF16 / BAMD_MODE_F16 / BAMD_MODE_F16X3 give a float32 handle with a notice on stderr
 * (bamd_mode_of() reports BAMD_MODE_F32); BAMD_MODE_F64 returns BAMD_ERR_UNSUPPORTED.  Served on such a handle: bamd_encode,
 * bamd_decode (with the un-normalise / int-mask epilogue), bamd_forward_loss, bamd_fwd_bwd, bamd_adam_step, bamd_train_step,
 * bamd_train_epoch, bamd_train_epoch_dp (and the communicator calls), bamd_load_params, bamd_param_count, bamd_path_of
 * (BAMD_PATH_FUSED).  bamd_activation_means (the reference model has no hooks, training.py:287) and bamd_fwd_bwd_latent return
 * BAMD_ERR_UNSUPPORTED. */
int bamd_create_pjconv(int z_dim, int mode, int device, bamd_handle **out);

/* Which kernels serve this handle's throughput calls (bamd_encode / bamd_decode / bamd_fwd_bwd at large batches).  The fused
 * register-chained / wide-layer kernels are template instantiations.  EXACT instantiations for the shapes the reference ships configs
 * for: AE(24, z) for z in {15, 12, 10, 8, 6, 5, 4, 3, 2} (models.py:116-183 at the compression ratios of baler.py:117-123),
 * CFD_dense_AE(2500, 25), CFD_dense_AE(625, 7) (exafel1_config.py:14-15,33: 25 x 25 blocks) and the 512-column model; an F64 handle of
 * the 24-column AE has fused fp64 kernels for inference and for training steps of any size.  Every OTHER model with the reference's
 * hidden widths (200-100-50; models.py:122-139, 192-209 build them for any n_features / z_dim) is served by a CLASS instantiation with
 * run-time widths:
 *   - up to 63 columns, latent <= 31: every kernel (BAMD_PATH_FUSED);
 *   - 64 .. 127 columns, latent <= 31: a handle with TWO sets of packed weights -- the small-batch class for training steps up to the
 *     small-batch limit (default 12288 rows; BALER_AMD_LATENCY_ROWS at bamd_create; reference batch_size = 512) and the wide class
 *     below for encode / decode / forward + loss and larger training batches (BAMD_PATH_FUSED).  BALER_AMD_MID_HYBRID=0: the
 *     small-batch class alone, larger batches chunk after chunk on its kernels (BAMD_PATH_FUSED_INFER);
 *   - 48 .. 4096 columns, latent <= 63, that no class above takes: the wide-layer kernels with the column count and the latent as
 *     kernel arguments -- encode / decode / forward + loss fused, a training pass = two fused row-local launches + the layer-wise
 *     weight-gradient kernels, as for the exact wide shapes (BAMD_PATH_FUSED; BALER_AMD_WIDE_CLASS=0 switches the class off);
 *   - F64 handles: class instantiations of the fp64 kernels for up to 63 columns with a latent of up to 31 (every kernel), up to 127
 *     columns with a latent of up to 63 (inference, and training steps on the 4-row chain), and 128 .. 4096 columns with a latent of up
 *     to 63 for encode / decode / forward + loss only (fused64w.hip, the column count and the latent as kernel arguments): such a
 *     handle trains layer by layer and reports BAMD_PATH_FUSED_INFER; bamd_create says so once on stderr unless BALER_AMD_QUIET=1.
 *     BALER_AMD_F64_WIDE=0 at bamd_create puts it back on the layer-wise kernels (BAMD_PATH_GENERIC), BALER_AMD_F64_WIDE_WGS caps its grid;
 *   - BAMD_ACT_RELU handles of FPGA_prototype_model (n_features, 20, 10, z, 10, 20, n_features) for n_features <= 64 and z <= 32,
 *     BAMD_MODE_F32 and BAMD_MODE_F64: fused kernels with n_features and z as kernel arguments (fpga.hip; BAMD_PATH_FUSED;
 *     fp32 training batches above 8192 rows run on the layer-wise kernels, which are faster there).
 *     Every other BAMD_ACT_RELU handle runs on the layer-wise kernels.
 * Any other shape (other hidden widths, more than 4096 columns, a latent above 63) runs on the layer-wise kernels (activations
 * through HBM, 1.5-2.5x slower): bamd_create prints one line to stderr for such a handle unless BALER_AMD_QUIET=1.  There is no model
 * object in the reference to query (models.py builds nn.Linear layers of any width); this call exists so that callers and tests can tell. */
typedef enum bamd_path {
    BAMD_PATH_GENERIC = 0,   /* generic.hip: LDS-tiled MFMA GEMM per layer */
    BAMD_PATH_FUSED = 1,     /* fused.hip: register chain (24-column AE) or streamed wide layers + chain */
    BAMD_PATH_BF16 = 2,      /* bf16.hip / bf16_train.hip (24-column AE, BAMD_MODE_BF16); its small batches use the fused fp32 step */
    BAMD_PATH_FUSED_INFER = 3, /* 64..127 columns with BALER_AMD_MID_HYBRID=0 or BALER_AMD_WIDE_CLASS=0: fused.hip for encode / decode / forward + loss and
                              * the small-batch training kernels (larger batches chunk after chunk on the same kernels); an F64 handle of
                              * 128 .. 4096 columns: fused64w.hip for encode / decode / forward + loss, training layer by layer */
    BAMD_PATH_F16 = 4,       /* bf16.hip's binary16 instantiations for inference (24-column AE, BAMD_MODE_F16); training on the fused fp32 kernels */
    BAMD_PATH_F16X3 = 5      /* f16x3.hip: split-binary16 inference at fp32 accuracy (24-column AE, BAMD_MODE_F16X3); training on the fused fp32 kernels */
} bamd_path;
int bamd_path_of(const bamd_handle *h);   /* a bamd_path, or BAMD_ERR_INVALID for a null handle */
int64_t bamd_param_count(const bamd_handle *h);
int bamd_mode_of(const bamd_handle *h);    /* the mode the handle COMPUTES in (BAMD_MODE_BF16 / BAMD_MODE_F16 / BAMD_MODE_F16X3 asked of a shape without such kernels: BAMD_MODE_F32) */

/* (Re)build the handle's MFMA-fragment-packed weight copy from the caller's flat parameter vector
 * (device pointer; dtype F32 or F64).  Call after loading a checkpoint or changing params outside
 * bamd_adam_step().  Replaces: model.load_state_dict (data_processing.py:105-110). */
int bamd_load_params(bamd_handle *h, const void *params, int dtype, void *stream);

/* ---- normalisation -----------------------------------------------------------------------------
 * Replaces: data_processing.find_minmax (data_processing.py:113-130).  features = [min ; max-min],
 * (2, n_cols) float64, device memory. */
int bamd_minmax(const void *x, int dtype, int64_t n_rows, int n_cols, double *features,
                void *stream);
/* The same reduction as bamd_minmax() with the raw extrema as output: minmax = [min ; max], (2, n_cols) float64.
 * For row-sharded tables (one process per GPU): every rank reduces its own rows, the caller combines the ranks
 * with one MIN and one MAX all-reduce of n_cols doubles each and forms range = max - min once -- bit-identical to
 * data_processing.find_minmax (data_processing.py:113-130) over the whole table. */
int bamd_col_minmax(const void *x, int dtype, int64_t n_rows, int n_cols, double *minmax, void *stream);
/* Replaces: helper.normalize -> data_processing.normalize (helper.py:261-274,
 * data_processing.py:133-153): out = (x - min)/(max - min) per column, evaluated in float64 and
 * rounded to out_dtype. */
int bamd_normalize(const void *x, int dtype, int64_t n_rows, int n_cols, const double *features,
                   void *out, int out_dtype, void *stream);
/* Replaces: data_processing.renormalize_func (data_processing.py:188-203) + the per-column
 * astype cast at baler.py:426-435: out = x*range + min (float64), then truncation toward zero for
 * columns with int_mask[c] != 0 (int_mask may be NULL; it is a DEVICE pointer of n_cols bytes). */
int bamd_renormalize(const void *x, int dtype, int64_t n_rows, int n_cols, const double *features,
                     const uint8_t *int_mask, double *out, void *stream);

/* ---- inference ---------------------------------------------------------------------------------
 * Replaces: AE.encode (models.py:141-145) as driven by helper.compress's loop (helper.py:583-611).
 * x: (n_rows, n_features) row-major, x_dtype.  If features != NULL the rows are min-max normalised
 * on load with features = [min ; range] (device, float64) -- the fused form of helper.py:500-504.
 * z: (n_rows, z_dim) row-major, z_dtype: BAMD_F32 / BAMD_F64, or BAMD_F16 / BAMD_BF16 for 16-bit codes (2 bytes per element,
 * rounded as described at bamd_dtype; the conversion is part of the encode launch for the fp32 register-chain, bf16 and
 * layer-wise kernels, and one row-conversion launch behind a float32 workspace for the wide-layer kernels, the fp64 chain,
 * FPGA_prototype_model and PJ_Conv_AE), or BAMD_U8 for 8-bit codes (1 byte per element, see bamd_code8: float32 workspace and
 * one row-conversion launch for every family), or BAMD_U1 .. BAMD_U7 for packed sub-byte codes (z is then (n_rows, S) bytes,
 * S = ceil(z_dim * b / 8), see bamd_codeb; the same route).  x_dtype is BAMD_F32 or BAMD_F64. */
int bamd_encode(bamd_handle *h, const void *x, int x_dtype, int64_t n_rows, const double *features,
                void *z, int z_dtype, void *stream);
/* Replaces: AE.decode (models.py:147-152) as driven by helper.decompress (helper.py:700-723), with
 * the optional un-normalise + int-column truncation epilogue of baler.py:420-435 fused in when
 * features != NULL (int_mask may still be NULL).  z_dtype may be BAMD_F16 / BAMD_BF16: the codes are widened exactly on load and
 * the result is bit-identical to decoding the widened float32 codes; BAMD_U8 codes and packed BAMD_U1 .. BAMD_U7 rows likewise.  out_dtype is BAMD_F32 or BAMD_F64. */
int bamd_decode(bamd_handle *h, const void *z, int z_dtype, int64_t n_rows, const double *features,
                const uint8_t *int_mask, void *out, int out_dtype, void *stream);
/* Replaces: AE.forward (models.py:154-156) + utils.mse_sum_loss_l1(validate=True)
 * (utils.py:195-211) as used by training.validate (training.py:104-137).
 * recon may be NULL.  *loss_sum (device, float64) is OVERWRITTEN with sum((recon-x)^2)/n_features
 * of this batch. */
int bamd_forward_loss(bamd_handle *h, const void *x, int x_dtype, int64_t n_rows,
                      const double *features, void *recon, int recon_dtype, double *loss_sum,
                      void *stream);

/* ---- training ----------------------------------------------------------------------------------
 * Replaces: one iteration of training.fit's loop body up to loss.backward() (training.py:64-92):
 * zero_grad, forward, loss = sum((r-x)^2)/n_features, backward.
 * grads: device buffer of bamd_param_count()+1 elements of the handle's parameter type (float for
 * MODE_F32/BF16, double for MODE_F64); it is OVERWRITTEN with the gradient of this batch in
 * state-dict order, and element [param_count] receives the batch loss.  Summation order is fixed
 * (no float atomics): results are bitwise reproducible run to run.
 * Data-parallel use: each rank passes its slice of the global batch, then SUM-all-reduces the
 * whole buffer (the loss is a row sum, so the global-batch gradient is the sum of shard gradients). */
int bamd_fwd_bwd(bamd_handle *h, const void *x, int x_dtype, int64_t n_rows, const double *features,
                 void *grads, void *stream);
/* bamd_fwd_bwd() with an extra term dL/dz injected at the bottleneck: latent_grad is (n_rows, z_dim) of the
 * handle's parameter type and is ADDED to the gradient that reaches the encoder output.  Replaces:
 * loss.backward() of training.py:73-92 when config.custom_loss_function == "loss_function_swae" (the
 * loss then has a term that depends on z = model.encode(x) only).  grads[param_count] still receives the
 * reconstruction loss sum((r-x)^2)/n_cols alone.  Wide-layer models (CFD_dense_AE shapes with a fused path) run it on the fused
 * row-local launches, the latent term added at the bottleneck of the input-gradient chain; other shapes on the layer-wise kernels. */
int bamd_fwd_bwd_latent(bamd_handle *h, const void *x, int x_dtype, int64_t n_rows,
                        const double *features, const void *latent_grad, void *grads, void *stream);
/* Replaces: utils.compute_swd (utils.py:58-77) and its backward: for each of n_proj unit vectors
 * proj[s] (n_proj, z_dim) the projections of z and of prior (both (n_rows, z_dim)) are sorted across
 * the batch; *loss_out = reg_weight * mean_{s,k} (sort(z.P_s)_k - sort(prior.P_s)_k)^2 (float64), and
 * dz_out (n_rows, z_dim, `dtype`) = d loss / d z.  The random draws are the caller's (the reference
 * takes them from torch's global generator, utils.py:59,79-91).  2 <= n_rows <= 1048576 (up to 4096 rows one workgroup per
 * projection sorts in LDS; larger batches, e.g. CFD_project_animation's 6000, take passes through global memory).
 * The order of the sort is total, the one of a stable sort (numpy.argsort(kind="stable")): a NaN key sorts last, after +inf, and equal
 * keys -- identical latent rows, all NaNs -- are ordered by row, so each row of a tie group meets its own prior value and the result
 * is the same bits on every call.  Non-finite inputs propagate as IEEE arithmetic has them and never move a store: *loss_out is NaN
 * when a projection of z or of prior is NaN (a NaN anywhere in z, prior or proj), the rows of dz_out whose z holds a NaN are NaN,
 * and every other row is what the same arithmetic gives in float64 (a NaN in prior reaches the row at the top rank of each
 * projection; a NaN in proj[s] makes that projection, and with it all of dz_out, NaN).  +-inf in z sort as values: the loss is +inf
 * (NaN where +inf meets +inf of the prior at the same rank), that row of dz_out is non-finite, the others are finite. */
int bamd_swd(const void *z, const void *prior, const void *proj, int dtype, int64_t n_rows, int z_dim,
             int n_proj, double reg_weight, double *loss_out, void *dz_out, void *stream);
/* Replaces: torch.optim.Adam.step + zero_grad (training.py:68,95,266) on the flat buffers, and
 * refreshes the handle's packed weight copy.  params/m/v/grads: device, handle parameter type.
 * If loss_accum != NULL (device, float64): *loss_accum += grads[param_count]  (the running_loss of
 * training.py:97 without the per-step host sync). */
int bamd_adam_step(bamd_handle *h, void *params, const void *grads, void *m, void *v,
                   const bamd_adam *hp, double *loss_accum, void *stream);
/* Replaces: the whole body of the training.fit batch loop (training.py:64-97: zero_grad, forward,
 * loss, backward, optimizer.step, running_loss += loss) in ONE call; exactly bamd_fwd_bwd() followed
 * by bamd_adam_step() on the same arguments, for single-process training (no all-reduce between the
 * two).  Small batches (the reference's batch_size = 512 regime) run as two launches: the layer chain,
 * then one workgroup per weight-gradient tile that also applies Adam to the parameters it owns.
 * grads may be NULL (the gradient is then not materialised); otherwise as in bamd_fwd_bwd(). */
int bamd_train_step(bamd_handle *h, const void *x, int x_dtype, int64_t n_rows, const double *features,
                    void *params, void *grads, void *m, void *v, const bamd_adam *hp,
                    double *loss_accum, void *stream);

/* Replaces: ONE EPOCH of training.fit's batch loop (training.py:64-97) -- `for idx, inputs in enumerate(train_dl)`: sequential
 * batches of `batch_size` rows of the resident table, no shuffling, the partial last batch kept (training.py:237-263) -- in ONE
 * call: the loop runs inside the library, every batch exactly as bamd_train_step() (same kernels, same arguments, hp->step for the
 * first batch and +1 for every following one, one learning rate for the epoch as the reference's per-epoch scheduler gives it),
 * enqueued back to back on `stream` with no host synchronisation and no host round trip per step.  Bit-identical to the loop of
 * bamd_train_step() calls it replaces.  x: (n_rows, n_features) row-major, x_dtype.  *loss_accum += every batch's loss
 * (running_loss of training.py:97); grads (may be NULL) holds the LAST batch's gradient and loss afterwards (the "Training Loss"
 * training.py:100 prints).  *steps_out (host, may be NULL) receives the number of optimiser steps taken = ceil(n_rows / batch_size).
 * Single-process form (uniform batch size); the data-parallel epoch is bamd_train_epoch_dp() below. */
int bamd_train_epoch(bamd_handle *h, const void *x, int x_dtype, int64_t n_rows, int64_t batch_size, const double *features,
                     void *params, void *grads, void *m, void *v, const bamd_adam *hp, double *loss_accum, int64_t *steps_out,
                     void *stream);

/* ---- data-parallel training inside the library ("bmi_allreduce_init/... or pass ncclComm_t"; 8(e)) ----------
 * The reference is single-process; its batch loop (training.py:64-97) becomes data parallel by summing the [grads | loss] vector over
 * the ranks between loss.backward() (:92) and optimizer.step() (:93).  With a communicator attached to the handle, bamd_train_step()
 * and bamd_train_epoch_dp() run that sequence -- bamd_fwd_bwd on this rank's rows, ONE ncclAllReduce(ncclSum) of nparams + 1 elements
 * in place on `grads`, bamd_adam_step -- inside the library on the caller's stream: one host call per step / per epoch instead of three
 * Python -> C -> RCCL round trips per step.  RCCL is resolved at run time (dlopen of the librccl the process already has, else
 * librccl.so.1): the library has no link-time dependency on it, and handles without a communicator never touch it.
 *
 * bamd_comm_unique_id: rank 0 fills `id128` (128 bytes, ncclGetUniqueId) and hands it to the other ranks by any means (the Python
 *   host broadcasts it over its torch.distributed group).
 * bamd_comm_init: every rank, collectively: ncclCommInitRank(world, id, rank) on the handle's device; the handle owns the communicator
 *   (bamd_destroy / bamd_comm_release destroy it).  world = 1 is valid (RCCL on one GPU: the sum over one rank is the identity).
 * bamd_comm_attach: use an EXISTING ncclComm_t (`comm`, e.g. the caller's own) instead; the caller keeps ownership.
 * bamd_comm_release: detach (and destroy an owned communicator); the handle is single-process again.
 * bamd_allreduce_sum: the collective alone, in place on `buf` (count elements of dtype BAMD_F32 / BAMD_F64) -- for callers that keep
 *   the three-call sequence (e.g. the sliced-Wasserstein step) and for timing it. */
int bamd_comm_unique_id(void *id128);
int bamd_comm_init(bamd_handle *h, const void *id128, int rank, int world);
int bamd_comm_attach(bamd_handle *h, void *comm, int world);
int bamd_comm_release(bamd_handle *h);
int bamd_comm_world(const bamd_handle *h);      /* ranks of the attached communicator; 0 without one */
int bamd_allreduce_sum(bamd_handle *h, void *buf, int dtype, int64_t count, void *stream);
/* One epoch of the data-parallel batch loop in ONE call: `x` holds THIS rank's rows of every global batch back to back (the
 * block-cyclic shard of SURVEY 8(e)), batch_rows[i] (host array, n_batches entries, each >= 0: an empty slice contributes a zero
 * gradient) = this rank's rows of global batch i.  Every batch runs fwd_bwd -> all-reduce -> Adam as described above (hp->step for the
 * first, +1 per batch); without a communicator it is the single-process loop with explicit batch sizes (each batch exactly
 * bamd_train_step).  *loss_accum += every GLOBAL batch's loss; grads (may be NULL) holds the last batch's summed gradient and loss. */
int bamd_train_epoch_dp(bamd_handle *h, const void *x, int x_dtype, const int64_t *batch_rows, int64_t n_batches,
                        const double *features, void *params, void *grads, void *m, void *v, const bamd_adam *hp,
                        double *loss_accum, void *stream);

/* ---- diagnostics -------------------------------------------------------------------------------
 * Replaces: the EMD term of utils.mse_loss_emd_l1 (utils.py:112-119): sum over rows of the 1-D
 * Wasserstein distance between the row's column values of x and recon.  *out (device, float64)
 * is overwritten.  Forward-only metric; n_cols <= 4096 (more is refused with BAMD_ERR_INVALID).
 * Per row: mean_k |sort(x_row)_k - sort(recon_row)_k|; keys are compared in `dtype` and only ever moved, so the
 * sort is exact, and the differences are formed in float64.  A NaN anywhere in x or recon makes *out NaN.
 * +-inf sort as values: +inf at the same rank on both sides gives NaN (inf - inf), on one side only +inf.
 * Every sum has a fixed order that depends on the table's shape alone: the result is bitwise repeatable and
 * does not depend on how many workgroups ran (BALER_AMD_EMD_WGS, read per call, lowers the grid of the
 * 65 .. 4096-column kernel).  Up to 64 columns: one thread per row; above: rows sorted in LDS (emd.hip). */
int bamd_emd_rows(const void *x, const void *recon, int dtype, int64_t n_rows, int n_cols,
                  double *out, void *stream);
/* ---- error-bounded deltas side channel (config.save_error_bounded_deltas) -------------------------
 * Replaces: helper.save_error_bounded_requirement (helper.py:442-470) for a whole table at once.
 * x, recon: n_elems values of `dtype` (the normalised input and decode(encode(x)), row-major).
 * flags[i] = |(recon[i]-x[i])/x[i]*100| > bound with numpy's rules (+-inf -> 0, NaN never exceeds);
 * deltas[i] = IEEE binary16 bits of float16(recon[i]) - float16(x[i]) (np.subtract(dtype=float16)).
 * The caller compacts flags/deltas into the per-batch (row, col) lists of helper.py:589-606. */
int bamd_error_deltas(const void *x, const void *recon, int dtype, int64_t n_elems, double bound,
                      uint8_t *flags, uint16_t *deltas, void *stream);
/* Replaces: the delta loop of helper.decompress (helper.py:708-718): for i < count,
 * out[rows[i]][cols[i]] -= float16 deltas[i]; out is (n_rows, n_cols) of `dtype`, row-major, decoder
 * output BEFORE un-normalisation.  rows/cols/deltas are device arrays; (row, col) pairs are unique. */
int bamd_apply_deltas(void *out, int dtype, int n_cols, const int64_t *rows, const int32_t *cols,
                      const uint16_t *deltas, int64_t count, void *stream);
/* Replaces: activation extraction (models.py:160-183, diagnostics.py:10-47): mean over the batch of
 * leaky_relu(pre-activation) for every activated layer; out is (n_layers-2, max_nodes) float64
 * device memory, padded with NaN. */
int bamd_activation_means(bamd_handle *h, const void *x, int x_dtype, int64_t n_rows,
                          const double *features, double *out, int max_nodes, void *stream);
/* Replaces: the per-column statistics of plotting.plot_1D (plotting.py:118-123, 143-147, 203-234) -- residual = after - before,
 * response = (after - before) / before * 100, their mean and RMS, the residual's extrema and the value range -- for two row-major
 * tables before / after (n_rows, n_cols), both of `dtype`; n_cols 1 .. 128 (more: BAMD_ERR_UNSUPPORTED).  Handle-free.
 * Row cut (plotting.get_index_to_cut, plotting.py:60-73, 118-120): a row is left out of every statistic when
 * before[row][cut_col] < cut; a NaN there keeps the row, as numpy's comparison does; cut_col < 0: no cut.
 * The elementwise arithmetic is numpy's: the input dtype, one rounding per operation (fp32 division correctly rounded).
 * out: (13, n_cols) float64, device memory, one row per statistic over the kept rows of each column:
 *    0 count            1 sum(residual)   2 sum(residual^2)   3 min(residual)   4 max(residual)
 *    5 sum(response)    6 sum(response^2)
 *    7 min(before)      8 max(before)     9 min(after)       10 max(after)
 *   11 min(before + after)               12 max(before + after)      (plot_1D's histogram range, plotting.py:146-147)
 * Sums are float64 whatever the dtype, in a fixed order (no float atomics: bitwise repeatable), and propagate inf / NaN as IEEE
 * does (a zero in `before` gives +-inf or NaN, as in numpy); extrema skip NaN; a column without kept values has +inf / -inf.
 * accumulate != 0: `out` holds the result of earlier calls and this call's rows are added to it (sums and the count add, extrema
 * combine), so a table can be fed in row chunks.  n_rows = 0: BAMD_OK; `out` is set to the neutral elements, or left alone. */
int bamd_column_moments(const void *before, const void *after, int dtype, int64_t n_rows, int n_cols, int cut_col, double cut,
                        double *out, int accumulate, void *stream);
/* Replaces: the four np.histogram calls per column of plotting.plot_1D (plotting.py:150-170, 192-224): response, residual, before
 * and after, with the tables, the row cut and the arithmetic of bamd_column_moments.  Edge arrays are float64 device memory,
 * strictly increasing, 2 .. 1025 edges each: edges_resp[n_er] and edges_resid[n_ed] serve every column, edges_val is
 * (n_cols, n_ev) and serves `before` and `after` of its column; a NULL edge array skips that histogram.  counts_* are int64
 * device memory, (n_cols, edges - 1).  numpy's rule for explicit bins: bin k holds edges[k] <= v < edges[k+1], the last bin also
 * v == edges[-1]; NaN and values outside [edges[0], edges[-1]] are not counted; values are compared as float64.
 * accumulate != 0: the counts of this call's rows are added to counts_*; otherwise they are overwritten.  Integer sums: the
 * result does not depend on any order.  n_rows = 0: BAMD_OK (counts zeroed, or left alone).
 * n_ed < 0: per-column residual bins.  edges_resid is then (n_cols, -n_ed) float64, one strictly increasing edge array per
 * column, and counts_resid is (n_cols, -n_ed - 1); -n_ed is 2 .. 1025 (n_ed = -1 and n_ed < -1025: BAMD_ERR_INVALID).  The
 * edges need not be evenly spaced (the bin is found by bisection, values and edges compared as float64), the first edge may be
 * -inf and the last +inf.  The bin rule, the row cut, accumulate and n_rows = 0 are as above; n_er and n_ev keep their meaning,
 * and the other histograms of the same call give the counts that a call of their own gives.  (Exact order statistics of the
 * residual -- the box-and-whisker quartiles of plotting.plot_box_and_whisker -- are selected with it: baler_amd/colbox.py.) */
int bamd_column_hist(const void *before, const void *after, int dtype, int64_t n_rows, int n_cols, int cut_col, double cut,
                     const double *edges_resp, int n_er, int64_t *counts_resp, const double *edges_resid, int n_ed,
                     int64_t *counts_resid, const double *edges_val, int n_ev, int64_t *counts_before, int64_t *counts_after,
                     int accumulate, void *stream);

#ifdef __cplusplus
}
#endif

/* The report mode for 2-D data -- per-frame and per-pixel statistics of two tables of frames -- has a header of its own. */
#include "baler_amd_frames.h"

#endif /* BALER_AMD_H */
