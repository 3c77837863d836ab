// C ABI entry points of libbaler_amd.so (see include/baler_amd.h).  gfx950 only.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>

#include "bamd_internal.hpp"
#include "fused.hpp"
#include "bf16.hpp"

namespace bamd {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }

int DevBuf::ensure(size_t need) {
    if (need <= bytes) return BAMD_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    // round up so that slowly growing batches do not reallocate every call
    size_t want = (need + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
        set_error(std::string("hipMalloc(") + std::to_string(want) + "): " + hipGetErrorString(e));
        p = nullptr;
        return BAMD_ERR_ALLOC;
    }
    bytes = want;
    return BAMD_OK;
}

void DevBuf::release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
}

}  // namespace bamd

using namespace bamd;

namespace {
// The handle's buffers live on its device: make it current for the duration of a call and give the caller's current
// device back afterwards (a single process that drives several GPUs must not find its device changed under it).
struct DeviceGuard {
    int prev = -1, rc = hipSuccess;
    explicit DeviceGuard(int dev = -1) { if (dev >= 0) select(dev); }   // (a create call selects once the ordinal is known to exist)
    void select(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) rc = (int)hipSetDevice(dev); else prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
// ---- the kernel families: their precedence is written down HERE, once for inference and once for training, and every entry point
// below switches on one of the two routes (a new family is added there).  PjConv: pjconv.hip; Bf16: bf16.hip,
// bf16_train.hip; F16: the binary16 instantiations of bf16.hip (inference only: such a handle TRAINS on Fused, like an F32 handle); F16X3: f16x3.hip
// (inference only, like F16) -- these three infer through ONE state and one set of entry points (bf16.hpp), where the mode has named
// the kernels at setup; Fpga: fpga.hip; Fused: the fp32 register chain and wide-layer kernels of fused.hip; Fused64: the fp64 chain;
// Generic: layer by layer (generic.hip) -- any shape, and what a family that declines a call (BAMD_ERR_UNSUPPORTED) falls back to.
enum class Family { PjConv, Bf16, F16, F16X3, Fpga, Fused, Fused64, Generic };

// encode / decode / forward + loss: the handle alone decides
Family infer_family(const bamd_handle *h) {
    if (h->pj_state) return Family::PjConv;
    if (h->infer16_state) return h->mode == BAMD_MODE_BF16 ? Family::Bf16 : h->mode == BAMD_MODE_F16 ? Family::F16 : Family::F16X3;
    if (h->fpga_state) return Family::Fpga;
    if (h->fused_ok) return Family::Fused;
    if (h->mode == BAMD_MODE_F64 && h->fused64_state) return Family::Fused64;      // (also the wide fp64 class, which only infers)
    return Family::Generic;
}
// BF16 handles of the 24-column model train SMALL batches on the fp32 small-batch kernels: measured us per bamd_train_step,
// fp32 / bf16 kernels: 512 rows 23 / 34, 2048 rows 34 / 37, 8192 rows 72 / 51, 32768 rows 161 / 80 -- the bf16 pair needs ~3000
// rows to win (its workgroups own 64 rows each: a 512-row batch occupies 8 CUs).  BALER_AMD_BF16_SMALL_ROWS overrides (0: never).
int64_t bf16_small_rows() {
    const char *e = getenv("BALER_AMD_BF16_SMALL_ROWS");       // read per call: tests toggle it
    return e ? atoll(e) : 3072;
}
bool bf16_kernels_train(const bamd_handle *h, int64_t n_rows) {
    return h->mode == BAMD_MODE_BF16 && bf16_train_ok(h) && !(h->fused_ok && n_rows <= bf16_small_rows());
}
// fwd_bwd / train_step of a batch of n_rows > 0 rows: the handle and the batch size decide.  bamd_train_step and bamd_fwd_bwd read the
// SAME route, which is what keeps bamd_train_step == bamd_fwd_bwd + bamd_adam_step.
Family train_family(const bamd_handle *h, int64_t n_rows) {
    if (h->pj_state) return Family::PjConv;
    if (bf16_kernels_train(h, n_rows)) return Family::Bf16;
    if (fpga_trains(h, n_rows)) return Family::Fpga;
    if (h->fused_ok) return Family::Fused;
    if (h->mode == BAMD_MODE_F64 && fused64_trains(h)) return Family::Fused64;      // (the wide fp64 class trains layer by layer)
    return Family::Generic;
}

// (4 is not a mode: BAMD_MODE_F16X3 is 5, see include/baler_amd.h)
bool known_mode(int mode) {
    return mode == BAMD_MODE_F32 || mode == BAMD_MODE_F64 || mode == BAMD_MODE_BF16 || mode == BAMD_MODE_F16 || mode == BAMD_MODE_F16X3;
}
bool quiet() { const char *q = getenv("BALER_AMD_QUIET"); return q && q[0] == '1'; }      // BALER_AMD_QUIET=1: no notices on stderr
std::string dims_string(const bamd_handle *h) {      // "24-200-100-50-15-50-100-200-24"
    std::string d;
    for (size_t l = 0; l < h->dims.size(); ++l) d += (l ? "-" : "") + std::to_string(h->dims[l]);
    return d;
}
// The create calls: `device` exists, is current for the life of `guard`, and is a gfx950.  `fn`: the entry point the messages name.
int open_device(const char *fn, int device, DeviceGuard &guard) {
    int ndev = bamd_device_count();
    if (ndev <= 0) {
        if (ndev == 0) set_error("no HIP device visible");
        return BAMD_ERR_NO_DEVICE;
    }
    BAMD_REQUIRE_AS(fn, device >= 0 && device < ndev, "device ordinal out of range");
    guard.select(device);
    BAMD_REQUIRE_AS(fn, guard.rc == hipSuccess, "cannot select the device");
    hipDeviceProp_t prop;
    BAMD_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error(std::string("libbaler_amd is built for gfx950 only; device is ") + prop.gcnArchName);
        return BAMD_ERR_NO_DEVICE;
    }
    return BAMD_OK;
}
// bamd_encode / bamd_decode with 8-bit or packed sub-byte codes, or with 16-bit codes on a family that does not convert them in its kernels (latent_in_kernel below), chunk by
// chunk: body(r0, rows) finds room for `rows` float32 latent rows in h->lat32 (at most 256 MiB of them; BALER_AMD_LAT32_ROWS: several
// chunks at small sizes, for tests) and converts on its side of the family call.
template <typename Body>
int lat32_chunks(bamd_handle *h, int64_t n_rows, Body body) {
    const int64_t zd = h->dims[h->L / 2];
    int64_t chunk = env_ll("BALER_AMD_LAT32_ROWS", 0);
    if (chunk <= 0) chunk = std::max<int64_t>(1024, ((int64_t)256 << 20) / (zd * 4));
    for (int64_t r0 = 0; r0 < n_rows; r0 += chunk) {
        const int64_t rows = std::min(n_rows - r0, chunk);
        int rc = h->lat32.ensure((size_t)rows * zd * sizeof(float));
        if (!rc) rc = body(r0, rows);
        if (rc) return rc;
    }
    return BAMD_OK;
}
}  // namespace

// BAMD_F16 / BAMD_BF16 / BAMD_U8 / BAMD_U1 .. BAMD_U7 are storage types of latent codes: legal as z_dtype of bamd_encode / bamd_decode and nowhere else.
// Every other dtype argument is checked here, by name, before anything is launched or written.
#define BAMD_WIDE_DTYPE(d, name) \
    BAMD_REQUIRE(dtype_wide(d), name " must be BAMD_F32 or BAMD_F64 (BAMD_F16 / BAMD_BF16 / BAMD_U8 / BAMD_U1 .. BAMD_U7 are latent codes: z_dtype of bamd_encode / bamd_decode only)")

extern "C" {

int bamd_abi_version(void) { return BAMD_ABI_VERSION; }

const char *bamd_last_error(void) { return g_err.c_str(); }

int bamd_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        set_error(std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
        return BAMD_ERR_NO_DEVICE;
    }
    return n;
}

int bamd_create(const int *dims, int n_layers, int mode, int device, bamd_handle **out) {
    return bamd_create_act(dims, n_layers, BAMD_ACT_LEAKY_RELU, mode, device, out);
}

int bamd_create_act(const int *dims, int n_layers, int act, int mode, int device, bamd_handle **out) {
    BAMD_REQUIRE(dims && out, "null argument");
    BAMD_REQUIRE(n_layers >= 2 && n_layers % 2 == 0, "n_layers must be even and >= 2");
    BAMD_REQUIRE(act == BAMD_ACT_LEAKY_RELU || act == BAMD_ACT_RELU, "unknown activation");
    BAMD_REQUIRE(known_mode(mode), "unknown mode");
    for (int l = 0; l <= n_layers; ++l) BAMD_REQUIRE(dims[l] > 0, "layer widths must be positive");
    DeviceGuard guard;
    if (int rc = open_device(__func__, device, guard)) return rc;
    bamd_handle *h = new bamd_handle();
    h->L = n_layers;
    h->act = act;
    h->mode = mode;
    h->device = device;
    h->dims.assign(dims, dims + n_layers + 1);
    h->esize = mode == BAMD_MODE_F64 ? 8 : 4;
    int64_t off = 0;
    for (int l = 0; l < n_layers; ++l) {
        h->w_off.push_back(off);
        off += (int64_t)dims[l + 1] * dims[l];
        h->b_off.push_back(off);
        off += dims[l + 1];
        h->sum_dims += dims[l + 1];
    }
    h->nparams = off;
    for (int l = 0; l <= n_layers; ++l) h->max_dim = dims[l] > h->max_dim ? dims[l] : h->max_dim;
    // BAMD_MODE_BF16 of a shape without bf16 kernels (any AE / CFD_dense_AE(n_features, z_dim) the reference builds, models.py:122-139,
    // 192-209, other than the instantiated ones): the handle computes in float32 on whatever serves the shape there (run-time-width
    // classes, layer-wise kernels) and says so; bamd_mode_of() then reports BAMD_MODE_F32.  A slower path, not an error.
    bool demoted = false;
    if ((mode == BAMD_MODE_BF16 && !bf16_has_kernels(h) && !fused_has_bf16_kernels(h)) || (mode == BAMD_MODE_F16 && !bf16_has_kernels(h)) ||
        (mode == BAMD_MODE_F16X3 && !f16x3_has_kernels(h))) {
        h->mode = BAMD_MODE_F32;      // (BAMD_MODE_F16 / BAMD_MODE_F16X3 follow the same rule; they have no wide-model kernels)
        demoted = true;
    }
    int rc = h->params.ensure((size_t)(h->nparams + 1) * h->esize);
    if (rc) { delete h; return rc; }
    rc = fused_setup(h);      // every family that can serve the shape sets its state up; the two routes choose among them per call
    if (!rc) rc = fused64_setup(h);
    if (!rc) rc = fpga_setup(h);
    if (!rc && h->mode == BAMD_MODE_BF16 && !fused_serves_bf16_inference(h)) {   // (wide models in the bf16 mode are served by fused.hip)
        rc = infer16_setup(h);
        if (!rc) rc = bf16_train_setup(h);
    }
    if (!rc && (h->mode == BAMD_MODE_F16 || h->mode == BAMD_MODE_F16X3)) rc = infer16_setup(h);   // binary16 / hi | lo inference fragments beside the fused fp32 state it trains on
    if (rc) { bamd_destroy(h); return rc; }
    *out = h;
    const int path = bamd_path_of(h);
    if (demoted && !quiet())
        fprintf(stderr, "[baler_amd] model %s: %s only; this handle computes in float32 (%s)\n", dims_string(h).c_str(),
                mode == BAMD_MODE_F16 ? "BAMD_MODE_F16 has kernels for the 24-column AE with LeakyReLU"
                : mode == BAMD_MODE_F16X3 ? "BAMD_MODE_F16X3 has kernels for the 24-column AE with LeakyReLU"
                                      : "BAMD_MODE_BF16 has kernels for the 24-column AE and the 2500-25 / 625-7 / 512-6 wide models",
                path == BAMD_PATH_GENERIC ? "layer-wise kernels" : infer_family(h) == Family::Fpga ? "fused FPGA_prototype_model kernels" : "fused run-time-width kernels");
    if (path == BAMD_PATH_FUSED_INFER && infer_family(h) == Family::Fused64 && !quiet())
        fprintf(stderr, "[baler_amd] model %s (fp64) has fused encode / decode / validation kernels only: training runs layer by layer "
                        "(generic.hip, activations through HBM)\n", dims_string(h).c_str());
    else if ((path == BAMD_PATH_GENERIC || path == BAMD_PATH_FUSED_INFER) && !quiet()) {
        const std::string infer_only = "throughput training kernels (encode / decode / validation and training steps of up to " +
                                       std::to_string((long long)fused_latency_rows(h)) + " rows are fused)";
        fprintf(stderr, "[baler_amd] model %s (%s) has no fused %s: %s run layer by layer (generic.hip, activations through HBM)\n",
                dims_string(h).c_str(), h->mode == BAMD_MODE_F64 ? "fp64" : h->mode == BAMD_MODE_BF16 ? "bf16" : "fp32",
                path == BAMD_PATH_GENERIC ? "kernel instantiation" : infer_only.c_str(),
                path == BAMD_PATH_GENERIC ? "encode / decode / training" : "larger training batches");
    }
    return BAMD_OK;
}

int bamd_create_pjconv(int z_dim, int mode, int device, bamd_handle **out) {
    BAMD_REQUIRE(out, "null argument");
    BAMD_REQUIRE(z_dim >= 1 && z_dim <= 2450, "PJ_Conv_AE latent size must be in 1..2450 (encoder.5 = Linear(500, z), decoder.0 = Linear(z, 500))");
    BAMD_REQUIRE(known_mode(mode), "unknown mode");
    if (mode == BAMD_MODE_F64) {
        set_error("bamd_create_pjconv: PJ_Conv_AE computes in float32 only (the reference model's parameters and 2-D data are float32, "
                  "training.py:222-227, helper.py:556-558); BAMD_MODE_F64 is not supported");
        return BAMD_ERR_UNSUPPORTED;
    }
    DeviceGuard guard;
    if (int rc = open_device(__func__, device, guard)) return rc;
    bamd_handle *h = new bamd_handle();
    h->L = 2;                                  // rows of 784 values in and out, z_dim = dims[L / 2]
    h->dims = {784, z_dim, 784};
    h->mode = BAMD_MODE_F32;
    h->device = device;
    h->esize = 4;
    h->nparams = pj_param_count(z_dim);
    int rc = h->params.ensure((size_t)(h->nparams + 1) * h->esize);
    if (rc) { delete h; return rc; }
    rc = pj_setup(h, z_dim);
    if (rc) { bamd_destroy(h); return rc; }
    if (mode == BAMD_MODE_BF16 && !quiet())
        fprintf(stderr, "[baler_amd] model PJ_Conv_AE(z=%d): BAMD_MODE_BF16 has kernels for the 24-column AE and the 2500-25 / 625-7 / "
                        "512-6 wide models only; this handle computes in float32 (fused PJ_Conv_AE kernels)\n", z_dim);
    if (mode == BAMD_MODE_F16 && !quiet())
        fprintf(stderr, "[baler_amd] model PJ_Conv_AE(z=%d): BAMD_MODE_F16 has kernels for the 24-column AE with LeakyReLU only; this "
                        "handle computes in float32 (fused PJ_Conv_AE kernels)\n", z_dim);
    if (mode == BAMD_MODE_F16X3 && !quiet())
        fprintf(stderr, "[baler_amd] model PJ_Conv_AE(z=%d): BAMD_MODE_F16X3 has kernels for the 24-column AE with LeakyReLU only; this "
                        "handle computes in float32 (fused PJ_Conv_AE kernels)\n", z_dim);
    *out = h;
    return BAMD_OK;
}

int bamd_path_of(const bamd_handle *h) {
    BAMD_REQUIRE(h, "null handle");
    switch (infer_family(h)) {
    case Family::Bf16: return BAMD_PATH_BF16;
    case Family::F16: return BAMD_PATH_F16;
    case Family::F16X3: return BAMD_PATH_F16X3;
    case Family::Fused: return fused_trains(h) ? BAMD_PATH_FUSED : BAMD_PATH_FUSED_INFER;
    case Family::Fused64: return fused64_trains(h) ? BAMD_PATH_FUSED : BAMD_PATH_FUSED_INFER;
    case Family::Generic: return BAMD_PATH_GENERIC;
    default: return BAMD_PATH_FUSED;
    }
}

void bamd_destroy(bamd_handle *h) {
    if (!h) return;
    DeviceGuard guard(h->device);
    // every family: a handle may own several states (a BF16 handle: bf16, bf16-train and fused); no-ops without the state
    fused_teardown(h);
    fused64_teardown(h);
    fpga_teardown(h);
    pj_teardown(h);
    infer16_teardown(h);
    bf16_train_teardown(h);
    comm_teardown(h);
    h->params.release();
    h->packed.release();
    h->work.release();
    h->slabs.release();
    h->lossp.release();
    h->gscratch.release();
    h->lat32.release();
    delete h;
}

int64_t bamd_param_count(const bamd_handle *h) { return h ? h->nparams : 0; }
int bamd_mode_of(const bamd_handle *h) { return h ? h->mode : BAMD_ERR_INVALID; }
int bamd_act_of(const bamd_handle *h) { return h ? h->act : BAMD_ERR_INVALID; }

int bamd_load_params(bamd_handle *h, const void *params, int dtype, void *stream) {
    BAMD_REQUIRE(h && params, "null argument");
    BAMD_WIDE_DTYPE(dtype, "dtype");
    DeviceGuard guard(h->device);
    BAMD_REQUIRE(guard.rc == hipSuccess, "cannot select the handle's device");
    hipStream_t s = (hipStream_t)stream;
    int rc = launch_convert(params, dtype, h->params.p, h->param_dtype(), h->nparams, s);
    if (rc) return rc;
    h->params_loaded = true;
    switch (infer_family(h)) {
    case Family::PjConv: return BAMD_OK;             // the PJ_Conv_AE kernels read the flat copy itself
    case Family::Bf16:
    case Family::F16:
    case Family::F16X3:                              // several families: the 16-bit inference fragments, ...
        rc = infer16_pack(h, s);
        h->infer16_stale = false;
        if (h->mode == BAMD_MODE_BF16) {             // ... the bf16 training fragments, ...
            h->bf16_train_stale = false;
            if (!rc) rc = bf16_train_pack(h, s);
        }
        return rc ? rc : fused_pack(h, s);           // ... and the fp32 fragments the handle trains on (Bf16: its small batches; a no-op without them)
    default:
        // a handle may train on another family than it infers on, so this packs by compute type, not by route (no-ops without the state)
        return h->mode == BAMD_MODE_F64 ? fused64_pack(h, s) : fused_pack(h, s);
    }
}

int bamd_minmax(const void *x, int dtype, int64_t n_rows, int n_cols, double *features, void *stream) {
    BAMD_WIDE_DTYPE(dtype, "dtype");
    return launch_minmax(x, dtype, n_rows, n_cols, features, (hipStream_t)stream);
}

int bamd_col_minmax(const void *x, int dtype, int64_t n_rows, int n_cols, double *minmax, void *stream) {
    BAMD_WIDE_DTYPE(dtype, "dtype");
    return launch_minmax(x, dtype, n_rows, n_cols, minmax, (hipStream_t)stream, true);
}

int bamd_normalize(const void *x, int dtype, int64_t n_rows, int n_cols, const double *features, void *out,
                   int out_dtype, void *stream) {
    BAMD_WIDE_DTYPE(dtype, "dtype");
    BAMD_WIDE_DTYPE(out_dtype, "out_dtype");
    return launch_normalize(x, dtype, n_rows, n_cols, features, out, out_dtype, (hipStream_t)stream);
}

int bamd_renormalize(const void *x, int dtype, int64_t n_rows, int n_cols, const double *features,
                     const uint8_t *int_mask, double *out, void *stream) {
    BAMD_WIDE_DTYPE(dtype, "dtype");
    return launch_renormalize(x, dtype, n_rows, n_cols, features, int_mask, out, (hipStream_t)stream);
}

// Family::Bf16 re-rounds its fragments on demand: a training step refreshes only what the next step reads, inference lags (lazily);
// F16 / F16X3 have inference fragments only
static int bf16_train_sync(bamd_handle *h, hipStream_t s) { return std::exchange(h->bf16_train_stale, false) ? bf16_train_pack(h, s) : BAMD_OK; }
static int infer16_sync(bamd_handle *h, hipStream_t s) { return std::exchange(h->infer16_stale, false) ? infer16_pack(h, s) : BAMD_OK; }

// Every path that has just written h->params / h->packed (the Adam kernel, or Adam inside a weight-gradient launch) ends here: lazily
// refreshed float32 copies are stale, and a BF16 handle's bf16 fragments are re-rounded (on demand where the handle has both sets).
// Several families: whichever one trained the batch, the fused family's and the inference family's copies follow.
static int params_stepped(bamd_handle *h, hipStream_t s) {
    fused_params_changed(h);
    fused64_params_changed(h);
    if (infer_family(h) == Family::Bf16) {
        if (bf16_train_ok(h)) { h->infer16_stale = true; h->bf16_train_stale = true; }
        else return infer16_pack(h, s);
    }
    if (infer_family(h) == Family::F16 || infer_family(h) == Family::F16X3) h->infer16_stale = true;      // re-rounded / re-split by the next inference call
    return BAMD_OK;
}

#define BAMD_CHECK_MODEL(h)                                                        \
    BAMD_REQUIRE(h, "null handle");                                                \
    BAMD_REQUIRE((h)->params_loaded, "bamd_load_params() has not been called");    \
    DeviceGuard guard_((h)->device);                                               \
    BAMD_REQUIRE(guard_.rc == hipSuccess, "cannot select the handle's device");

// The family dispatch of bamd_encode (features: normalise on load), bamd_decode (renorm / int_mask: un-normalise on store) and
// bamd_forward_loss (`out`: the reconstruction, may be null).  The latent's dtype may be a 16-bit type only where latent_in_kernel() says
// the family's kernels round / widen the codes themselves.
static int infer_rows(bamd_handle *h, InferKind kind, const void *in, int in_dtype, int64_t n, const double *features, void *out,
                      int out_dtype, const double *renorm, const uint8_t *int_mask, double *loss_sum, hipStream_t s) {
    int rc = BAMD_ERR_UNSUPPORTED;      // what a family answers to a call it declines: the layer-wise kernels serve it
    switch (infer_family(h)) {
    case Family::PjConv:
        if (kind == K_ENCODE) return pj_encode(h, in, in_dtype, n, features, out, out_dtype, s);
        if (kind == K_DECODE) return pj_decode(h, in, in_dtype, n, renorm, int_mask, out, out_dtype, s);
        return pj_forward_loss(h, in, in_dtype, n, features, out, out_dtype, loss_sum, s);
    case Family::Bf16:
    case Family::F16:
    case Family::F16X3:    // the same entry points: the state's kernels are the mode's
        if ((rc = infer16_sync(h, s))) return rc;
        if (kind == K_ENCODE) return infer16_encode(h, in, in_dtype, n, features, out, out_dtype, s);
        if (kind == K_DECODE) return infer16_decode(h, in, in_dtype, n, renorm, int_mask, out, out_dtype, s);
        return infer16_forward_loss(h, in, in_dtype, n, features, out, out_dtype, loss_sum, s);
    case Family::Fpga:
        return fpga_infer(h, kind, in, in_dtype, n, features, out, out_dtype, renorm, int_mask, loss_sum, s);
    case Family::Fused:
        if (kind == K_ENCODE) return fused_encode(h, in, in_dtype, n, features, out, out_dtype, s);
        if (kind == K_DECODE) return fused_decode(h, in, in_dtype, n, renorm, int_mask, out, out_dtype, s);
        return fused_forward_loss(h, in, in_dtype, n, features, out, out_dtype, loss_sum, s);
    case Family::Fused64: rc = fused64_infer(h, kind, in, in_dtype, n, features, out, out_dtype, renorm, int_mask, loss_sum, s); break;
    case Family::Generic: break;
    }
    if (rc != BAMD_ERR_UNSUPPORTED) return rc;
    if (kind == K_FORWARD) return generic_forward_loss(h, in, in_dtype, n, features, out, out_dtype, loss_sum, s);
    const int mid = h->L / 2;
    return generic_forward(h, in, in_dtype, n, features, kind == K_ENCODE ? 0 : mid, kind == K_ENCODE ? mid : h->L, out, out_dtype, renorm,
                           int_mask, s);
}

// 16-bit latent codes (BAMD_F16 / BAMD_BF16).  The register-chain kernels of fused.hip, bf16.hip and the layer-wise path convert in
// the launch that touches the latent anyway (latent_io.hpp).  The wide-layer kernels, the fp64 chain, the FPGA_prototype_model
// kernels and the PJ_Conv_AE kernels keep their float32 / float64 stores: their latent goes through a float32 workspace and ONE row-conversion
// launch -- the same rounding (float32 first, then 16 bits) and the same exact widening, so the results are bit-identical either way.
// 8-bit codes (BAMD_U8) and packed sub-byte codes (BAMD_U1 .. BAMD_U7) take the workspace route on EVERY family: no encode / decode
// kernel knows them (latent_io.hpp), so the callers below ask this only for 16-bit codes.  Packed rows are byte-aligned
// (latent_row_bytes), so the workspace chunk that starts at row r0 starts at byte r0 * zrow like every other kind.
static bool latent_in_kernel(const bamd_handle *h) {
    const Family f = infer_family(h);      // (Fused: the register chain; the wide-layer kernels: workspace)
    return f == Family::Bf16 || f == Family::F16 || f == Family::F16X3 || f == Family::Generic || (f == Family::Fused && fused_latent_in_kernel(h));
}
int bamd_encode(bamd_handle *h, const void *x, int x_dtype, int64_t n_rows, const double *features, void *z,
                int z_dtype, void *stream) {
    BAMD_CHECK_MODEL(h);
    BAMD_WIDE_DTYPE(x_dtype, "x_dtype");
    BAMD_REQUIRE(dtype_wide(z_dtype) || dtype_half(z_dtype) || dtype_code8(z_dtype) || dtype_codeb(z_dtype),
                 "z_dtype must be BAMD_F32, BAMD_F64, BAMD_F16, BAMD_BF16, BAMD_U8 or BAMD_U1 .. BAMD_U7");
    BAMD_REQUIRE(n_rows >= 0 && ((x && z) || n_rows == 0), "bad arguments");
    if (n_rows == 0) return BAMD_OK;
    hipStream_t s = (hipStream_t)stream;
    if (dtype_wide(z_dtype) || (dtype_half(z_dtype) && latent_in_kernel(h)))
        return infer_rows(h, K_ENCODE, x, x_dtype, n_rows, features, z, z_dtype, nullptr, nullptr, nullptr, s);
    const int64_t zd = h->dims[h->L / 2];
    const size_t xrow = (size_t)h->dims[0] * dtype_bytes(x_dtype), zrow = latent_row_bytes(zd, z_dtype);
    return lat32_chunks(h, n_rows, [&](int64_t r0, int64_t rows) {
        const int rc = infer_rows(h, K_ENCODE, (const char *)x + (size_t)r0 * xrow, x_dtype, rows, features, h->lat32.p, BAMD_F32, nullptr,
                                  nullptr, nullptr, s);
        return rc ? rc : launch_convert_rows(h->lat32.p, BAMD_F32, (char *)z + (size_t)r0 * zrow, z_dtype, rows, (int)zd, s);
    });
}

int bamd_decode(bamd_handle *h, const void *z, int z_dtype, int64_t n_rows, const double *features,
                const uint8_t *int_mask, void *out, int out_dtype, void *stream) {
    BAMD_CHECK_MODEL(h);
    BAMD_REQUIRE(dtype_wide(z_dtype) || dtype_half(z_dtype) || dtype_code8(z_dtype) || dtype_codeb(z_dtype),
                 "z_dtype must be BAMD_F32, BAMD_F64, BAMD_F16, BAMD_BF16, BAMD_U8 or BAMD_U1 .. BAMD_U7");
    BAMD_WIDE_DTYPE(out_dtype, "out_dtype");
    BAMD_REQUIRE(n_rows >= 0 && ((z && out) || n_rows == 0), "bad arguments");
    if (n_rows == 0) return BAMD_OK;
    hipStream_t s = (hipStream_t)stream;
    if (dtype_wide(z_dtype) || (dtype_half(z_dtype) && latent_in_kernel(h)))
        return infer_rows(h, K_DECODE, z, z_dtype, n_rows, nullptr, out, out_dtype, features, int_mask, nullptr, s);
    const int64_t zd = h->dims[h->L / 2];
    const size_t zrow = latent_row_bytes(zd, z_dtype), orow = (size_t)h->dims[h->L] * dtype_bytes(out_dtype);
    return lat32_chunks(h, n_rows, [&](int64_t r0, int64_t rows) {
        const int rc = launch_convert_rows((const char *)z + (size_t)r0 * zrow, z_dtype, h->lat32.p, BAMD_F32, rows, (int)zd, s);
        return rc ? rc : infer_rows(h, K_DECODE, h->lat32.p, BAMD_F32, rows, nullptr, (char *)out + (size_t)r0 * orow, out_dtype, features,
                                    int_mask, nullptr, s);
    });
}

int bamd_forward_loss(bamd_handle *h, const void *x, int x_dtype, int64_t n_rows, const double *features,
                      void *recon, int recon_dtype, double *loss_sum, void *stream) {
    BAMD_CHECK_MODEL(h);
    BAMD_WIDE_DTYPE(x_dtype, "x_dtype");
    if (recon) BAMD_WIDE_DTYPE(recon_dtype, "recon_dtype");
    BAMD_REQUIRE(x && loss_sum && n_rows > 0, "bad arguments");
    return infer_rows(h, K_FORWARD, x, x_dtype, n_rows, features, recon, recon_dtype, nullptr, nullptr, loss_sum, (hipStream_t)stream);
}

// [grads | loss] of a batch on the family `fam` = train_family(h, n_rows) (checked arguments; n_rows may be 0)
static int fwd_bwd_rows(bamd_handle *h, Family fam, const void *x, int x_dtype, int64_t n_rows, const double *features, void *grads,
                        hipStream_t s) {
    if (n_rows == 0) {  // an empty shard of a global batch contributes a zero gradient and zero loss
        BAMD_HIP(hipMemsetAsync(grads, 0, (size_t)(h->nparams + 1) * h->esize, s));
        return BAMD_OK;
    }
    int rc = BAMD_ERR_UNSUPPORTED;      // what a family answers to a batch it declines: the layer-wise kernels serve it
    switch (fam) {
    case Family::PjConv: return pj_step(h, x, x_dtype, n_rows, features, grads, nullptr, nullptr, nullptr, nullptr, nullptr, s);
    case Family::Bf16:
        if ((rc = bf16_train_sync(h, s))) return rc;
        return bf16_fwd_bwd(h, x, x_dtype, n_rows, features, grads, s);
    case Family::Fpga: return fpga_step(h, x, x_dtype, n_rows, features, nullptr, grads, nullptr, nullptr, nullptr, nullptr, nullptr, s);
    case Family::Fused: return fused_fwd_bwd(h, x, x_dtype, n_rows, features, grads, s);
    case Family::Fused64:      // small batches: fp64 chain + weight-gradient tiles; otherwise the layer-wise kernels
        rc = fused64_step(h, x, x_dtype, n_rows, features, grads, nullptr, nullptr, nullptr, nullptr, nullptr, s);
        break;
    case Family::F16:      // inference families: train_family() never returns them
    case Family::F16X3:
    case Family::Generic: break;
    }
    if (rc != BAMD_ERR_UNSUPPORTED) return rc;
    return generic_fwd_bwd(h, x, x_dtype, n_rows, features, grads, s);
}

int bamd_fwd_bwd(bamd_handle *h, const void *x, int x_dtype, int64_t n_rows, const double *features,
                 void *grads, void *stream) {
    BAMD_CHECK_MODEL(h);
    BAMD_WIDE_DTYPE(x_dtype, "x_dtype");
    BAMD_REQUIRE(grads && n_rows >= 0 && (x || n_rows == 0), "bad arguments");
    return fwd_bwd_rows(h, train_family(h, n_rows), x, x_dtype, n_rows, features, grads, (hipStream_t)stream);
}

int bamd_fwd_bwd_latent(bamd_handle *h, const void *x, int x_dtype, int64_t n_rows, const double *features,
                        const void *latent_grad, void *grads, void *stream) {
    BAMD_CHECK_MODEL(h);
    BAMD_WIDE_DTYPE(x_dtype, "x_dtype");
    BAMD_REQUIRE(grads && x && n_rows > 0, "bad arguments");
    const Family fam = train_family(h, n_rows);
    if (fam == Family::PjConv) {
        set_error("bamd_fwd_bwd_latent: not implemented for PJ_Conv_AE (the sliced-Wasserstein loss is refused for convolutional models)");
        return BAMD_ERR_UNSUPPORTED;
    }
    if (!latent_grad) return fwd_bwd_rows(h, fam, x, x_dtype, n_rows, features, grads, (hipStream_t)stream);
    if (fam == Family::Fpga)
        return fpga_step(h, x, x_dtype, n_rows, features, latent_grad, grads, nullptr, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream);
    // the regulariser's gradient enters between the decoder's and the encoder's backward products: layer-wise path
    return generic_fwd_bwd(h, x, x_dtype, n_rows, features, grads, (hipStream_t)stream, latent_grad);
}

int bamd_swd(const void *z, const void *prior, const void *proj, int dtype, int64_t n_rows, int z_dim, int n_proj,
             double reg_weight, double *loss_out, void *dz_out, void *stream) {
    BAMD_WIDE_DTYPE(dtype, "dtype");
    return launch_swd(z, prior, proj, dtype, n_rows, z_dim, n_proj, reg_weight, loss_out, dz_out, (hipStream_t)stream);
}

int bamd_adam_step(bamd_handle *h, void *params, const void *grads, void *m, void *v, const bamd_adam *hp,
                   double *loss_accum, void *stream) {
    BAMD_CHECK_MODEL(h);
    BAMD_REQUIRE(params && grads && m && v && hp, "null argument");
    BAMD_REQUIRE(hp->step >= 1, "step must be >= 1");
    hipStream_t s = (hipStream_t)stream;
    // Several families: Adam also refreshes, in its one launch, the packed weight copy that the handle's training kernels read -- the fused
    // family's (also on a BF16 handle, for its small batches) or the fp64 chain's.  Both lists stay null for a handle without such a copy.
    const int *sc_off = nullptr, *sc_idx = nullptr;
    void *packed = nullptr;
    fused_scatter(h, &sc_off, &sc_idx, &packed);
    if (h->mode == BAMD_MODE_F64) fused64_scatter(h, &sc_off, &sc_idx, &packed);
    int rc = launch_adam(params, h->params.p, grads, m, v, h->nparams, h->esize, *hp, loss_accum, sc_off, sc_idx, packed, s);
    return rc == BAMD_OK ? params_stepped(h, s) : rc;
}

int bamd_train_step(bamd_handle *h, const void *x, int x_dtype, int64_t n_rows, const double *features, void *params,
                    void *grads, void *m, void *v, const bamd_adam *hp, double *loss_accum, void *stream) {
    BAMD_CHECK_MODEL(h);
    BAMD_WIDE_DTYPE(x_dtype, "x_dtype");
    BAMD_REQUIRE(params && m && v && hp && n_rows >= 0 && (x || n_rows == 0), "bad arguments");
    BAMD_REQUIRE(hp->step >= 1, "step must be >= 1");
    hipStream_t s = (hipStream_t)stream;
    const Family fam = train_family(h, n_rows);      // ONE route for every attempt below and for the fwd_bwd of the tail
    const bool one_call = !h->comm && n_rows > 0;    // data parallel: the gradients are summed over the ranks between fwd_bwd and Adam
    int rc = BAMD_ERR_UNSUPPORTED;      // a family without a step of its own, or one that declines this batch: fwd_bwd + Adam below
    if (one_call) {
        switch (fam) {
        case Family::PjConv:      // forward + loss + backward, the slab sums, then Adam over the flat vector
            return pj_step(h, x, x_dtype, n_rows, features, grads, params, m, v, hp, loss_accum, s);
        case Family::Fpga:        // forward + backward, then the slab sum with Adam: two launches
            return fpga_step(h, x, x_dtype, n_rows, features, nullptr, grads, params, m, v, hp, loss_accum, s);
        case Family::Fused:       // small batches: Adam (+ re-pack) in the weight-gradient launch
            rc = fused_train_step(h, x, x_dtype, n_rows, features, grads, params, m, v, *hp, loss_accum, s);
            if (rc == BAMD_OK && (h->mode == BAMD_MODE_BF16 || h->mode == BAMD_MODE_F16 || h->mode == BAMD_MODE_F16X3)) rc = params_stepped(h, s);
            break;
        case Family::Fused64: rc = fused64_step(h, x, x_dtype, n_rows, features, grads, params, m, v, hp, loss_accum, s); break;
        default: break;      // Bf16, Generic: no step of their own
        }
    }
    if (rc != BAMD_ERR_UNSUPPORTED) return rc;
    if (!grads) {
        rc = h->gscratch.ensure((size_t)(h->nparams + 1) * h->esize);
        if (rc) return rc;
        grads = h->gscratch.p;
    }
    // small batches on the layer-wise / wide launches: Adam inside the weight-gradient launch.  Only for models whose training runs on
    // generic.hip anyway (no fused state, or the wide launches): a fused narrow handle that declined above (BALER_AMD_LATENCY_ROWS below
    // the batch) keeps its throughput pair, as README says of that knob.
    if (one_call && (fam == Family::Generic || (fam == Family::Fused && fused_wide_train(h)))) {
        rc = generic_small_train_step(h, x, x_dtype, n_rows, features, grads, params, m, v, *hp, loss_accum, s);
        if (rc != BAMD_ERR_UNSUPPORTED) return rc == BAMD_OK ? params_stepped(h, s) : rc;
    }
    rc = fwd_bwd_rows(h, fam, x, x_dtype, n_rows, features, grads, s);
    // this rank's rows -> [grads | loss] summed over the ranks -> the replicated Adam step
    if (!rc && h->comm) rc = comm_allreduce_sum(h, grads, h->param_dtype(), h->nparams + 1, s);
    return rc ? rc : bamd_adam_step(h, params, grads, m, v, hp, loss_accum, stream);
}

// One epoch of bamd_train_step calls over consecutive rows of x.  batch_rows: the sizes of the n_batches batches (data parallel: this
// rank's share of every global batch, 0 allowed); null: batches of batch_size rows, the last one shorter.
static int train_batches(bamd_handle *h, const void *x, int x_dtype, const int64_t *batch_rows, int64_t n_batches, int64_t batch_size,
                         int64_t n_rows, const double *features, void *params, void *grads, void *m, void *v, const bamd_adam *hp,
                         double *loss_accum, void *stream) {
    const size_t row_bytes = (size_t)h->dims[0] * dtype_bytes(x_dtype);
    bamd_adam step_hp = *hp;
    int64_t r0 = 0;
    for (int64_t b = 0; b < n_batches; ++b) {
        const int64_t rows = batch_rows ? batch_rows[b] : std::min(batch_size, n_rows - r0);
        BAMD_REQUIRE_AS("bamd_train_epoch_dp", rows >= 0 && (x || rows == 0), "bad batch_rows entry");   // (only a batch_rows entry can fail it)
        step_hp.step = hp->step + b;
        const int rc = bamd_train_step(h, (const char *)x + (size_t)r0 * row_bytes, x_dtype, rows, features, params, grads, m, v, &step_hp,
                                       loss_accum, stream);
        if (rc) return rc;
        r0 += rows;
    }
    return BAMD_OK;
}

int bamd_train_epoch(bamd_handle *h, const void *x, int x_dtype, int64_t n_rows, int64_t batch_size, const double *features, void *params,
                     void *grads, void *m, void *v, const bamd_adam *hp, double *loss_accum, int64_t *steps_out, void *stream) {
    BAMD_REQUIRE(h && hp, "null argument");
    BAMD_REQUIRE(batch_size > 0 && n_rows >= 0 && (x || n_rows == 0), "bad arguments");
    BAMD_WIDE_DTYPE(x_dtype, "x_dtype");
    const int64_t steps = n_rows / batch_size + (n_rows % batch_size != 0);
    const int rc = train_batches(h, x, x_dtype, nullptr, steps, batch_size, n_rows, features, params, grads, m, v, hp, loss_accum, stream);
    if (!rc && steps_out) *steps_out = steps;
    return rc;
}

int bamd_train_epoch_dp(bamd_handle *h, const void *x, int x_dtype, const int64_t *batch_rows, int64_t n_batches, const double *features,
                        void *params, void *grads, void *m, void *v, const bamd_adam *hp, double *loss_accum, void *stream) {
    BAMD_REQUIRE(h && hp, "null argument");
    BAMD_REQUIRE(n_batches >= 0 && (batch_rows || n_batches == 0), "bad arguments");
    BAMD_WIDE_DTYPE(x_dtype, "x_dtype");
    return train_batches(h, x, x_dtype, batch_rows, n_batches, 0, 0, features, params, grads, m, v, hp, loss_accum, stream);
}

int bamd_emd_rows(const void *x, const void *recon, int dtype, int64_t n_rows, int n_cols, double *out,
                  void *stream) {
    BAMD_WIDE_DTYPE(dtype, "dtype");
    return launch_emd_rows(x, recon, dtype, n_rows, n_cols, out, (hipStream_t)stream);
}

int bamd_error_deltas(const void *x, const void *recon, int dtype, int64_t n_elems, double bound, uint8_t *flags,
                      uint16_t *deltas, void *stream) {
    BAMD_WIDE_DTYPE(dtype, "dtype");
    return launch_error_deltas(x, recon, dtype, n_elems, bound, flags, deltas, (hipStream_t)stream);
}

int bamd_apply_deltas(void *out, int dtype, int n_cols, const int64_t *rows, const int32_t *cols, const uint16_t *deltas,
                      int64_t count, void *stream) {
    BAMD_WIDE_DTYPE(dtype, "dtype");
    return launch_apply_deltas(out, dtype, n_cols, rows, cols, deltas, count, (hipStream_t)stream);
}

int bamd_activation_means(bamd_handle *h, const void *x, int x_dtype, int64_t n_rows, const double *features,
                          double *out, int max_nodes, void *stream) {
    BAMD_CHECK_MODEL(h);
    if (infer_family(h) == Family::PjConv) {
        set_error("bamd_activation_means: PJ_Conv_AE has no activation hooks (the reference model has none either, training.py:287)");
        return BAMD_ERR_UNSUPPORTED;
    }
    BAMD_WIDE_DTYPE(x_dtype, "x_dtype");
    BAMD_REQUIRE(x && out && n_rows > 0, "bad arguments");
    return generic_activation_means(h, x, x_dtype, n_rows, features, out, max_nodes, (hipStream_t)stream);
}

}  // extern "C"
