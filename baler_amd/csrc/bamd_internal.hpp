// Internal declarations shared by the translation units of libbaler_amd.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/baler_amd.h"
#include "latent_io.hpp"

namespace bamd {

constexpr double kSlope = 0.01;  // F.leaky_relu default negative_slope (models.py:142-150); cast to T at use

void set_error(const std::string &msg);

#define BAMD_HIP(call)                                                                      \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            bamd::set_error(std::string(#call) + ": " + hipGetErrorString(e_));             \
            return BAMD_ERR_HIP;                                                            \
        }                                                                                   \
    } while (0)

// `fn`: the public entry point the message names (callers match on bamd_last_error()); a helper shared by several passes theirs on
#define BAMD_REQUIRE_AS(fn, cond, msg)                                                      \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            bamd::set_error(std::string(fn) + ": " + (msg));                                \
            return BAMD_ERR_INVALID;                                                        \
        }                                                                                   \
    } while (0)
#define BAMD_REQUIRE(cond, msg) BAMD_REQUIRE_AS(__func__, cond, msg)
// The fused latent sizes of the 24-column AE: every kernel family that instantiates AE(24, Z) does so for X(Z) of this list
// (fused.hip find_ops; bf16_net.hpp infer16_find)
#define BAMD_AE24_LATENTS(X) X(15) X(12) X(10) X(8) X(6) X(5) X(4) X(3) X(2)
// What an inference launch computes.  The kernel templates of fused.hip and fused64_infer.hpp take it as an int parameter with these values.
enum InferKind : int { K_ENCODE = 0, K_DECODE = 1, K_FORWARD = 2 };

// Tuning knobs are read on EVERY call (a getenv is nothing beside a launch; tests and A/B runs toggle them inside one process)
inline long long env_ll(const char *name, long long dflt) {
    const char *e = getenv(name);
    return e && e[0] ? atoll(e) : dflt;
}
inline bool env_off(const char *name) {      // "NAME=0" switches a default-on path off
    const char *e = getenv(name);
    return e && e[0] == '0';
}
// a run-time bool as a template argument: fn(std::true_type / std::false_type)
template <class Fn> inline void with_bool(bool b, Fn &&fn) {
    if (b) fn(std::true_type{});
    else fn(std::false_type{});
}

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need);  // grow-only; returns bamd_status
    void release();
};

}  // namespace bamd

struct bamd_handle {
    int L = 0;
    int mode = 0;
    int act = BAMD_ACT_LEAKY_RELU;  // bamd_act: the activation after every layer but the last encoder and the last decoder layer
    int device = 0;
    std::vector<int> dims;          // L+1
    std::vector<int64_t> w_off;     // offset of W_l in the flat vector
    std::vector<int64_t> b_off;     // offset of b_l
    int64_t nparams = 0;
    int sum_dims = 0;               // sum of dims[1..L]
    int max_dim = 0;
    size_t esize = 4;               // sizeof parameter/compute scalar (4 or 8)

    bamd::DevBuf params;            // flat copy of the parameters in the compute type
    bamd::DevBuf packed;            // MFMA-fragment-packed weights for the fused kernels
    bamd::DevBuf work;              // activation workspace (generic path)
    bamd::DevBuf slabs;             // per-workgroup partial gradients
    bamd::DevBuf lossp;             // partial loss sums (double)
    bamd::DevBuf gscratch;          // gradient buffer of bamd_train_step() when the caller passes none
    bamd::DevBuf lat32;             // float32 latent rows either side of the row conversion (16-bit codes on the families that do not fuse it)
    bool params_loaded = false;
    bool fused_ok = false;          // shape is served by the fused register-chained kernels
    void *fused_state = nullptr;    // index maps of the fused path (fused.hip)
    void *fused_small = nullptr;    // 64..127-column tables: second fused state (small-batch class kernels) beside the wide class in fused_state
    bamd::DevBuf packed_small;      // ... and its fragment-packed weights (fused.hip: SmallScope swaps both in for a small-batch call)
    void *fused64_state = nullptr;  // maps + packed fp64 weights of the fp64 small-batch step (fused64.hip)
    void *infer16_state = nullptr;  // Infer16State (bf16_net.hpp) of the bf16 / f16 / fp16x3 inference modes: maps + packed fragments; the mode decides whose
    void *bf16_train_state = nullptr;   // packed bf16 weights + maps of the bf16 training kernels (bf16_train.hip)
    bool infer16_stale = false;     // the fragments of infer16_state lag h->params (re-packed lazily by the next inference call)
    bool bf16_train_stale = false;  // the bf16 TRAINING fragments lag h->params (re-packed by the next bf16 training launch)
    void *comm = nullptr;           // ncclComm_t of data-parallel training (comm.hip); null: single process
    bool comm_owned = false;        // created by bamd_comm_init (destroyed with the handle) vs attached by the caller
    int comm_world = 0;
    void *fpga_state = nullptr;     // FPGA_prototype_model shapes with ReLU (fpga.hip)
    void *pj_state = nullptr;       // PJ_Conv_AE handles (pjconv.hip; bamd_create_pjconv)

    int param_dtype() const { return esize == 8 ? BAMD_F64 : BAMD_F32; }   // bamd_dtype of params, grads, m and v
    bool has_act(int l) const { return !(l == L / 2 - 1 || l == L - 1); }
    bool f32_compute() const { return mode == BAMD_MODE_F32 || mode == BAMD_MODE_F16 || mode == BAMD_MODE_F16X3; }   // F16 / F16X3 handles are F32 handles outside their inference kernels
    bool leaky() const { return act == BAMD_ACT_LEAKY_RELU; }   // the fused / fp64 / bf16 families implement LeakyReLU(0.01) only
};

namespace bamd {

// ---- elementwise.hip ----------------------------------------------------------------------------
DevBuf &scratch_for(int purpose, hipStream_t s);   // grow-only scratch of the handle-free kernels, per (purpose, device, stream)
int launch_minmax(const void *x, int dtype, int64_t n, int c, double *features, hipStream_t s, bool raw = false);
int launch_normalize(const void *x, int dtype, int64_t n, int c, const double *features, void *out,
                     int out_dtype, hipStream_t s);
int launch_renormalize(const void *x, int dtype, int64_t n, int c, const double *features,
                       const uint8_t *int_mask, double *out, hipStream_t s);
int launch_convert(const void *src, int src_dtype, void *dst, int dst_dtype, int64_t count,
                   hipStream_t s);
int launch_convert_rows(const void *src, int src_dtype, void *dst, int dst_dtype, int64_t rows, int z,
                        hipStream_t s);   // latent rows against the float32 workspace: packed codes (bamd_codeb) need the row shape
int launch_emd_rows(const void *x, const void *recon, int dtype, int64_t n, int c, double *out,
                    hipStream_t s);
int launch_emd_rows_wide(const void *x, const void *recon, int dtype, int64_t n, int c, double *out,
                         hipStream_t s);   // emd.hip: 65 <= c <= 4096
int launch_swd(const void *z, const void *prior, const void *proj, int dtype, int64_t n, int d, int ns, double reg_weight,
               double *loss_out, void *dz_out, hipStream_t s);
int launch_error_deltas(const void *x, const void *recon, int dtype, int64_t n, double bound, uint8_t *flags, void *deltas,
                        hipStream_t s);
int launch_apply_deltas(void *out, int dtype, int n_cols, const int64_t *rows, const int32_t *cols, const void *deltas,
                        int64_t count, hipStream_t s);
int launch_adam(void *params, void *params_copy, const void *grads, void *m, void *v, int64_t np,
                size_t esize, const bamd_adam &hp, double *loss_accum, const int *sc_off, const int *sc_idx,
                void *packed, hipStream_t s);

// ---- comm.hip (RCCL resolved at run time) -----------------------------------------------------------
int comm_allreduce_sum(bamd_handle *h, void *buf, int dtype, int64_t count, hipStream_t s);
void comm_teardown(bamd_handle *h);

// ---- generic.hip (layer-by-layer MFMA path, any dims) -------------------------------------------
int generic_forward(bamd_handle *h, const void *x, int x_dtype, int64_t n, const double *features,
                    int l0, int l1, void *out, int out_dtype, const double *renorm,
                    const uint8_t *int_mask, hipStream_t s);
int generic_forward_loss(bamd_handle *h, const void *x, int x_dtype, int64_t n,
                         const double *features, void *recon, int recon_dtype, double *loss_sum,
                         hipStream_t s);
int generic_fwd_bwd(bamd_handle *h, const void *x, int x_dtype, int64_t n, const double *features,
                    void *grads, hipStream_t s,
                    const void *latent_grad = nullptr);
int generic_small_train_step(bamd_handle *h, const void *x, int x_dtype, int64_t n, const double *features, void *grads, void *params,
                             void *m, void *v, const bamd_adam &hp, double *loss_accum, hipStream_t s);   // latent_grad: (n, z_dim) of the compute type, added to dL/dz
int generic_activation_means(bamd_handle *h, const void *x, int x_dtype, int64_t n,
                             const double *features, double *out, int max_nodes, hipStream_t s);

// ---- fpga.hip (FPGA_prototype_model [n, 20, 10, z, 10, 20, n] with ReLU, n <= 64, z <= 32; F32 / F64) ----------------------
bool fpga_matches(const bamd_handle *h);         // the shape and activation of the family (whatever the mode)
int fpga_setup(bamd_handle *h);                  // leaves h->fpga_state null for other shapes / modes or BALER_AMD_FORCE_GENERIC=1
void fpga_teardown(bamd_handle *h);
// K_DECODE: renorm / int_mask un-normalise into a float64 output; K_FORWARD: loss_sum, `out` (the reconstruction) may be null
int fpga_infer(bamd_handle *h, InferKind kind, const void *in, int in_dtype, int64_t n, const double *features, void *out, int out_dtype,
               const double *renorm, const uint8_t *int_mask, double *loss_sum, hipStream_t s);
bool fpga_trains(const bamd_handle *h, int64_t n_rows);   // this training batch runs on fpga.hip (else: the layer-wise kernels)
// fwd + loss + bwd (hp == nullptr), or the whole training step with Adam in the second launch; latent_grad may be null
int fpga_step(bamd_handle *h, const void *x, int x_dtype, int64_t n, const double *features, const void *latent_grad, void *grads,
              void *params, void *m, void *v, const bamd_adam *hp, double *loss_accum, hipStream_t s);

// ---- pjconv.hip (PJ_Conv_AE on 28 x 28 frames, rows of 784 values, latent 1..2450; float32) ------------------------------------
int pj_setup(bamd_handle *h, int z);
void pj_teardown(bamd_handle *h);
int64_t pj_param_count(int z);
int pj_encode(bamd_handle *h, const void *x, int x_dtype, int64_t n, const double *features, void *z, int z_dtype, hipStream_t s);
// renorm / int_mask: un-normalise into a float64 output
int pj_decode(bamd_handle *h, const void *z, int z_dtype, int64_t n, const double *renorm, const uint8_t *int_mask, void *out,
              int out_dtype, hipStream_t s);
int pj_forward_loss(bamd_handle *h, const void *x, int x_dtype, int64_t n, const double *features, void *recon, int recon_dtype,
                    double *loss_sum, hipStream_t s);
// fwd + loss + bwd into grads ([grads | loss]; null: the handle's scratch), then Adam when hp != nullptr
int pj_step(bamd_handle *h, const void *x, int x_dtype, int64_t n, const double *features, void *grads, void *params, void *m, void *v,
            const bamd_adam *hp, double *loss_accum, hipStream_t s);

// ---- one Adam step ----------------------------------------------------------------------------------------------------------
// The scalars every parameter of a step shares.  adam_scalars() holds the only bias-correction arithmetic of the library and
// adam_update() the only per-element update: adam_k (elementwise.hip) and the weight-gradient kernels that apply Adam to the
// parameters they own inline the same operations in the same order (-ffp-contract=off), so bamd_train_step ==
// bamd_fwd_bwd + bamd_adam_step to the last bit on every kernel family.
struct AdamScalars {
    double b1, b2, eps, step_size, bc2_sqrt;
};
inline AdamScalars adam_scalars(const bamd_adam &hp) {
    const double bc1 = 1.0 - pow(hp.beta1, (double)hp.step);
    const double bc2 = 1.0 - pow(hp.beta2, (double)hp.step);
    return {hp.beta1, hp.beta2, hp.eps, hp.lr / bc1, sqrt(bc2)};
}
// Where the state of one Adam step lives, and its scalars: what a weight-gradient kernel that applies Adam to the parameters it owns
// takes.  pcopy: the handle's own copy of the parameters; packed / sc_off / sc_idx: the fragment-packed copy and the CSR lists
// parameter -> packed positions it is refreshed through (null: none).
template <typename T> struct AdamTargets {
    T *params, *pcopy, *m, *v, *packed;
    const int *sc_off, *sc_idx;
    double *loss_accum;
    AdamScalars s;
};
template <typename T>
inline AdamTargets<T> adam_targets(const bamd_handle *h, void *params, void *m, void *v, void *packed, const void *sc_off, const void *sc_idx,
                                   double *loss_accum, const bamd_adam &hp) {
    return {(T *)params, (T *)h->params.p, (T *)m, (T *)v, (T *)packed, (const int *)sc_off, (const int *)sc_idx, loss_accum, adam_scalars(hp)};
}

#if defined(__HIPCC__)
// torch.optim.Adam single-tensor step (training.py:266; torch/optim/adam.py _single_tensor_adam) of one element.  The arithmetic
// runs in float64 and m, v and the returned parameter are rounded to the storage type once, so the fp32 mode differs from the
// fp64 reference by storage rounding only.
template <typename T>
__device__ __forceinline__ T adam_update(const AdamScalars &a, T g, T &m, T &v, T p) {
    const double gi = (double)g;
    double mi = (double)m, vi = (double)v;
    mi = mi + (gi - mi) * (1.0 - a.b1);            // exp_avg.lerp_(grad, 1 - beta1)
    vi = vi * a.b2 + (1.0 - a.b2) * gi * gi;       // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1-beta2)
    const double denom = sqrt(vi) / a.bc2_sqrt + a.eps;
    const double pi = (double)p - a.step_size * (mi / denom);
    m = (T)mi;
    v = (T)vi;
    return (T)pi;
}

// ---- fixed-order sums of ONE 256-thread workgroup (bitwise reproducible) ------------------------------------------------------
// One double per thread through a fixed tree in `sh` (256 doubles of LDS); every thread returns the sum.  A caller whose `sh`
// aliases LDS still being read puts its own barrier in front.
__device__ __forceinline__ double block_sum_tree(double v, double *sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
        __syncthreads();
    }
    return sh[0];
}
// Sum of n doubles in memory: 256 strided partial sums, then the tree.  (A single thread adding the partials one after the
// other -- what every loss reduction here did first -- is a chain of dependent L2 round trips: 6.5 us for 32 partials.)
__device__ __forceinline__ double block_sum_fixed(const double *__restrict__ part, int n, double *sh) {
    double s = 0.0;
    for (int k = threadIdx.x; k < n; k += 256) s += part[k];
    return block_sum_tree(s, sh);
}
// The finishing launch of a loss: one workgroup, *dst = (or +=) scale * sum of the partials.  (Internal linkage: every
// translation unit that launches it registers its own copy, like the kernels of its own file.)
namespace {
template <typename TO>
__global__ void __launch_bounds__(256) sum_partials_fixed_k(const double *__restrict__ part, int n, double scale, TO *dst, int accumulate) {
    __shared__ double sh[256];
    const double s = block_sum_fixed(part, n, sh) * scale;
    if (threadIdx.x == 0) *dst = accumulate ? (TO)((double)*dst + s) : (TO)s;
}
}  // namespace
#endif
}  // namespace bamd
