// FPGA_prototype_model (reference models.py:410-463): n -> 20 -> 10 -> z -> 10 -> 20 -> n, ReLU after en1, en2, de1 and de2,
// for 1 <= n <= 64 and 1 <= z <= 32 (n and z are kernel arguments, 20 and 10 compile-time).
//
// Layer-parallel: a workgroup of four waves shares a 64-row tile (lane = row); for every layer each wave takes one output unit (or,
// backward, one input feature) at a time for all 64 rows, so its weights are wave-uniform and stream through the scalar cache, and
// the tile's activations live in LDS in feature-major order (stride 65: row r of feature c at c * 65 + r, conflict-free).
// Workgroups are persistent over the tiles.
//
// Training: the forward activations of the tile stay in LDS; the backward pass walks the layers from de3 to en1, and once a layer's
// dL/d pre-activation is in LDS the workgroup reduces dW_l = dZ_l^T Y_{l-1} and db_l over the tile's 64 rows into registers (thread t
// owns the parameters t + 256 i) while it forms the previous layer's dL/d pre-activation.  Each workgroup writes one partial-gradient
// slab and one loss partial; a second launch sums the slabs in workgroup order (and optionally runs Adam: adam_update):
// no float atomics, results are bitwise repeatable, and a training step is two launches at any batch size.
#include <algorithm>
#include <cmath>

#include "bamd_internal.hpp"

namespace bamd {
namespace {

constexpr int H1 = 20, H2 = 10;          // hidden widths (models.py:414-424)
constexpr int kMaxF = 64, kMaxZ = 32;     // the family's scope
constexpr int RT = 64;                    // rows per tile = lanes per workgroup
constexpr int LD = RT + 1;                // LDS stride of one feature of a tile
constexpr size_t kLds = 160 * 1024;       // LDS of one CU (gfx950)

struct Layout {   // offsets of the flat state-dict vector
    int n, z;
    int w[6], b[6], N[6], K[6];
    int np;
};
__host__ __device__ inline Layout make_layout(int n, int z) {
    Layout o{};
    o.n = n; o.z = z;
    const int dims[7] = {n, H1, H2, z, H2, H1, n};
    int off = 0;
    for (int l = 0; l < 6; ++l) {
        o.K[l] = dims[l]; o.N[l] = dims[l + 1];
        o.w[l] = off; off += dims[l] * dims[l + 1];
        o.b[l] = off; off += dims[l + 1];
    }
    o.np = off;
    return o;
}

template <typename T> __device__ __forceinline__ T relu(T v) { return (v > (T)0 || v != v) ? v : (T)0; }   // relu(nan) = nan
template <typename T> __device__ __forceinline__ T relu_grad(T y, T g) { return y <= (T)0 ? (T)0 : g; }    // threshold_backward
__device__ __forceinline__ float fmadd(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double fmadd(double a, double b, double c) { return fma(a, b, c); }

__device__ __forceinline__ double load_any(const void *p, int f64, int64_t i) {
    return f64 ? ((const double *)p)[i] : (double)((const float *)p)[i];
}

// rows [r0, r0 + rows) of a (., w) row-major buffer -> tile[c * LD + r]; lanes past `rows` get zeros.  With `feat`: min-max
// normalised on load in float64 ((x - min) / range, as normalize_k), rounded to T.
template <typename T>
__device__ void load_tile(const void *src, int f64, int64_t r0, int rows, int w, const double *feat, T *tile) {
    for (int e = threadIdx.x; e < RT * w; e += blockDim.x) {
        const int r = e / w, c = e - r * w;
        T v = (T)0;
        if (r < rows) {
            const double x = load_any(src, f64, r0 * w + e);
            v = feat ? (T)((x - feat[c]) / feat[w + c]) : (T)x;
        }
        tile[c * LD + r] = v;
    }
}

// the reverse: tile -> rows of `dst` (dtype f64 / f32).  With `renorm`: x * range + min with two roundings and the int_mask
// truncation (renormalize_k), float64 output.
template <typename T>
__device__ void store_tile(void *dst, int f64, int64_t r0, int rows, int w, const double *renorm, const uint8_t *int_mask,
                           const T *tile) {
    for (int e = threadIdx.x; e < rows * w; e += blockDim.x) {
        const int r = e / w, c = e - r * w;
        const T v = tile[c * LD + r];
        if (renorm) {
            double o = __dadd_rn(__dmul_rn((double)v, renorm[w + c]), renorm[c]);
            if (int_mask && int_mask[c]) o = trunc(o);
            ((double *)dst)[r0 * w + e] = o;
        } else if (f64) {
            ((double *)dst)[r0 * w + e] = (double)v;
        } else {
            ((float *)dst)[r0 * w + e] = (float)v;
        }
    }
}

// ---- layer-parallel pieces: the NT threads of a workgroup (NW waves) share a 64-row tile; a wave owns one output unit (or one
// input feature) of a layer for all 64 rows (lane = row), so its weights are wave-uniform and come through the scalar cache ---------
constexpr int NT = 256, NW = NT / 64;
constexpr int kMaxP = (kMaxF * H1 + H1 + H1 * H2 + H2 + H2 * kMaxZ + kMaxZ + kMaxZ * H2 + H2 + H2 * H1 + H1 + H1 * kMaxF + kMaxF + NT - 1) / NT;

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// out[u][r] = act(b[u] + sum_k W[u][k] in[k][r]) for u < N (rows r = lanes)
template <typename T, int l>
__device__ __forceinline__ void fwd_layer(const T *__restrict__ P, const Layout &o, const T *in, T *out) {
    constexpr bool act = l != 2 && l != 5;
    const int lane = threadIdx.x & 63, N = o.N[l], K = o.K[l];
    for (int u0 = threadIdx.x >> 6; u0 < N; u0 += NW) {
        const int u = uniform(u0);
        const T *w = P + o.w[l] + u * K;
        T s = P[o.b[l] + u];
        for (int k = 0; k < K; ++k) s = fmadd(w[k], in[k * LD + lane], s);
        out[u * LD + lane] = act ? relu(s) : s;
    }
}

// dnext[k][r] = sum_u D[u][r] W_l[u][k] (+ add[r][k]), masked by the ReLU of layer l-1 when it has one (yin = its output)
template <typename T, int l>
__device__ __forceinline__ void dx_layer(const T *__restrict__ P, const Layout &o, const T *D, const T *yin, T *dnext, const T *add,
                                         int add_ld, bool valid) {
    constexpr bool mask = l - 1 != 2;
    const int lane = threadIdx.x & 63, N = o.N[l], K = o.K[l];
    for (int k0 = threadIdx.x >> 6; k0 < K; k0 += NW) {
        const int k = uniform(k0);
        const T *w = P + o.w[l] + k;
        T s = (T)0;
        for (int u = 0; u < N; ++u) s = fmadd(w[u * K], D[u * LD + lane], s);
        if (add && valid) s += add[(int64_t)lane * add_ld + k];
        dnext[k * LD + lane] = mask ? relu_grad(yin[k * LD + lane], s) : s;
    }
}

// acc (thread t owns the parameters t + i * NT) += [dW_l | db_l] = D^T [Y | 1] over the tile's 64 rows
template <typename T, int l>
__device__ __forceinline__ void dw_layer(const Layout &o, const T *D, const T *Y, T (&acc)[kMaxP]) {
    const int N = o.N[l], K = o.K[l];
#pragma unroll
    for (int i = 0; i < kMaxP; ++i) {
        const int q = (int)threadIdx.x + i * NT - o.w[l];
        if (q < 0 || q >= N * K + N) continue;
        T s[4] = {(T)0, (T)0, (T)0, (T)0};     // four interleaved partial sums over the rows (r mod 4), then a fixed tree
        if (q < N * K) {
            const int u = q / K, k = q - u * K;
#pragma unroll 1
            for (int r = 0; r < RT; r += 4)
#pragma unroll
                for (int v = 0; v < 4; ++v) s[v] = fmadd(D[u * LD + r + v], Y[k * LD + r + v], s[v]);
        } else {
            const int u = q - N * K;
#pragma unroll 1
            for (int r = 0; r < RT; r += 4)
#pragma unroll
                for (int v = 0; v < 4; ++v) s[v] += D[u * LD + r + v];
        }
        acc[i] += (s[0] + s[1]) + (s[2] + s[3]);
    }
}

// fixed-order sum of the NT threads' values (valid in thread 0)
__device__ __forceinline__ double block_sum_nt(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < NT; ++i) s += red[i];
    __syncthreads();
    return s;
}

// the activation tiles of one row tile in LDS: Y[l] = input of layer l (Y[0] = the normalised rows, Y[6] = the reconstruction)
template <typename T>
struct Tiles {
    T *y0, *y1, *y2, *y3, *y4, *y5, *y6;
    __device__ Tiles(int n, int z, T *base) {
        y0 = base; y1 = y0 + n * LD; y2 = y1 + H1 * LD; y3 = y2 + H2 * LD; y4 = y3 + z * LD; y5 = y4 + H2 * LD; y6 = y5 + H1 * LD;
    }
};

// kind (an InferKind) K_ENCODE: x -> z; K_DECODE: z -> out (optionally un-normalised); K_FORWARD: forward + loss (recon may be null)
template <typename T>
__global__ void __launch_bounds__(NT) fpga_infer_k(int kind, int n, int z, const void *in, int in_f64, int64_t n_rows,
                                                   const double *features, const T *__restrict__ P, void *out, int out_f64,
                                                   const double *renorm, const uint8_t *int_mask, double *loss_part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ double red[NT];
    const Layout o = make_layout(n, z);
    const Tiles<T> Y(n, z, (T *)lds_raw);
    const int lane = threadIdx.x & 63;
    const int64_t ntiles = (n_rows + RT - 1) / RT;
    double lsum = 0.0;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t r0 = tile * RT;
        const int rows = (int)std::min<int64_t>(RT, n_rows - r0);
        __syncthreads();
        if (kind == K_DECODE) {
            load_tile<T>(in, in_f64, r0, rows, z, nullptr, Y.y3);
        } else {
            load_tile<T>(in, in_f64, r0, rows, n, features, Y.y0);
            __syncthreads();
            fwd_layer<T, 0>(P, o, Y.y0, Y.y1);
            __syncthreads();
            fwd_layer<T, 1>(P, o, Y.y1, Y.y2);
            __syncthreads();
            fwd_layer<T, 2>(P, o, Y.y2, Y.y3);
        }
        if (kind != K_ENCODE) {
            __syncthreads();
            fwd_layer<T, 3>(P, o, Y.y3, Y.y4);
            __syncthreads();
            fwd_layer<T, 4>(P, o, Y.y4, Y.y5);
            __syncthreads();
            fwd_layer<T, 5>(P, o, Y.y5, Y.y6);
        }
        __syncthreads();
        if (kind == K_FORWARD && lane < rows)
            for (int k = threadIdx.x >> 6; k < n; k += NW) {
                const T d = Y.y6[k * LD + lane] - Y.y0[k * LD + lane];
                lsum += (double)d * (double)d;
            }
        if (out) store_tile<T>(out, out_f64, r0, rows, kind == K_ENCODE ? z : n, kind == K_DECODE ? renorm : nullptr, int_mask, kind == K_ENCODE ? Y.y3 : Y.y6);
    }
    if (kind == K_FORWARD) {
        const double s = block_sum_nt(lsum, red);
        if (threadIdx.x == 0) loss_part[blockIdx.x] = s;
    }
}

// fwd + loss + bwd of the rows of this workgroup's tiles -> one partial-gradient slab (np entries) + one loss partial
template <typename T>
__global__ void __launch_bounds__(NT) fpga_fwd_bwd_k(int n, int z, const void *x, int x_f64, int64_t n_rows, const double *features,
                                                     const T *__restrict__ P, const T *__restrict__ latent_grad, T *__restrict__ part,
                                                     int64_t part_stride, double *loss_part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ double red[NT];
    const Layout o = make_layout(n, z);
    const Tiles<T> Y(n, z, (T *)lds_raw);
    // dL/d pre-activation of the layer being reduced, two buffers: de3, de1, en3 in Da (widths n, 10, 10 -> max(n, 10)), de2, en3's
    // input gradient and en1 in Db (widths 20, z, 20)
    T *Da = Y.y6;
    T *Db = Da + std::max(n, H2) * LD;
    const int lane = threadIdx.x & 63;
    const double gscale = 2.0 / n;
    T acc[kMaxP];
#pragma unroll
    for (int i = 0; i < kMaxP; ++i) acc[i] = (T)0;
    const int64_t ntiles = (n_rows + RT - 1) / RT;
    double lsum = 0.0;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t r0 = tile * RT;
        const int rows = (int)std::min<int64_t>(RT, n_rows - r0);
        const bool valid = lane < rows;
        __syncthreads();
        load_tile<T>(x, x_f64, r0, rows, n, features, Y.y0);
        __syncthreads();
        fwd_layer<T, 0>(P, o, Y.y0, Y.y1);
        __syncthreads();
        fwd_layer<T, 1>(P, o, Y.y1, Y.y2);
        __syncthreads();
        fwd_layer<T, 2>(P, o, Y.y2, Y.y3);
        __syncthreads();
        fwd_layer<T, 3>(P, o, Y.y3, Y.y4);
        __syncthreads();
        fwd_layer<T, 4>(P, o, Y.y4, Y.y5);
        __syncthreads();
        // de3 + loss: Da[k][r] = 2 (recon - x) / n, zero for the lanes past the batch
        for (int k0 = threadIdx.x >> 6; k0 < n; k0 += NW) {
            const int k = uniform(k0);
            const T *w = P + o.w[5] + k * H1;
            T s = P[o.b[5] + k];
            for (int j = 0; j < H1; ++j) s = fmadd(w[j], Y.y5[j * LD + lane], s);
            T d = (T)0;
            if (valid) {
                const T e = s - Y.y0[k * LD + lane];
                lsum += (double)e * (double)e;
                d = (T)(gscale * (double)e);
            }
            Da[k * LD + lane] = d;
        }
        // walk back: reduce layer l's weight gradient and form layer l-1's dL/d pre-activation from the same buffer
        const T *lg = latent_grad ? latent_grad + r0 * z : nullptr;
        __syncthreads();
        dw_layer<T, 5>(o, Da, Y.y5, acc);
        dx_layer<T, 5>(P, o, Da, Y.y5, Db, nullptr, 0, valid);
        __syncthreads();
        dw_layer<T, 4>(o, Db, Y.y4, acc);
        dx_layer<T, 4>(P, o, Db, Y.y4, Da, nullptr, 0, valid);
        __syncthreads();
        dw_layer<T, 3>(o, Da, Y.y3, acc);
        dx_layer<T, 3>(P, o, Da, Y.y3, Db, lg, z, valid);
        __syncthreads();
        dw_layer<T, 2>(o, Db, Y.y2, acc);
        dx_layer<T, 2>(P, o, Db, Y.y2, Da, nullptr, 0, valid);
        __syncthreads();
        dw_layer<T, 1>(o, Da, Y.y1, acc);
        dx_layer<T, 1>(P, o, Da, Y.y1, Db, nullptr, 0, valid);
        __syncthreads();
        dw_layer<T, 0>(o, Db, Y.y0, acc);
    }
#pragma unroll
    for (int i = 0; i < kMaxP; ++i) {
        const int p = (int)threadIdx.x + i * NT;
        if (p < o.np) part[(int64_t)blockIdx.x * part_stride + p] = acc[i];
    }
    const double s = block_sum_nt(lsum, red);
    if (threadIdx.x == 0) loss_part[blockIdx.x] = s;
}

struct FpgaAdam {
    int on;
    AdamScalars s;
};

// slabs -> gradient (workgroup order), loss; with Adam on: the optimiser step on the summed gradient
template <typename T>
__global__ void __launch_bounds__(256) fpga_reduce_k(const T *__restrict__ part, int nblk, int64_t part_stride, int np,
                                                     const double *__restrict__ loss_part, double loss_scale, T *grads,
                                                     FpgaAdam ad, T *params, T *pcopy, T *m, T *v, double *loss_accum) {
    __shared__ double sh[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0) {
        const double ls = block_sum_fixed(loss_part, nblk, sh);
        if (threadIdx.x == 0) {
            const T loss = (T)(ls * loss_scale);
            if (grads) grads[np] = loss;
            if (ad.on && loss_accum) *loss_accum += (double)loss;
        }
    }
    if (i >= np) return;
    T g = (T)0;
    for (int b = 0; b < nblk; ++b) g += part[(int64_t)b * part_stride + i];
    if (grads) grads[i] = g;
    if (!ad.on) return;
    T mi = m[i], vi = v[i];
    const T pi = adam_update(ad.s, g, mi, vi, params[i]);
    m[i] = mi;
    v[i] = vi;
    params[i] = pi;
    pcopy[i] = pi;
}

struct FpgaState {
    int n = 0, z = 0;
    int cus = 0;
    DevBuf part;      // per-workgroup partial gradients
    DevBuf lossp;     // per-workgroup loss partials
};

FpgaState *fst(const bamd_handle *h) { return (FpgaState *)h->fpga_state; }

// LDS of a workgroup: the tiles Y[0..6] (inference) or Y[0..5] + the two gradient buffers (training)
size_t infer_lds(const Layout &o, int esize) {
    return (size_t)esize * (size_t)(o.n + H1 + H2 + o.z + H2 + H1 + o.n) * LD;
}
size_t train_lds(const Layout &o, int esize) {
    return (size_t)esize * (size_t)(o.n + H1 + H2 + o.z + H2 + H1 + std::max(o.n, H2) + std::max(H1, o.z)) * LD;
}
// persistent grid: enough workgroups to fill every CU at the occupancy the LDS allows, never more than the tiles
int grid_for(const FpgaState *st, int64_t n_rows, size_t lds) {
    const int64_t ntiles = (n_rows + RT - 1) / RT;
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(2048 / NT, kLds / (lds + NT * sizeof(double))));
    return (int)std::min<int64_t>(ntiles, (int64_t)st->cus * per_cu);
}

template <typename T>
int infer_T(bamd_handle *h, InferKind kind, const void *in, int in_dtype, int64_t n_rows, const double *features, void *out, int out_dtype,
            const double *renorm, const uint8_t *int_mask, double *loss_sum, hipStream_t s) {
    FpgaState *st = fst(h);
    const Layout o = make_layout(st->n, st->z);
    const size_t lds = infer_lds(o, sizeof(T));
    const int grid = grid_for(st, n_rows, lds);
    if (kind == K_FORWARD) {
        if (int rc = st->lossp.ensure(sizeof(double) * grid)) return rc;
    }
    BAMD_HIP(hipFuncSetAttribute((const void *)fpga_infer_k<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(fpga_infer_k<T>, dim3(grid), dim3(NT), lds, s, kind, st->n, st->z, in, in_dtype == BAMD_F64 ? 1 : 0, n_rows,
                       features, (const T *)h->params.p, out, out_dtype == BAMD_F64 ? 1 : 0, renorm, int_mask,
                       (double *)st->lossp.p);
    BAMD_HIP(hipGetLastError());
    if (kind == K_FORWARD) {
        hipLaunchKernelGGL(sum_partials_fixed_k<double>, dim3(1), dim3(256), 0, s, (const double *)st->lossp.p, grid, 1.0 / st->n,
                           loss_sum, 0);
        BAMD_HIP(hipGetLastError());
    }
    return BAMD_OK;
}

template <typename T>
int step_T(bamd_handle *h, const void *x, int x_dtype, int64_t n_rows, const double *features, const void *latent_grad, void *grads,
           void *params, void *m, void *v, const bamd_adam *hp, double *loss_accum, hipStream_t s) {
    FpgaState *st = fst(h);
    const Layout o = make_layout(st->n, st->z);
    const size_t lds = train_lds(o, sizeof(T));
    const int grid = grid_for(st, n_rows, lds);
    const int64_t stride = (o.np + 63) & ~63;
    if (int rc = st->part.ensure(sizeof(T) * (size_t)stride * grid)) return rc;
    if (int rc = st->lossp.ensure(sizeof(double) * grid)) return rc;
    BAMD_HIP(hipFuncSetAttribute((const void *)fpga_fwd_bwd_k<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(fpga_fwd_bwd_k<T>, dim3(grid), dim3(NT), lds, s, st->n, st->z, x, x_dtype == BAMD_F64 ? 1 : 0, n_rows, features,
                       (const T *)h->params.p, (const T *)latent_grad, (T *)st->part.p, stride, (double *)st->lossp.p);
    BAMD_HIP(hipGetLastError());
    FpgaAdam ad{};
    if (hp) {
        ad.on = 1;
        ad.s = adam_scalars(*hp);
    }
    hipLaunchKernelGGL(fpga_reduce_k<T>, dim3((o.np + 255) / 256), dim3(256), 0, s, (const T *)st->part.p, grid, stride, o.np,
                       (const double *)st->lossp.p, 1.0 / st->n, (T *)grads, ad, (T *)params, (T *)h->params.p, (T *)m, (T *)v,
                       loss_accum);
    BAMD_HIP(hipGetLastError());
    return BAMD_OK;
}

}  // namespace

bool fpga_matches(const bamd_handle *h) {
    if (h->act != BAMD_ACT_RELU || h->L != 6) return false;
    const std::vector<int> &d = h->dims;
    return d[1] == H1 && d[2] == H2 && d[4] == H2 && d[5] == H1 && d[6] == d[0] && d[0] >= 1 && d[0] <= kMaxF && d[3] >= 1 &&
           d[3] <= kMaxZ;
}

// Training batches the fused pass serves: every fp64 batch (6.5x the layer-wise step at 1M rows), fp32 batches up to kF32TrainRows
// rows (512 rows: 57 vs 91 us); larger fp32 batches run faster on the layer-wise kernels (32768 rows: 211 vs 134 us;
// profiles/fpga_bench.json).
constexpr int64_t kF32TrainRows = 8192;
bool fpga_trains(const bamd_handle *h, int64_t n_rows) {
    return h->fpga_state && (h->esize == 8 || n_rows <= kF32TrainRows);
}

int fpga_setup(bamd_handle *h) {
    if (!fpga_matches(h) || (h->mode != BAMD_MODE_F32 && h->mode != BAMD_MODE_F64)) return BAMD_OK;
    const char *env = getenv("BALER_AMD_FORCE_GENERIC");
    if (env && env[0] == '1') return BAMD_OK;
    FpgaState *st = new FpgaState();
    st->n = h->dims[0];
    st->z = h->dims[3];
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) != hipSuccess) { delete st; set_error("fpga_setup: hipGetDeviceProperties"); return BAMD_ERR_HIP; }
    st->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1;
    h->fpga_state = st;
    return BAMD_OK;
}

void fpga_teardown(bamd_handle *h) {
    FpgaState *st = fst(h);
    if (!st) return;
    st->part.release();
    st->lossp.release();
    delete st;
    h->fpga_state = nullptr;
}

int fpga_infer(bamd_handle *h, InferKind kind, const void *in, int in_dtype, int64_t n, const double *features, void *out, int out_dtype,
               const double *renorm, const uint8_t *int_mask, double *loss_sum, hipStream_t s) {
    BAMD_REQUIRE(in_dtype == BAMD_F32 || in_dtype == BAMD_F64, "bad input dtype");
    BAMD_REQUIRE(!out || out_dtype == BAMD_F32 || out_dtype == BAMD_F64, "bad output dtype");
    BAMD_REQUIRE(!(kind == K_DECODE && renorm && out_dtype != BAMD_F64), "decode with features needs a float64 output");
    if (h->esize == 8) return infer_T<double>(h, kind, in, in_dtype, n, features, out, out_dtype, renorm, int_mask, loss_sum, s);
    return infer_T<float>(h, kind, in, in_dtype, n, features, out, out_dtype, renorm, int_mask, loss_sum, s);
}

int fpga_step(bamd_handle *h, const void *x, int x_dtype, int64_t n, const double *features, const void *latent_grad, void *grads,
              void *params, void *m, void *v, const bamd_adam *hp, double *loss_accum, hipStream_t s) {
    BAMD_REQUIRE(x_dtype == BAMD_F32 || x_dtype == BAMD_F64, "bad input dtype");
    if (h->esize == 8) return step_T<double>(h, x, x_dtype, n, features, latent_grad, grads, params, m, v, hp, loss_accum, s);
    return step_T<float>(h, x, x_dtype, n, features, latent_grad, grads, params, m, v, hp, loss_accum, s);
}

}  // namespace bamd
