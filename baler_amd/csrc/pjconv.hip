// PJ_Conv_AE (reference models.py:668-715) on 28 x 28 frames, float32:
//   encoder.0 Conv2d(1, 20, 5, s2, p2) 28 -> 14, LeakyReLU(0.2); encoder.2 Conv2d(20, 50, 5, s2, p2) 14 -> 7; flatten (c*49 + y*7 + x);
//   encoder.4 Linear(2450, 500); encoder.5 Linear(500, z);
//   decoder.0 Linear(z, 500), LeakyReLU(0.2); decoder.2 Linear(500, 2450), unflatten (50, 7, 7);
//   decoder.4 ConvTranspose2d(50, 20, 5, s2, p2, op1) 7 -> 14; decoder.5 ConvTranspose2d(20, 1, 5, s2, p2, op1) 14 -> 28, LeakyReLU(0.2).
// Loss: utils.mse_sum_loss_l1(validate=True) with number_of_columns = true_data.shape[1] = 1 channel, i.e. the plain sum of squared
// errors (NOT divided by 784).
//
// Every layer except decoder.5 is ONE implicit GEMM on the fp32 MFMA (v_mfma_f32_16x16x4_f32, an exact k-ordered fmaf chain): a
// workgroup of four waves owns a (32 WM) x (32 WN) output tile, stages 32-deep k slices of both operands in LDS through the layer's
// gather (the "op" structs below: zero-padded taps of a strided convolution, the stride-2 phases of a transposed one, rows of a Linear
// layer) and applies the layer's epilogue (bias, LeakyReLU derivative) on the store.  Activations of a group of images live in HBM
// between launches.  decoder.5 (one output channel, K = 500 with 3/4 structural zeros) runs on the VALU with the loss, dL/drecon and
// the decode epilogue (un-normalise + int truncation) fused in.
//
// Backward: the input gradient of a convolution is the transposed convolution with the same weights, that of a transposed
// convolution the direct one, so the same ops serve both directions.  Weight gradients are GEMMs over images x pixels split into
// per-slab partial sums (blockIdx.z); one launch sums the slabs in slab order in float64 (no float atomics: bitwise repeatable).
// Training batches and inference runs are processed in groups of images (kTrainGroup / kInferGroup); the gradient of a multi-group
// batch accumulates group by group in a float64 buffer in group order.
#include <algorithm>
#include <cmath>

#include "bamd_internal.hpp"

namespace bamd {
namespace {

constexpr int P28 = 784, P14 = 196, P7 = 49;
constexpr int C1 = 20, C2 = 50, F2 = C2 * P7, HID = 500;   // F2 = 2450
constexpr float kNeg = 0.2f;                                // nn.LeakyReLU(0.2)
constexpr int kInferGroup = 8192, kTrainGroup = 4096;       // images per group of launches

struct Off {   // offsets of the flat state-dict vector (per tensor: weight row-major, then bias)
    int64_t w1, b1, w2, b2, w4, b4, w5, b5, w6, b6, w7, b7, w8, b8, w9, b9, np;
};
Off offsets(int z) {
    Off o{};
    int64_t p = 0;
    auto take = [&p](int64_t n) { const int64_t q = p; p += n; return q; };
    o.w1 = take(C1 * 25);        o.b1 = take(C1);
    o.w2 = take(C2 * C1 * 25);   o.b2 = take(C2);
    o.w4 = take((int64_t)HID * F2); o.b4 = take(HID);
    o.w5 = take((int64_t)z * HID);  o.b5 = take(z);
    o.w6 = take((int64_t)HID * z);  o.b6 = take(HID);
    o.w7 = take((int64_t)F2 * HID); o.b7 = take(F2);
    o.w8 = take(C2 * C1 * 25);   o.b8 = take(C1);
    o.w9 = take(C1 * 25);        o.b9 = take(1);
    o.np = p;
    return o;
}

__device__ __forceinline__ float lrelu(float v) { return v > 0.f ? v : v * kNeg; }
// torch's leaky_relu_backward: the gradient passes where the pre-activation is > 0; an exact zero takes the 0.2 branch
__device__ __forceinline__ float dlrelu(float pre) { return pre > 0.f ? 1.f : kNeg; }

using v4 = __attribute__((ext_vector_type(4))) float;
constexpr int KC = 32, NTH = 256;

// C[m][n] = sum_{k in slab} op.a(m, k) * op.b(k, n), slab = blockIdx.z covering k in [z * ks, min(K, (z + 1) * ks)).  Operands outside
// the matrix load as zeros (an exact no-op of the fmaf chain).  Wave w owns the WM x WN 16 x 16 blocks at (w >> 1, w & 1).
// Staging: consecutive lanes take consecutive k, or (op.a_mn / op.b_mn) consecutive m / n -- whichever index is contiguous in memory,
// so every operand is read coalesced.
template <class Op, int WM, int WN>
__global__ void __launch_bounds__(NTH) gemm_k(Op op, int M, int N, int K, int ks) {
    constexpr int TM = 32 * WM, TN = 32 * WN;
    __shared__ float As[TM][KC + 1], Bs[TN][KC + 1];
    const int m0 = blockIdx.x * TM, n0 = blockIdx.y * TN;
    const int kb = blockIdx.z * ks, ke = min(K, kb + ks);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = (w >> 1) * 16 * WM, wn = (w & 1) * 16 * WN;
    v4 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) acc[i][j] = v4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = kb; k0 < ke; k0 += KC) {
#pragma unroll
        for (int e = tid; e < TM * KC; e += NTH) {
            const int r = op.a_mn ? e % TM : e >> 5, kk = op.a_mn ? e / TM : e & 31, k = k0 + kk, m = m0 + r;
            As[r][kk] = (m < M && k < ke) ? op.a(m, k) : 0.f;
        }
#pragma unroll
        for (int e = tid; e < TN * KC; e += NTH) {
            const int r = op.b_mn ? e % TN : e >> 5, kk = op.b_mn ? e / TN : e & 31, k = k0 + kk, n = n0 + r;
            Bs[r][kk] = (n < N && k < ke) ? op.b(k, n) : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < KC; kk += 4) {
            float a[WM], b[WN];
#pragma unroll
            for (int i = 0; i < WM; ++i) a[i] = As[wm + 16 * i + (lane & 15)][kk + (lane >> 4)];
#pragma unroll
            for (int j = 0; j < WN; ++j) b[j] = Bs[wn + 16 * j + (lane & 15)][kk + (lane >> 4)];
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int n = n0 + wn + 16 * j + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + 16 * i + (lane >> 4) * 4 + r;
                if (m < M && n < N) op.store(m, n, acc[i][j][r], blockIdx.z);
            }
        }
}

// ---- the layers as GEMM operand gathers ---------------------------------------------------------------------------------------------
// Linear: out[m][n] = sum_k act(in[m][k]) * W(n, k) (+ bias[n]) (* lrelu'(pre[m][n])).  wt = 0: W(n, k) = w[n][k] (forward);
// wt = 1: W(n, k) = w[k][n] (input gradient through w).  out64: float64 output instead of `out`.
struct LinOp {
    const float *in, *w, *bias, *pre;
    float *out;
    double *out64;
    int N, K, in_leaky, wt;
    int a_mn, b_mn;     // b_mn = wt: w[k][n] is contiguous in n
    __device__ float a(int m, int k) const { const float v = in[(int64_t)m * K + k]; return in_leaky ? lrelu(v) : v; }
    __device__ float b(int k, int n) const { return wt ? w[(int64_t)k * N + n] : w[(int64_t)n * K + k]; }
    __device__ void store(int m, int n, float acc, int) const {
        const int64_t i = (int64_t)m * N + n;
        float v = bias ? acc + bias[n] : acc;
        if (pre) v *= dlrelu(pre[i]);
        if (out64) out64[i] = (double)v; else out[i] = v;
    }
};

// Conv2d(CIN -> N, k5, stride 2, pad 2) HIN -> HOUT: rows m = (image, output pixel), k = (ci, ky, kx), w[n][ci][ky][kx].
template <int CIN, int HIN, int HOUT>
struct ConvOp {
    static constexpr int PI = HIN * HIN, PO = HOUT * HOUT, K = CIN * 25;
    const float *in, *w, *bias;
    float *out;
    int N, in_leaky;
    static constexpr int a_mn = 0, b_mn = 0;
    __device__ float a(int m, int k) const {
        const int b = m / PO, p = m - b * PO, oy = p / HOUT, ox = p - oy * HOUT;
        const int ci = k / 25, t = k - ci * 25, ky = t / 5, kx = t - ky * 5;
        const int iy = 2 * oy - 2 + ky, ix = 2 * ox - 2 + kx;
        if ((unsigned)iy >= (unsigned)HIN || (unsigned)ix >= (unsigned)HIN) return 0.f;
        const float v = in[(int64_t)b * (CIN * PI) + ci * PI + iy * HIN + ix];
        return in_leaky ? lrelu(v) : v;
    }
    __device__ float b(int k, int n) const { return w[n * K + k]; }
    __device__ void store(int m, int n, float acc, int) const {
        const int b = m / PO, p = m - b * PO;
        out[(int64_t)b * N * PO + n * PO + p] = bias ? acc + bias[n] : acc;
    }
};

// ConvTranspose2d(CIN -> N, k5, stride 2, pad 2, output_padding 1) HIN -> 2 HIN as an output-stationary gather, ONE stride-2 phase
// (PY, PX) per launch: out[oy][ox] += in[iy][ix] * w[ci][n][ky][kx] where oy = 2 iy - 2 + ky, so an output row of parity PY takes
// only the taps ky = PY, PY + 2, ... (3 taps for PY = 0, 2 for PY = 1) from input rows iy = qy + 1 - jy (oy = 2 qy + PY, ky = PY + 2 jy).
// Rows m = (image, qy, qx) of the phase, k = (ci, jy, jx): no k slot holds a structural zero; only taps past the image border load as
// zeros.  Epilogue: + bias, or * lrelu'(pre) (the input gradient of a LeakyReLU-activated convolution).
template <int CIN, int HIN, int PY, int PX>
struct ConvTOp {
    static constexpr int HOUT = 2 * HIN, PI = HIN * HIN, PO = HOUT * HOUT, TY = 3 - PY, TX = 3 - PX, T = TY * TX, K = CIN * T;
    static constexpr int a_mn = 0, b_mn = 0;
    const float *in, *w, *bias, *pre;
    float *out;
    int N;
    __device__ float a(int m, int k) const {
        const int b = m / PI, q = m - b * PI, qy = q / HIN, qx = q - qy * HIN;
        const int ci = k / T, t = k - ci * T, jy = t / TX, jx = t - jy * TX;
        const int iy = qy + 1 - jy, ix = qx + 1 - jx;
        if ((unsigned)iy >= (unsigned)HIN || (unsigned)ix >= (unsigned)HIN) return 0.f;
        return in[(int64_t)b * (CIN * PI) + ci * PI + iy * HIN + ix];
    }
    __device__ float b(int k, int n) const {
        const int ci = k / T, t = k - ci * T, jy = t / TX, jx = t - jy * TX;
        return w[(ci * N + n) * 25 + (PY + 2 * jy) * 5 + PX + 2 * jx];
    }
    __device__ void store(int m, int n, float acc, int) const {
        const int b = m / PI, q = m - b * PI, qy = q / HIN, qx = q - qy * HIN;
        const int64_t i = (int64_t)b * N * PO + n * PO + (2 * qy + PY) * HOUT + 2 * qx + PX;
        float v = bias ? acc + bias[n] : acc;
        if (pre) v *= dlrelu(pre[i]);
        out[i] = v;
    }
};

// Linear weight gradient of one slab of images: dW[o][i] = sum_b d[b][o] * act(x[b][i]); the extra column n = I is db[o].
struct LinWgradOp {
    const float *d, *x;
    float *slab;
    int64_t pg;
    int O, I, x_leaky;
    static constexpr int a_mn = 1, b_mn = 1;     // d[b][o] and x[b][i] are contiguous along o / i
    __device__ float a(int m, int k) const { return d[(int64_t)k * O + m]; }
    __device__ float b(int k, int n) const {
        if (n == I) return 1.f;
        const float v = x[(int64_t)k * I + n];
        return x_leaky ? lrelu(v) : v;
    }
    __device__ void store(int m, int n, float acc, int s) const {
        slab[s * pg + (n < I ? (int64_t)m * I + n : (int64_t)O * I + m)] = acc;
    }
};

// Weight gradient of a stride-2 (transposed) convolution between a small grid HS (CS channels) and the large grid HL = 2 HS (CL
// channels): dW[cs][cl][ky][kx] = sum_{image, y, x} sm[cs][y][x] * lg[cl][2y - 2 + ky][2x - 2 + kx].  For Conv2d the small side is the
// output (dW[out][in]); for ConvTranspose2d it is the input (dW[in][out]): one op for both.  with_bias: column CL*25 is sum sm[cs].
template <int CL, int HL, int HS>
struct ConvWgradOp {
    static constexpr int PS = HS * HS, PL = HL * HL, NW = CL * 25;
    const float *sm, *lg;
    float *slab;
    int64_t pg;
    int CS, lg_leaky;
    static constexpr int a_mn = 0, b_mn = 0;
    __device__ float a(int m, int k) const { const int b = k / PS, p = k - b * PS; return sm[(int64_t)b * CS * PS + m * PS + p]; }
    __device__ float b(int k, int n) const {
        if (n == NW) return 1.f;
        const int b = k / PS, p = k - b * PS, y = p / HS, x = p - y * HS;
        const int cl = n / 25, t = n - cl * 25, ky = t / 5, kx = t - ky * 5;
        const int iy = 2 * y - 2 + ky, ix = 2 * x - 2 + kx;
        if ((unsigned)iy >= (unsigned)HL || (unsigned)ix >= (unsigned)HL) return 0.f;
        const float v = lg[(int64_t)b * (CL * PL) + cl * PL + iy * HL + ix];
        return lg_leaky ? lrelu(v) : v;
    }
    __device__ void store(int m, int n, float acc, int s) const {
        slab[s * pg + (n < NW ? (int64_t)m * NW + n : (int64_t)CS * NW + m)] = acc;
    }
};

// Bias gradient of a transposed convolution: db[c] = sum_{image, pixel} d[c][pixel].
template <int P>
struct ChanSumOp {
    const float *d;
    float *slab;
    int64_t pg;
    int C;
    static constexpr int a_mn = 0, b_mn = 0;
    __device__ float a(int m, int k) const { const int b = k / P, p = k - b * P; return d[(int64_t)b * C * P + m * P + p]; }
    __device__ float b(int, int) const { return 1.f; }
    __device__ void store(int m, int, float acc, int s) const { slab[s * pg + m] = acc; }
};

template <int WM, int WN, class Op>
int gemm(const Op &op, int M, int N, int K, int ks, hipStream_t s) {
    if (M <= 0 || N <= 0 || K <= 0) return BAMD_OK;
    dim3 g((unsigned)((M + 32 * WM - 1) / (32 * WM)), (unsigned)((N + 32 * WN - 1) / (32 * WN)), (unsigned)((K + ks - 1) / ks));
    hipLaunchKernelGGL((gemm_k<Op, WM, WN>), g, dim3(NTH), 0, s, op, M, N, K, ks);
    BAMD_HIP(hipGetLastError());
    return BAMD_OK;
}

// ---- row staging, decoder.5 + loss, slab and loss reductions ------------------------------------------------------------------------
// rows -> float32, min-max normalised on load in float64 ((x - min) / range, as normalize_k) when feat is given
__global__ void __launch_bounds__(256) prep_k(const void *x, int f64, int64_t count, const double *feat, float *out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    const double v = f64 ? ((const double *)x)[e] : (double)((const float *)x)[e];
    const int c = (int)(e % P28);
    out[e] = feat ? (float)((v - feat[c]) / feat[P28 + c]) : (float)v;
}

// decoder.5 per output pixel (thread = (image, pixel)): pre = b + sum over the 2-3 x 2-3 taps of its stride-2 phase, recon = lrelu(pre).
// kind 1 (decode): store recon (float32 / float64; renorm: x * range + min, int truncation, float64).  kind 2 (forward + loss): loss
// partial, recon optional.  kind 3 (training): loss partial and dL/dpre = 2 (recon - x) lrelu'(pre).  One float64 loss partial per
// workgroup, summed in a fixed tree.
struct Dec5Args {
    const float *y8, *w9, *b9, *xn;
    float *d9;
    void *out;
    int out_f64, kind;
    const double *renorm;
    const uint8_t *int_mask;
    double *loss_part;
    int64_t count;
};
__global__ void __launch_bounds__(256) dec5_k(Dec5Args a) {
    __shared__ double sh[256];
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double l = 0.0;
    if (e < a.count) {
        const int64_t b = e / P28;
        const int p = (int)(e - b * P28), oy = p / 28, ox = p - oy * 28;
        const float *in = a.y8 + b * (C1 * P14);
        float acc = 0.f;
        for (int ci = 0; ci < C1; ++ci)
            for (int ky = (oy & 1); ky < 5; ky += 2) {
                const int iy = (oy + 2 - ky) >> 1;
                if (iy < 0 || iy >= 14) continue;
                for (int kx = (ox & 1); kx < 5; kx += 2) {
                    const int ix = (ox + 2 - kx) >> 1;
                    if (ix < 0 || ix >= 14) continue;
                    acc = fmaf(in[ci * P14 + iy * 14 + ix], a.w9[ci * 25 + ky * 5 + kx], acc);
                }
            }
        const float pre = acc + a.b9[0];
        const float r = lrelu(pre);
        if (a.kind == 1 && a.renorm) {
            double o = __dadd_rn(__dmul_rn((double)r, a.renorm[P28 + p]), a.renorm[p]);
            if (a.int_mask && a.int_mask[p]) o = trunc(o);
            ((double *)a.out)[e] = o;
        } else if (a.out) {
            if (a.out_f64) ((double *)a.out)[e] = (double)r; else ((float *)a.out)[e] = r;
        }
        if (a.kind >= 2) {
            const double d = (double)r - (double)a.xn[e];
            l = d * d;
            if (a.kind == 3) a.d9[e] = 2.f * (r - a.xn[e]) * dlrelu(pre);
        }
    }
    if (!a.loss_part) return;
    const double wsum = block_sum_tree(l, sh);
    if (threadIdx.x == 0) a.loss_part[blockIdx.x] = wsum;
}

__global__ void __launch_bounds__(256) loss_final_k(const double *part, int n, float *gloss, double *loss_sum) {
    __shared__ double sh[256];
    const double s = block_sum_fixed(part, n, sh);
    if (threadIdx.x == 0) {
        if (gloss) *gloss = (float)s;
        if (loss_sum) *loss_sum = s;
    }
}

struct Region {
    const float *slab;
    int64_t p0, pg;
    int S;
};
constexpr int kRegions = 10;
struct Regions { Region r[kRegions]; };
// gradient[p0 + i] = sum over the slabs in slab order (float64), + the previous groups' sum, rounded once on the last group
__global__ void __launch_bounds__(256) reduce_k(Regions R, double *gacc, float *grads, int first, int last) {
    const Region g = R.r[blockIdx.y];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < g.pg; i += (int64_t)gridDim.x * 256) {
        double a = 0.0;
        for (int s = 0; s < g.S; ++s) a += (double)g.slab[s * g.pg + i];
        if (!first) a += gacc[g.p0 + i];
        if (last) grads[g.p0 + i] = (float)a;
        else gacc[g.p0 + i] = a;
    }
}

// ---- handle state -----------------------------------------------------------------------------------------------------------------
struct PJState {
    int z;
    Off o;
    DevBuf ws;      // activations (and, training, their gradients) of one group of images
    DevBuf slab;    // per-slab partial weight gradients of one group
    DevBuf gacc;    // float64 gradient of the groups so far (batches of more than kTrainGroup images)
    DevBuf lossp;   // per-workgroup loss partials of the whole call
};

struct Bufs {
    float *X, *A1, *Y2, *Y4, *Z, *A6, *Y7, *Y8;   // forward: input, encoder.0 pre-activation, ..., decoder.4 output
    float *D9, *D8, *D7, *D6, *DZ, *D4, *D2, *D1;  // backward: dL/d(pre-)activation of the same tensors
};
int64_t fwd_floats(int z) { return P28 + C1 * P14 + F2 + HID + z + HID + F2 + C1 * P14; }
Bufs carve(float *p, int64_t g, int z, bool train) {
    Bufs B{};
    float **f[] = {&B.X, &B.A1, &B.Y2, &B.Y4, &B.Z, &B.A6, &B.Y7, &B.Y8};
    float **d[] = {&B.D9, &B.D8, &B.D7, &B.D6, &B.DZ, &B.D4, &B.D2, &B.D1};
    const int64_t w[] = {P28, C1 * P14, F2, HID, z, HID, F2, C1 * P14};
    for (int i = 0; i < 8; ++i) { *f[i] = p; p += g * w[i]; }
    if (train)
        for (int i = 0; i < 8; ++i) { *d[i] = p; p += g * w[i]; }
    return B;
}

PJState *state(bamd_handle *h) { return (PJState *)h->pj_state; }
const float *W(bamd_handle *h, int64_t off) { return (const float *)h->params.p + off; }

// x rows [0, n) -> the group's float32 input (normalised on load); float32 rows without features are read in place
int stage_rows(const void *x, int f64, int64_t n, const double *feat, float *X, const float **xin, hipStream_t s) {
    if (!f64 && !feat) { *xin = (const float *)x; return BAMD_OK; }
    const int64_t cnt = n * P28;
    hipLaunchKernelGGL(prep_k, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, x, f64, cnt, feat, X);
    BAMD_HIP(hipGetLastError());
    *xin = X;
    return BAMD_OK;
}

// ConvTranspose2d 50 -> 20, 7x7 -> 14x14 (decoder.4, and encoder.2's input gradient): one launch per stride-2 phase
int convT_50_20(const float *in, const float *w, const float *bias, const float *pre, float *out, int nb, hipStream_t s) {
    int rc = gemm<2, 1>(ConvTOp<C2, 7, 0, 0>{in, w, bias, pre, out, C1}, nb * P7, C1, C2 * 9, C2 * 9, s);
    if (!rc) rc = gemm<2, 1>(ConvTOp<C2, 7, 0, 1>{in, w, bias, pre, out, C1}, nb * P7, C1, C2 * 6, C2 * 6, s);
    if (!rc) rc = gemm<2, 1>(ConvTOp<C2, 7, 1, 0>{in, w, bias, pre, out, C1}, nb * P7, C1, C2 * 6, C2 * 6, s);
    if (!rc) rc = gemm<2, 1>(ConvTOp<C2, 7, 1, 1>{in, w, bias, pre, out, C1}, nb * P7, C1, C2 * 4, C2 * 4, s);
    return rc;
}

#define PJ_TRY(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)

int encoder(bamd_handle *h, const Bufs &B, const float *x, int nb, float *z32, double *z64, hipStream_t s) {
    const Off &o = state(h)->o;
    const int z = state(h)->z;
    PJ_TRY((gemm<2, 1>(ConvOp<1, 28, 14>{x, W(h, o.w1), W(h, o.b1), B.A1, C1, 0}, nb * P14, C1, 25, 25, s)));
    PJ_TRY((gemm<2, 2>(ConvOp<C1, 14, 7>{B.A1, W(h, o.w2), W(h, o.b2), B.Y2, C2, 1}, nb * P7, C2, C1 * 25, C1 * 25, s)));
    PJ_TRY((gemm<1, 1>(LinOp{B.Y2, W(h, o.w4), W(h, o.b4), nullptr, B.Y4, nullptr, HID, F2, 0, 0, 0, 0}, nb, HID, F2, F2, s)));
    return gemm<1, 1>(LinOp{B.Y4, W(h, o.w5), W(h, o.b5), nullptr, z32, z64, z, HID, 0, 0, 0, 0}, nb, z, HID, HID, s);
}

// decoder.0 .. decoder.4 (decoder.5 is dec5_k)
int decoder_convs(bamd_handle *h, const Bufs &B, const float *zin, int nb, hipStream_t s) {
    const Off &o = state(h)->o;
    const int z = state(h)->z;
    PJ_TRY((gemm<1, 1>(LinOp{zin, W(h, o.w6), W(h, o.b6), nullptr, B.A6, nullptr, HID, z, 0, 0, 0, 0}, nb, HID, z, z, s)));
    PJ_TRY((gemm<1, 2>(LinOp{B.A6, W(h, o.w7), W(h, o.b7), nullptr, B.Y7, nullptr, F2, HID, 1, 0, 0, 0}, nb, F2, HID, HID, s)));
    return convT_50_20(B.Y7, W(h, o.w8), W(h, o.b8), nullptr, B.Y8, nb, s);
}

int dec5(bamd_handle *h, const Bufs &B, int nb, int kind, const float *xn, void *out, int out_f64, const double *renorm,
         const uint8_t *int_mask, double *loss_part, hipStream_t s) {
    const Off &o = state(h)->o;
    Dec5Args a{B.Y8, W(h, o.w9), W(h, o.b9), xn, B.D9, out, out_f64, kind, renorm, int_mask, loss_part, (int64_t)nb * P28};
    hipLaunchKernelGGL(dec5_k, dim3((unsigned)((a.count + 255) / 256)), dim3(256), 0, s, a);
    BAMD_HIP(hipGetLastError());
    return BAMD_OK;
}
int dec5_blocks(int64_t nb) { return (int)((nb * P28 + 255) / 256); }

int ensure_ws(bamd_handle *h, int64_t g, bool train) {
    PJState *st = state(h);
    return st->ws.ensure((size_t)g * fwd_floats(st->z) * (train ? 2 : 1) * sizeof(float));
}

// images per weight-gradient slab (the K split of each reduction over images x pixels)
constexpr int kSlabLin = 256, kSlabConv2 = 16, kSlabConv1 = 4, kSlabBias9 = 1;

struct WgradPlan {
    Regions R;
    int64_t floats;
};
WgradPlan wgrad_plan(const PJState *st, int nb, float *base) {
    const Off &o = st->o;
    const int z = st->z;
    const int64_t p0[kRegions] = {o.w1, o.w2, o.w4, o.w5, o.w6, o.w7, o.w8, o.b8, o.w9, o.b9};
    const int64_t pg[kRegions] = {C1 * 25 + C1, C2 * C1 * 25 + C2, (int64_t)HID * F2 + HID, (int64_t)z * HID + z, (int64_t)HID * z + HID,
                                  (int64_t)F2 * HID + F2, C2 * C1 * 25, C1, C1 * 25, 1};
    const int per[kRegions] = {kSlabConv1, kSlabConv2, kSlabLin, kSlabLin, kSlabLin, kSlabLin, kSlabConv2, kSlabConv1, kSlabConv1, kSlabBias9};
    WgradPlan P{};
    int64_t off = 0;
    for (int i = 0; i < kRegions; ++i) {
        const int S = (nb + per[i] - 1) / per[i];
        P.R.r[i] = Region{base ? base + off : nullptr, p0[i], pg[i], S};
        off += (int64_t)S * pg[i];
    }
    P.floats = off;
    return P;
}

// forward + loss + backward of one group of nb images whose normalised rows are `x`; weight gradients into the slabs of `P`
int group_fwd_bwd(bamd_handle *h, const Bufs &B, const float *x, int nb, const WgradPlan &P, double *loss_part, hipStream_t s) {
    const PJState *st = state(h);
    const Off &o = st->o;
    const int z = st->z;
    PJ_TRY(encoder(h, B, x, nb, B.Z, nullptr, s));
    PJ_TRY(decoder_convs(h, B, B.Z, nb, s));
    PJ_TRY(dec5(h, B, nb, 3, x, nullptr, 0, nullptr, nullptr, loss_part, s));
    // input gradients, decoder.5 back to encoder.0
    PJ_TRY((gemm<2, 1>(ConvOp<1, 28, 14>{B.D9, W(h, o.w9), nullptr, B.D8, C1, 0}, nb * P14, C1, 25, 25, s)));
    PJ_TRY((gemm<2, 2>(ConvOp<C1, 14, 7>{B.D8, W(h, o.w8), nullptr, B.D7, C2, 0}, nb * P7, C2, C1 * 25, C1 * 25, s)));
    PJ_TRY((gemm<1, 1>(LinOp{B.D7, W(h, o.w7), nullptr, B.A6, B.D6, nullptr, HID, F2, 0, 1, 0, 1}, nb, HID, F2, F2, s)));
    PJ_TRY((gemm<1, 1>(LinOp{B.D6, W(h, o.w6), nullptr, nullptr, B.DZ, nullptr, z, HID, 0, 1, 0, 1}, nb, z, HID, HID, s)));
    PJ_TRY((gemm<1, 1>(LinOp{B.DZ, W(h, o.w5), nullptr, nullptr, B.D4, nullptr, HID, z, 0, 1, 0, 1}, nb, HID, z, z, s)));
    PJ_TRY((gemm<1, 2>(LinOp{B.D4, W(h, o.w4), nullptr, nullptr, B.D2, nullptr, F2, HID, 0, 1, 0, 1}, nb, F2, HID, HID, s)));
    PJ_TRY(convT_50_20(B.D2, W(h, o.w2), nullptr, B.A1, B.D1, nb, s));
    // weight gradients (region order of wgrad_plan)
    float *sl[kRegions];
    for (int i = 0; i < kRegions; ++i) sl[i] = (float *)P.R.r[i].slab;
    const Region *R = P.R.r;
    PJ_TRY((gemm<1, 1>(ConvWgradOp<1, 28, 14>{B.D1, x, sl[0], R[0].pg, C1, 0}, C1, 25 + 1, nb * P14, kSlabConv1 * P14, s)));
    PJ_TRY((gemm<2, 2>(ConvWgradOp<C1, 14, 7>{B.D2, B.A1, sl[1], R[1].pg, C2, 1}, C2, C1 * 25 + 1, nb * P7, kSlabConv2 * P7, s)));
    PJ_TRY((gemm<1, 1>(LinWgradOp{B.D4, B.Y2, sl[2], R[2].pg, HID, F2, 0}, HID, F2 + 1, nb, kSlabLin, s)));
    PJ_TRY((gemm<1, 1>(LinWgradOp{B.DZ, B.Y4, sl[3], R[3].pg, z, HID, 0}, z, HID + 1, nb, kSlabLin, s)));
    PJ_TRY((gemm<1, 1>(LinWgradOp{B.D6, B.Z, sl[4], R[4].pg, HID, z, 0}, HID, z + 1, nb, kSlabLin, s)));
    PJ_TRY((gemm<1, 1>(LinWgradOp{B.D7, B.A6, sl[5], R[5].pg, F2, HID, 1}, F2, HID + 1, nb, kSlabLin, s)));
    PJ_TRY((gemm<2, 2>(ConvWgradOp<C1, 14, 7>{B.Y7, B.D8, sl[6], R[6].pg, C2, 0}, C2, C1 * 25, nb * P7, kSlabConv2 * P7, s)));
    PJ_TRY((gemm<1, 1>(ChanSumOp<P14>{B.D8, sl[7], R[7].pg, C1}, C1, 1, nb * P14, kSlabConv1 * P14, s)));
    PJ_TRY((gemm<1, 1>(ConvWgradOp<1, 28, 14>{B.Y8, B.D9, sl[8], R[8].pg, C1, 0}, C1, 25, nb * P14, kSlabConv1 * P14, s)));
    return gemm<1, 1>(ChanSumOp<P28>{B.D9, sl[9], R[9].pg, 1}, 1, 1, nb * P28, kSlabBias9 * P28, s);
}

}  // namespace

int pj_setup(bamd_handle *h, int z) {
    PJState *st = new PJState();
    st->z = z;
    st->o = offsets(z);
    h->pj_state = st;
    return BAMD_OK;
}

void pj_teardown(bamd_handle *h) {
    PJState *st = state(h);
    if (!st) return;
    st->ws.release();
    st->slab.release();
    st->gacc.release();
    st->lossp.release();
    delete st;
    h->pj_state = nullptr;
}

int64_t pj_param_count(int z) { return offsets(z).np; }

int pj_encode(bamd_handle *h, const void *x, int x_dtype, int64_t n, const double *features, void *z, int z_dtype, hipStream_t s) {
    BAMD_REQUIRE(x_dtype == BAMD_F32 || x_dtype == BAMD_F64, "bad x dtype");
    BAMD_REQUIRE(z_dtype == BAMD_F32 || z_dtype == BAMD_F64, "bad z dtype");
    PJState *st = state(h);
    const int64_t G = std::min<int64_t>(n, kInferGroup);
    PJ_TRY(ensure_ws(h, G, false));
    const Bufs B = carve((float *)st->ws.p, G, st->z, false);
    const size_t xb = dtype_bytes(x_dtype);
    for (int64_t r0 = 0; r0 < n; r0 += G) {
        const int nb = (int)std::min<int64_t>(G, n - r0);
        const float *xin = nullptr;
        PJ_TRY(stage_rows((const char *)x + (size_t)r0 * P28 * xb, x_dtype == BAMD_F64, nb, features, B.X, &xin, s));
        float *z32 = z_dtype == BAMD_F32 ? (float *)z + r0 * st->z : nullptr;
        double *z64 = z_dtype == BAMD_F64 ? (double *)z + r0 * st->z : nullptr;
        PJ_TRY(encoder(h, B, xin, nb, z32, z64, s));
    }
    return BAMD_OK;
}

int pj_decode(bamd_handle *h, const void *z, int z_dtype, int64_t n, const double *renorm, const uint8_t *int_mask, void *out,
              int out_dtype, hipStream_t s) {
    BAMD_REQUIRE(z_dtype == BAMD_F32 || z_dtype == BAMD_F64, "bad z dtype");
    BAMD_REQUIRE(out_dtype == BAMD_F32 || out_dtype == BAMD_F64, "bad output dtype");
    BAMD_REQUIRE(!(renorm && out_dtype != BAMD_F64), "decode with features needs a float64 output");
    PJState *st = state(h);
    const int64_t G = std::min<int64_t>(n, kInferGroup);
    PJ_TRY(ensure_ws(h, G, false));
    const Bufs B = carve((float *)st->ws.p, G, st->z, false);
    const size_t ob = dtype_bytes(out_dtype);
    for (int64_t r0 = 0; r0 < n; r0 += G) {
        const int nb = (int)std::min<int64_t>(G, n - r0);
        const float *zin = (const float *)z + r0 * st->z;
        if (z_dtype == BAMD_F64) {
            PJ_TRY(launch_convert((const double *)z + r0 * st->z, BAMD_F64, B.Z, BAMD_F32, (int64_t)nb * st->z, s));
            zin = B.Z;
        }
        PJ_TRY(decoder_convs(h, B, zin, nb, s));
        PJ_TRY(dec5(h, B, nb, 1, nullptr, (char *)out + (size_t)r0 * P28 * ob, out_dtype == BAMD_F64, renorm, int_mask, nullptr, s));
    }
    return BAMD_OK;
}

int pj_forward_loss(bamd_handle *h, const void *x, int x_dtype, int64_t n, const double *features, void *recon, int recon_dtype,
                    double *loss_sum, hipStream_t s) {
    BAMD_REQUIRE(x_dtype == BAMD_F32 || x_dtype == BAMD_F64, "bad x dtype");
    BAMD_REQUIRE(!recon || recon_dtype == BAMD_F32 || recon_dtype == BAMD_F64, "bad recon dtype");
    PJState *st = state(h);
    const int64_t G = std::min<int64_t>(n, kInferGroup);
    PJ_TRY(ensure_ws(h, G, false));
    const Bufs B = carve((float *)st->ws.p, G, st->z, false);
    int64_t nparts = 0;
    for (int64_t r0 = 0; r0 < n; r0 += G) nparts += dec5_blocks(std::min<int64_t>(G, n - r0));
    PJ_TRY(st->lossp.ensure((size_t)nparts * sizeof(double)));
    const size_t xb = dtype_bytes(x_dtype), rb = dtype_bytes(recon_dtype);
    int64_t part = 0;
    for (int64_t r0 = 0; r0 < n; r0 += G) {
        const int nb = (int)std::min<int64_t>(G, n - r0);
        const float *xin = nullptr;
        PJ_TRY(stage_rows((const char *)x + (size_t)r0 * P28 * xb, x_dtype == BAMD_F64, nb, features, B.X, &xin, s));
        PJ_TRY(encoder(h, B, xin, nb, B.Z, nullptr, s));
        PJ_TRY(decoder_convs(h, B, B.Z, nb, s));
        void *r = recon ? (char *)recon + (size_t)r0 * P28 * rb : nullptr;
        PJ_TRY(dec5(h, B, nb, 2, xin, r, recon_dtype == BAMD_F64, nullptr, nullptr, (double *)st->lossp.p + part, s));
        part += dec5_blocks(nb);
    }
    hipLaunchKernelGGL(loss_final_k, dim3(1), dim3(256), 0, s, (const double *)st->lossp.p, (int)nparts, (float *)nullptr, loss_sum);
    BAMD_HIP(hipGetLastError());
    return BAMD_OK;
}

int pj_step(bamd_handle *h, const void *x, int x_dtype, int64_t n, const double *features, void *grads, void *params, void *m, void *v,
            const bamd_adam *hp, double *loss_accum, hipStream_t s) {
    BAMD_REQUIRE(x_dtype == BAMD_F32 || x_dtype == BAMD_F64, "bad x dtype");
    PJState *st = state(h);
    if (!grads) {
        PJ_TRY(h->gscratch.ensure((size_t)(h->nparams + 1) * sizeof(float)));
        grads = h->gscratch.p;
    }
    const int64_t G = std::min<int64_t>(n, kTrainGroup);
    PJ_TRY(ensure_ws(h, G, true));
    const Bufs B = carve((float *)st->ws.p, G, st->z, true);
    PJ_TRY(st->slab.ensure((size_t)wgrad_plan(st, (int)G, nullptr).floats * sizeof(float)));
    const int64_t groups = (n + G - 1) / G;
    if (groups > 1) PJ_TRY(st->gacc.ensure((size_t)h->nparams * sizeof(double)));
    int64_t nparts = 0;
    for (int64_t r0 = 0; r0 < n; r0 += G) nparts += dec5_blocks(std::min<int64_t>(G, n - r0));
    PJ_TRY(st->lossp.ensure((size_t)nparts * sizeof(double)));
    const size_t xb = dtype_bytes(x_dtype);
    int64_t part = 0, gi = 0;
    for (int64_t r0 = 0; r0 < n; r0 += G, ++gi) {
        const int nb = (int)std::min<int64_t>(G, n - r0);
        const float *xin = nullptr;
        PJ_TRY(stage_rows((const char *)x + (size_t)r0 * P28 * xb, x_dtype == BAMD_F64, nb, features, B.X, &xin, s));
        const WgradPlan P = wgrad_plan(st, nb, (float *)st->slab.p);
        PJ_TRY(group_fwd_bwd(h, B, xin, nb, P, (double *)st->lossp.p + part, s));
        part += dec5_blocks(nb);
        int64_t maxpg = 0;
        for (int i = 0; i < kRegions; ++i) maxpg = std::max(maxpg, P.R.r[i].pg);
        const unsigned gx = (unsigned)std::min<int64_t>((maxpg + 255) / 256, 2048);
        hipLaunchKernelGGL(reduce_k, dim3(gx, kRegions), dim3(256), 0, s, P.R, (double *)st->gacc.p, (float *)grads, gi == 0 ? 1 : 0,
                           gi == groups - 1 ? 1 : 0);
        BAMD_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(loss_final_k, dim3(1), dim3(256), 0, s, (const double *)st->lossp.p, (int)nparts, (float *)grads + h->nparams,
                       (double *)nullptr);
    BAMD_HIP(hipGetLastError());
    if (!hp) return BAMD_OK;
    return launch_adam(params, h->params.p, grads, m, v, h->nparams, sizeof(float), *hp, loss_accum, nullptr, nullptr, nullptr, s);
}

}  // namespace bamd
