// What the 16-bit inference kernels share (bf16.hip: bfloat16 and binary16; f16x3.hip: split binary16): the operand vector types,
// the BNet geometry of AE(F, Z) on the 16x16x32 MFMA with its fragment index maps, the row loaders, the bias pack kernel, and the
// store / loss epilogues of the two fp32 outputs (latent, reconstruction) as functions.  Device code in an anonymous namespace: every translation unit has its own copy.
#pragma once
#include "bamd_internal.hpp"

#include <type_traits>
#include <vector>

namespace bamd {
namespace {

// The 16-bit element type is a template parameter: V = bf8 (bfloat16, BAMD_MODE_BF16) or h8 (IEEE binary16, BAMD_MODE_F16: the
// contract is in include/baler_amd.h, the measurements in DESIGN.md section 13).  Geometry, LDS staging, loaders and the layer
// loops are the same text for both; the MFMA builtin, the rounding of a packed value and the activation epilogue (mfma16,
// pack8, act_pack in bf16.hip) differ.
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
template <class V> struct Elem;
template <> struct Elem<bf8> { using T = __bf16; };
template <> struct Elem<h8> { using T = _Float16; };
using v4 = float __attribute__((ext_vector_type(4)));

template <int F, int Z> struct BNet {
    static constexpr int L = 8;
    __host__ __device__ static constexpr int dim(int i) {
        return i == 0 ? F : i == 1 ? 200 : i == 2 ? 100 : i == 3 ? 50 : i == 4 ? Z : i == 5 ? 50 : i == 6 ? 100 : i == 7 ? 200 : F;
    }
    __host__ __device__ static constexpr bool act(int l) { return !(l == 3 || l == 7); }
    __host__ __device__ static constexpr int kb(int l) { return (dim(l) + 31) / 32; }       // 32-wide k blocks
    __host__ __device__ static constexpr int nt(int l) { return (dim(l + 1) + 15) / 16; }   // 16-wide output tiles
    __host__ __device__ static constexpr int frags(int l) { return kb(l) * nt(l); }
    // fragment / bias offsets inside a half (encoder = layers 0..3, decoder = 4..7)
    __host__ __device__ static constexpr int f_off(int l) { int s = 0; for (int j = (l < 4 ? 0 : 4); j < l; ++j) s += frags(j); return s; }
    __host__ __device__ static constexpr int b_off(int l) { int s = 0; for (int j = (l < 4 ? 0 : 4); j < l; ++j) s += nt(j) * 4; return s; }
    __host__ __device__ static constexpr int half_frags(int h) { return f_off(4 * h + 3) + frags(4 * h + 3); }
    __host__ __device__ static constexpr int half_bias(int h) { return b_off(4 * h + 3) + nt(4 * h + 3) * 4; }
    // input feature behind k slot (block q, lane group g, element e) of layer l; -1 = zero padding.
    // Layers fed from memory (0 and 4) use 8 consecutive features per lane; the others the C-tile pairing.
    __host__ __device__ static constexpr int in_feature(int l, int q, int g, int e) {
        int f = (l == 0 || l == 4) ? 32 * q + 8 * g + e : 32 * q + 16 * (e >> 2) + 4 * g + (e & 3);
        return f < dim(l) ? f : -1;
    }
    __host__ __device__ static constexpr int w_off_c(int l) { int s = 0; for (int j = 0; j < l; ++j) s += dim(j + 1) * dim(j) + dim(j + 1); return s; }
    __host__ __device__ static constexpr int b_off_c(int l) { return w_off_c(l) + dim(l + 1) * dim(l); }
    __host__ __device__ static constexpr int nparams() { return w_off_c(L); }
    static_assert(F <= 32 && Z <= 32, "first layers read one 32-feature block from memory");
    static constexpr size_t lds_bytes(int h) { return (size_t)half_frags(h) * 1024 + (size_t)half_bias(h) * 16 + 4 * 32 * sizeof(double); }
};

// Index maps of half `hf` (0: encoder, 1: decoder): for every element of the packed weight fragments ([layer][q][t][lane][e]) and of
// the bias fragments ([layer][t][g][r]) its position in the flat state-dict-order parameter vector, -1 = zero padding.
template <class N> void fragment_maps(int hf, std::vector<int> &wsrc, std::vector<int> &bsrc) {
    wsrc.assign((size_t)N::half_frags(hf) * 512, -1);
    bsrc.assign((size_t)N::half_bias(hf) * 4, -1);
    for (int l = 4 * hf; l < 4 * hf + 4; ++l) {
        const int K = N::dim(l), NN = N::dim(l + 1);
        for (int q = 0; q < N::kb(l); ++q)
            for (int t = 0; t < N::nt(l); ++t)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 8; ++e) {
                        const int i = lane & 15, g = lane >> 4;
                        const int nf = 16 * t + i, kf = N::in_feature(l, q, g, e);
                        if (nf < NN && kf >= 0)
                            wsrc[((size_t)(N::f_off(l) + q * N::nt(l) + t) * 64 + lane) * 8 + e] = N::w_off_c(l) + nf * K + kf;
                    }
        for (int t = 0; t < N::nt(l); ++t)
            for (int g = 0; g < 4; ++g)
                for (int r = 0; r < 4; ++r) {
                    const int nf = 16 * t + 4 * g + r;
                    if (nf < NN) bsrc[((size_t)N::b_off(l) + t * 4 + g) * 4 + r] = N::b_off_c(l) + nf;
                }
    }
}

// rows -> first k block: lane (j, g) reads features 8g .. 8g+7 of its row (64 contiguous bytes in fp64).  Branch-free:
// lanes beyond the last row read row 0 and lane groups / elements beyond D read feature 0 -- always inside the table, and
// never used (those k slots meet zero weights; rows beyond n are not stored and carry no loss).
// In two halves, so that the NEXT pass's rows can be requested while this pass computes: `issue` only loads (raw
// values stay in registers: 8 or 16 per batch tile), `finish` normalises, rounds and packs.  IN64 is a template parameter (a
// run-time dtype branch in front of the loads makes hipcc join the paths with conservative waits).
// IN is the bamd_dtype of the rows: float, double, or -- for the latent codes a decode reads -- binary16 / bfloat16 bit patterns,
// kept raw until `finish` widens them exactly (latent_io.hpp).
template <int IN> struct RawElem { using type = typename std::conditional<IN == BAMD_F64, double, typename std::conditional<IN == BAMD_F32, float, uint16_t>::type>::type; };
template <int D, int IN> struct RawBlock { typename RawElem<IN>::type v[8]; };
template <int D, int IN>
__device__ __forceinline__ void load_block_issue(RawBlock<D, IN> &raw, const void *x, int64_t row, bool valid, int g) {
    using T = typename RawElem<IN>::type;
    constexpr bool IN64 = IN == BAMD_F64;
    const int64_t base = (valid ? row : 0) * D;
    if (D % 8 == 0) {
        const int f0 = 8 * g < D ? 8 * g : 0;
        if (IN >= BAMD_F16) {      // eight codes: one 16-byte load
            const uint4 t = *(const uint4 *)((const uint16_t *)x + base + f0);
            const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) { raw.v[2 * e] = (T)(w[e] & 0xffffu); raw.v[2 * e + 1] = (T)(w[e] >> 16); }
        } else if (IN64) {
            const double2 *p = (const double2 *)((const double *)x + base + f0);
#pragma unroll
            for (int e = 0; e < 4; ++e) { const double2 t = p[e]; raw.v[2 * e] = (T)t.x; raw.v[2 * e + 1] = (T)t.y; }
        } else {
            const float4 *p = (const float4 *)((const float *)x + base + f0);
            const float4 t0 = p[0], t1 = p[1];
            raw.v[0] = (T)t0.x; raw.v[1] = (T)t0.y; raw.v[2] = (T)t0.z; raw.v[3] = (T)t0.w;
            raw.v[4] = (T)t1.x; raw.v[5] = (T)t1.y; raw.v[6] = (T)t1.z; raw.v[7] = (T)t1.w;
        }
    } else {   // narrow, unaligned rows (the latent codes): element loads; lane groups that hold no feature re-read feature 0
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int f = 8 * g + e < D ? 8 * g + e : 0;
            raw.v[e] = ((const T *)x)[base + f];
        }
    }
}
// the float32 values of a lane's 8 k slots: widened / normalised in float64, ONE rounding to float32, zero where the slot is padding
template <int D, int IN>
__device__ __forceinline__ void load_block_values(const RawBlock<D, IN> &raw, int g, const double *feats_lds, float (&v)[8]) {
    const int f0 = 8 * g < D ? 8 * g : 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        double d;
        if constexpr (IN >= BAMD_F16) d = (double)half_widen<IN == BAMD_BF16>(raw.v[e]); else d = (double)raw.v[e];
        const int f = D % 8 == 0 ? f0 + e : (8 * g + e < D ? 8 * g + e : 0);
        if (feats_lds) d = (d - feats_lds[f]) / feats_lds[32 + f];
        v[e] = (D % 8 == 0 || 8 * g + e < D) ? (float)d : 0.f;
    }
}
template <class V, int D, int IN>
__device__ __forceinline__ V load_block_finish(const RawBlock<D, IN> &raw, int g, const double *feats_lds) {
    float v[8];
    load_block_values<D, IN>(raw, g, feats_lds, v);
    V o;      // round to nearest even; binary16: a value beyond its range becomes +-inf (a binary16 code passes through exactly)
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (typename Elem<V>::T)v[e];
    return o;
}

// ---- epilogues of the two fp32 outputs.  Lane (j, g) holds the 4 consecutive features 16 t + 4 g + r of its row in tile t. ----
// The text of bf16_infer_kernel's two epilogues as functions, for f16x3.hip.  bf16.hip keeps its inline copy: calling these from
// there changes its register allocation (two instantiations get 8 - 12 bytes of scratch), and its kernels are held to their
// figures.  A change to either copy goes into both.
// Latent tile t of row `row` (the caller has checked the row): the output dtype test outside the element loop, a per-element feature
// test only for registers that are padding on some lane group.  dtype: the latent's bamd_dtype.
template <int Z> __device__ __forceinline__ void store_latent_tile(void *out, int dtype, int64_t row, int t, int g, const v4 &z) {
    const int64_t i0 = row * Z + 16 * t + 4 * g;
    if (dtype >= BAMD_F16) {      // 16-bit codes, rounded to nearest even
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (16 * t + 12 + r < Z || 16 * t + 4 * g + r < Z) ((uint16_t *)out)[i0 + r] = half_bits(dtype, z[r]);
    } else if (dtype) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (16 * t + 12 + r < Z || 16 * t + 4 * g + r < Z) ((double *)out)[i0 + r] = (double)z[r];
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (16 * t + 12 + r < Z || 16 * t + 4 * g + r < Z) ((float *)out)[i0 + r] = z[r];
    }
}
// Reconstruction tile t of row `row` (the caller has checked the row and 16 t + 4 g < F): un-normalise + int truncation when `renorm`
// (fl[64..]: min, fl[96..]: range), the store when `out`, and -- added to lacc element by element -- the squared error against the
// (normalised: fl[0..63]) row of xref when `xref`.
template <int F>
__device__ __forceinline__ void store_recon_tile(void *out, int out_f64, int64_t row, int t, int g, const v4 &y, bool renorm, const double *fl,
                                                   const uint8_t *imask, const void *xref, int xref_f64, bool xref_norm, double &lacc) {
    const int f0 = 16 * t + 4 * g;                   // this lane's 4 consecutive output features of tile t
    const int64_t i0 = row * F + f0;
    double d[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        d[r] = (double)y[r];
        if (renorm && f0 + r < F) {   // norm*range + min with two roundings (numpy), trunc for "int" columns (baler.py:420-435)
            d[r] = __dadd_rn(__dmul_rn(d[r], fl[96 + f0 + r]), fl[64 + f0 + r]);
            if (imask && imask[f0 + r]) d[r] = trunc(d[r]);
        }
    }
    if (out) {
        if (F % 4 == 0) {                            // 32 / 16 contiguous, aligned bytes per lane: vector stores
            if (out_f64) {
                *(double2 *)((double *)out + i0) = make_double2(d[0], d[1]);
                *(double2 *)((double *)out + i0 + 2) = make_double2(d[2], d[3]);
            } else {
                *(float4 *)((float *)out + i0) = make_float4((float)d[0], (float)d[1], (float)d[2], (float)d[3]);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (f0 + r < F) {
                    if (out_f64) ((double *)out)[i0 + r] = d[r]; else ((float *)out)[i0 + r] = (float)d[r];
                }
        }
    }
    if (xref) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (f0 + r < F) {
                double xv = xref_f64 ? ((const double *)xref)[i0 + r] : (double)((const float *)xref)[i0 + r];
                if (xref_norm) xv = (xv - fl[f0 + r]) / fl[32 + f0 + r];
                const double e = (double)y[r] - (double)(float)xv;
                lacc += e * e;
            }
    }
}

// fp32 bias fragments through their index map
__global__ void __launch_bounds__(256) pack_bias_k(const float *__restrict__ params, const int *__restrict__ src, int count,
                                                   float *__restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) dst[i] = src[i] >= 0 ? params[src[i]] : 0.f;
}

}  // namespace
}  // namespace bamd
