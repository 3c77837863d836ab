// What the 16-bit inference kernels share (bf16.hip: bfloat16 and binary16; f16x3.hip: split binary16): the operand vector types,
// the BNet geometry of AE(F, Z) on the 16x16x32 MFMA with its fragment index maps, the row loaders, the bias pack kernel, the
// store / loss epilogues of the two fp32 outputs (latent, reconstruction) as functions, and -- at the end -- the host side of a mode:
// its state, and setup / launch / pack written once over a policy that each file defines beside its kernels.
// Device code and the host templates in an anonymous namespace: every translation unit has its own copy.
#pragma once
#include "bamd_internal.hpp"

#include <type_traits>
#include <vector>

namespace bamd {

// The state of a bf16 / f16 / fp16x3 handle (h->infer16_state) and the calls of its instantiation.  The entry points (bf16.hpp) work
// through these alone; which policy filled `ops` is decided once, at setup, by h->mode.
struct Infer16Ops;
struct Infer16State {
    const Infer16Ops *ops = nullptr;
    DevBuf wsrc[2], bsrc[2];     // index maps (encoder half, decoder half)
    DevBuf w[2], b[2];           // packed 16-bit fragments (fp16x3: [hi | lo]) / fp32 bias fragments
    DevBuf zscratch;             // latent codes between the two launches of forward_loss
    int wcount[2] = {0, 0}, bcount[2] = {0, 0};
    int grid = 256;
};
struct Infer16Ops {
    int (*setup)(bamd_handle *, Infer16State *);
    // One launch of half `dec`.  in_dtype / out_dtype are bamd_dtype codes: 16-bit for the latent side of a decode / an encode.
    // loss_sum (decode with xref): per-workgroup partials into h->lossp (the caller has sized it), summed by a second launch.
    int (*run)(bamd_handle *, Infer16State *, bool dec, const void *xin, int in_dtype, int64_t n, const double *feats, void *out,
               int out_dtype, const uint8_t *imask, const void *xref, int xref_f64, const double *xref_feats, double *loss_sum,
               hipStream_t s);
    int (*pack)(bamd_handle *, Infer16State *, hipStream_t s);      // h->params (fp32) -> both halves' fragments
    int z_dim;
};

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

// ---- the host side of a mode, over a policy P that states what differs between the kernel families: ----
//   P::rows_per_pass, P::waves                  16 kMB and kWaves of the file's kernels
//   P::frag_bytes                               bytes of packed fragment per index-map entry
//   P::lds_bytes<F, Z>(half)                    dynamic LDS of a launch
//   P::kernel<F, Z, DEC, IN>()                  the kernel (every family has the signature below)
//   P::pack(params, src, count, dst, s)         launches the weight pack of one half
using Infer16Kernel = void (*)(const uint4 *wfrags, const v4 *bias, const void *xin, int64_t n, const double *feats, void *out, int out_dtype,
                               const uint8_t *imask, const void *xref, int xref_f64, const double *xref_feats, double *loss_part);

// *dst = scale * the sum of n partials: one launch of the file's sum_partials_fixed_k<double>.  Each file DEFINES this behind its
// instantiations: hipcc emits a template kernel where host code first names it, and named from run() below this kernel would leave the
// end of the file's code object for a place between the inference kernels.  Here the code objects keep the order they had (f16x3.hip's
// assembly is unchanged to the byte); forward_loss at 64 rows measured + 0.06 .. 0.11 us with the launch in run() and - 0.12 .. + 0.07 us
// this way, against 20 - 27 us (profiles/r9_infer16_one_host_side.txt)
void sum_loss(const double *part, int n, double scale, double *dst, hipStream_t s);

template <class P> int pack_halves(bamd_handle *h, Infer16State *st, hipStream_t s) {
    for (int hf = 0; hf < 2; ++hf) {
        P::pack((const float *)h->params.p, (const int *)st->wsrc[hf].p, st->wcount[hf], st->w[hf].p, s);
        hipLaunchKernelGGL(pack_bias_k, dim3((st->bcount[hf] + 255) / 256), dim3(256), 0, s, (const float *)h->params.p,
                           (const int *)st->bsrc[hf].p, st->bcount[hf], (float *)st->b[hf].p);
    }
    BAMD_HIP(hipGetLastError());
    return BAMD_OK;
}
template <class P, int F, int Z> struct Infer16Impl {
    using N = BNet<F, Z>;
    static bool matches(const bamd_handle *h) {
        if (h->L != 8) return false;
        for (int i = 0; i <= 8; ++i)
            if (h->dims[i] != N::dim(i)) return false;
        return true;
    }
    template <bool D_, int I_> static int allow_lds() {
        BAMD_HIP(hipFuncSetAttribute((const void *)P::template kernel<F, Z, D_, I_>(), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)P::template lds_bytes<F, Z>(D_ ? 1 : 0)));
        return BAMD_OK;
    }
    static int setup(bamd_handle *h, Infer16State *st) {
        for (int hf = 0; hf < 2; ++hf) {
            std::vector<int> wsrc, bsrc;
            fragment_maps<N>(hf, wsrc, bsrc);
            st->wcount[hf] = (int)wsrc.size();
            st->bcount[hf] = (int)bsrc.size();
            int rc = st->wsrc[hf].ensure(wsrc.size() * sizeof(int));
            if (rc) return rc;
            rc = st->bsrc[hf].ensure(bsrc.size() * sizeof(int));
            if (rc) return rc;
            rc = st->w[hf].ensure(wsrc.size() * P::frag_bytes);
            if (rc) return rc;
            rc = st->b[hf].ensure(bsrc.size() * sizeof(float));
            if (rc) return rc;
            BAMD_HIP(hipMemcpy(st->wsrc[hf].p, wsrc.data(), wsrc.size() * sizeof(int), hipMemcpyHostToDevice));
            BAMD_HIP(hipMemcpy(st->bsrc[hf].p, bsrc.data(), bsrc.size() * sizeof(int), hipMemcpyHostToDevice));
        }
        int rc = allow_lds<false, BAMD_F32>();
        if (!rc) rc = allow_lds<false, BAMD_F64>();
        if (!rc) rc = allow_lds<true, BAMD_F32>();
        if (!rc) rc = allow_lds<true, BAMD_F64>();
        if (!rc) rc = allow_lds<true, BAMD_F16>();
        if (!rc) rc = allow_lds<true, BAMD_BF16>();
        return rc;
    }
    static int run(bamd_handle *h, Infer16State *st, bool dec, const void *xin, int in_dtype, int64_t n, const double *feats, void *out,
                   int out_dtype, const uint8_t *imask, const void *xref, int xref_f64, const double *xref_feats, double *loss_sum,
                   hipStream_t s) {
        const int64_t npass = (n + P::rows_per_pass - 1) / P::rows_per_pass;
        int64_t wg = (npass + P::waves - 1) / P::waves;
        const int grid = (int)(wg < 1 ? 1 : (wg > st->grid ? st->grid : wg));
        double *loss_part = loss_sum ? (double *)h->lossp.p : nullptr;
        auto go = [&](auto decv, auto inv) {
            constexpr bool D_ = decltype(decv)::value;
            constexpr int I_ = decltype(inv)::value;
            constexpr Infer16Kernel kernel = P::template kernel<F, Z, D_, I_>();
            constexpr size_t lds = P::template lds_bytes<F, Z>(D_ ? 1 : 0);
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * P::waves), lds, s,
                               (const uint4 *)st->w[D_ ? 1 : 0].p, (const v4 *)st->b[D_ ? 1 : 0].p, xin, n, feats, out, out_dtype, imask, xref,
                               xref_f64, xref_feats, loss_part);
        };
        using i32 = std::integral_constant<int, BAMD_F32>;
        using i64 = std::integral_constant<int, BAMD_F64>;
        if (dec && in_dtype == BAMD_F16) go(std::true_type(), std::integral_constant<int, BAMD_F16>());
        else if (dec && in_dtype == BAMD_BF16) go(std::true_type(), std::integral_constant<int, BAMD_BF16>());
        else if (dec && in_dtype) go(std::true_type(), i64());
        else if (dec) go(std::true_type(), i32());
        else if (in_dtype) go(std::false_type(), i64());
        else go(std::false_type(), i32());
        if (loss_sum) sum_loss(loss_part, grid, 1.0 / F, loss_sum, s);
        BAMD_HIP(hipGetLastError());
        return BAMD_OK;
    }
    static const Infer16Ops *ops() {
        static const Infer16Ops o = {setup, run, pack_halves<P>, Z};
        return &o;
    }
};
// The instantiation of P's kernels for this handle's shape, or null: AE(24, Z) with LeakyReLU at the fused latent sizes
template <class P> const Infer16Ops *infer16_find(const bamd_handle *h) {
    if (!h->leaky()) return nullptr;
#define BAMD_INFER16(Z_) if (Infer16Impl<P, 24, Z_>::matches(h)) return Infer16Impl<P, 24, Z_>::ops();
    BAMD_AE24_LATENTS(BAMD_INFER16)
#undef BAMD_INFER16
    return nullptr;
}

}  // namespace
}  // namespace bamd
