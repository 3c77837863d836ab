// bf16 inference mode (BAMD_MODE_BF16): encode / decode / forward_loss of AE(F, Z) on v_mfma_f32_16x16x32_bf16 -- and its
// binary16 sibling (BAMD_MODE_F16) on v_mfma_f32_16x16x32_f16: the same kernel with another element type, 11 significant bits.
//
// A THROUGHPUT mode, not the parity mode: weights and layer inputs are rounded to bfloat16 (8 significant
// bits), accumulation is fp32; outputs follow the fp64 reference to ~3e-3 relative (measured, tests), against
// 1e-7 for the fp32 MFMA mode.  Training calls on a bf16 handle run on the fp32 layer-wise kernels.
//
// Same transposed register chain as fused.hip (Y^T = W X^T, batch rows on the MFMA column, a layer's C tiles
// ARE the next layer's B operand), re-derived for the 16x16x32 shape:
//   * one MFMA contracts 32 input features; lane (j = lane & 15, g = lane >> 4) supplies 8 consecutive k slots.
//     Two output tiles (2p, 2p+1) of a layer give lane (j, g) the 8 values {16(2p) + 4g + r, 16(2p+1) + 4g + r},
//     which after LeakyReLU and ONE v_cvt_pk_bf16_f32 per pair of values are k-block p of the next layer with
//     slot (g, e) -> feature 32p + 16(e >> 2) + 4g + (e & 3); the packed weights carry that permutation.
//   * a bf16 MFMA takes 16 cycles and eats a 1-KiB A fragment: 256 B/clk/CU if every MFMA fetched its own, 4x
//     the L1 rate and 2x the LDS rate.  So (a) the whole half-model (80 / 84 fragments) is staged ONCE per
//     workgroup into LDS, and (b) every fragment read feeds kMB = 4 batch tiles (64 rows per wave per pass):
//     8 waves x 1 KiB per 4 MFMAs = 32 B/clk/CU of LDS reads.
//   * 8 waves per workgroup (2 per SIMD, <= 256 registers) share the LDS copy; the VALU work of one wave
//     (LeakyReLU + conversions: ~2 instructions per value) overlaps the MFMAs of the other.
// Encode at fp64 I/O moves 312 B/row: at these MFMA rates the kernel is HBM-bound, not MFMA-bound.
#include "bf16.hpp"
#include "bf16_net.hpp"

#include <cstdlib>

namespace bamd {
namespace {

// The 16-bit element type V (bf8 / h8), the BNet geometry and the row loaders: bf16_net.hpp
#ifndef BAMD_BF16_KMB
#define BAMD_BF16_KMB 4
#endif
#ifndef BAMD_BF16_WAVES
#define BAMD_BF16_WAVES 8
#endif
constexpr int kMB = BAMD_BF16_KMB;        // 16-row batch tiles per wave per pass
constexpr int kWaves = BAMD_BF16_WAVES;   // waves per workgroup
constexpr int kRowsPerPass = 16 * kMB;

__device__ __forceinline__ v4 mfma16(bf8 a, bf8 b, v4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ v4 mfma16(h8 a, h8 b, v4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }

// LeakyReLU as max(x, 0.01 x) with FOUR v_mul_f32, not two v_pk_mul_f32: a packed fp32 multiply does not overlap the bf16 MFMA of its
// own wave at all (tools/probe/valu_beside_mfma_probe.hip: + 17 cycles for the first one in an MFMA slot, a plain VALU instruction
// + 0.5); measured on this kernel: float32 rows 11.7 -> 12.5 G rows/s encode, float64 rows unchanged (bound by their conversions)
__device__ __forceinline__ void lrelu4(v4 &a) {
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] = __builtin_elementwise_maximum(a[r], a[r] * 0.01f);
}
template <class V> __device__ __forceinline__ V pack8(const v4 &lo, const v4 &hi) {      // round to nearest even, no clamp
    using T = typename Elem<V>::T;
    V o;
#pragma unroll
    for (int r = 0; r < 4; ++r) { o[r] = (T)lo[r]; o[4 + r] = (T)hi[r]; }
    return o;
}
// The epilogue of a tile pair: (activation and) rounding of 8 accumulators to one k-block operand.  has1 = false: `hi` is zero padding.
//   bfloat16: LeakyReLU in fp32 (lrelu4), then round -- 2.5 VALU instructions per value.
//   binary16: round FIRST, then max(h, h * slope) on packed binary16 (v_cvt_pk_f16_f32, v_pk_mul_f16, v_pk_maximum3_f16: 1.5 per
//   value); the slope is the binary16 nearest to 0.01.  BAMD_F16_FP32_LRELU=1 builds the bfloat16 order for binary16 (A/B timing
//   only: tools/bench_f16_infer.py; its results differ in the last binary16 bit).
#ifndef BAMD_F16_FP32_LRELU
#define BAMD_F16_FP32_LRELU 0
#endif
template <class V, bool ACT> __device__ __forceinline__ V act_pack(v4 &lo, v4 &hi, bool has1) {
    if constexpr (std::is_same<V, h8>::value && !BAMD_F16_FP32_LRELU) {
        V o = pack8<V>(lo, hi);
        if (ACT) o = __builtin_elementwise_maximum(o, o * (_Float16)kSlope);
        return o;
    } else {
        if (ACT) { lrelu4(lo); if (has1) lrelu4(hi); }
        return pack8<V>(lo, hi);
    }
}

// One Linear (+ LeakyReLU) layer for kMB batch tiles.  w: this layer's fragments in LDS ([q][t], 64 lanes x 16 B
// each, already offset by the lane); bias: [t][g] float4.  Output tiles are produced in pairs = k blocks of the next layer.
template <int KB, int NT, bool ACT, class V>
__device__ __forceinline__ void blayer(const V (&in)[KB][kMB], V (&out)[(NT + 1) / 2][kMB], const V *w, const v4 *bias, int g) {
#pragma unroll
    for (int p = 0; p < (NT + 1) / 2; ++p) {
        const bool has1 = 2 * p + 1 < NT;
        v4 acc0[kMB], acc1[kMB];
        const v4 b0 = bias[(2 * p) * 4 + g];
        const v4 b1 = has1 ? bias[(2 * p + 1) * 4 + g] : (v4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) { acc0[mb] = b0; acc1[mb] = b1; }
        // fragment reads one step ahead of their MFMAs (hipcc placed every ds_read_b128 right in front of its use: a full LDS
        // round trip before each group of four MFMAs, SQ_WAIT_ANY 45-51 %); sched_barrier pins the order
        V a0 = w[(2 * p) * 64], a1 = has1 ? w[(2 * p + 1) * 64] : a0;
#pragma unroll
        for (int q = 0; q < KB; ++q) {
            V n0 = a0, n1 = a1;
            if (q + 1 < KB) {
                n0 = w[((q + 1) * NT + 2 * p) * 64];
                n1 = has1 ? w[((q + 1) * NT + 2 * p + 1) * 64] : n0;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mb = 0; mb < kMB; ++mb) {
                acc0[mb] = mfma16(a0, in[q][mb], acc0[mb]);
                if (has1) acc1[mb] = mfma16(a1, in[q][mb], acc1[mb]);
            }
            __builtin_amdgcn_sched_barrier(0);
            a0 = n0;
            a1 = n1;
        }
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) out[p][mb] = act_pack<V, ACT>(acc0[mb], acc1[mb], has1);      // without a second tile acc1 = 0: zero k slots
    }
}
// Two activated layers back to back with the roles swapped: ALL output tiles of the second layer are accumulators
// (NT1 x kMB tiles) and every k block of its input is consumed as soon as the first layer has produced it.  For
// en1 -> en2 this replaces the 200-feature activation (112 registers) + a second set of accumulators by 7 x 4
// accumulator tiles: the encoder fits 256 registers without scratch.
template <int KB, int NT, int NT1, class V>
__device__ __forceinline__ void blayer_pair(const V (&in)[KB][kMB], V (&out)[(NT1 + 1) / 2][kMB], const V *w, const v4 *bias,
                                            const V *w1, const v4 *bias1, int g) {
    v4 acc[NT1][kMB];
#pragma unroll
    for (int t = 0; t < NT1; ++t) {
        const v4 b = bias1[t * 4 + g];
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) acc[t][mb] = b;
    }
#pragma unroll
    for (int p = 0; p < (NT + 1) / 2; ++p) {
        const bool has1 = 2 * p + 1 < NT;
        v4 acc0[kMB], acc1[kMB];
        const v4 b0 = bias[(2 * p) * 4 + g];
        const v4 b1 = has1 ? bias[(2 * p + 1) * 4 + g] : (v4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) { acc0[mb] = b0; acc1[mb] = b1; }
        // fragment reads one step ahead of their MFMAs (hipcc placed every ds_read_b128 right in front of its use: a full LDS
        // round trip before each group of four MFMAs, SQ_WAIT_ANY 45-51 %); sched_barrier pins the order
        V a0 = w[(2 * p) * 64], a1 = has1 ? w[(2 * p + 1) * 64] : a0;
#pragma unroll
        for (int q = 0; q < KB; ++q) {
            V n0 = a0, n1 = a1;
            if (q + 1 < KB) {
                n0 = w[((q + 1) * NT + 2 * p) * 64];
                n1 = has1 ? w[((q + 1) * NT + 2 * p + 1) * 64] : n0;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mb = 0; mb < kMB; ++mb) {
                acc0[mb] = mfma16(a0, in[q][mb], acc0[mb]);
                if (has1) acc1[mb] = mfma16(a1, in[q][mb], acc1[mb]);
            }
            __builtin_amdgcn_sched_barrier(0);
            a0 = n0;
            a1 = n1;
        }
        V blk[kMB];
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) blk[mb] = act_pack<V, true>(acc0[mb], acc1[mb], has1);
        {
            V a = w1[(p * NT1) * 64];
#pragma unroll
            for (int t = 0; t < NT1; ++t) {
                V nx = a;
                if (t + 1 < NT1) nx = w1[(p * NT1 + t + 1) * 64];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int mb = 0; mb < kMB; ++mb) acc[t][mb] = mfma16(a, blk[mb], acc[t][mb]);
                __builtin_amdgcn_sched_barrier(0);
                a = nx;
            }
        }
    }
#pragma unroll
    for (int p = 0; p < (NT1 + 1) / 2; ++p)
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) {
            if (2 * p + 1 < NT1) {
                out[p][mb] = act_pack<V, true>(acc[2 * p][mb], acc[2 * p + 1][mb], true);
            } else {
                v4 zero = {0.f, 0.f, 0.f, 0.f};
                out[p][mb] = act_pack<V, true>(acc[2 * p][mb], zero, false);
            }
        }
}

// Layer l (+ LeakyReLU) fused with the LAST layer of the half: every k block of the last layer's input is consumed
// as soon as its tile pair is finished, so the widest activation (200 features x 64 rows = 112 registers) is never
// materialised (decode kept 99 registers in scratch without this).
template <int KB, int NT, int NT2, class V>
__device__ __forceinline__ void blayer_then_last(const V (&in)[KB][kMB], v4 (&y)[NT2][kMB], const V *w, const v4 *bias,
                                                 const V *w2, const v4 *bias2, int g) {
#pragma unroll
    for (int t = 0; t < NT2; ++t) {
        const v4 b = bias2[t * 4 + g];
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) y[t][mb] = b;
    }
#pragma unroll
    for (int p = 0; p < (NT + 1) / 2; ++p) {
        const bool has1 = 2 * p + 1 < NT;
        v4 acc0[kMB], acc1[kMB];
        const v4 b0 = bias[(2 * p) * 4 + g];
        const v4 b1 = has1 ? bias[(2 * p + 1) * 4 + g] : (v4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) { acc0[mb] = b0; acc1[mb] = b1; }
        // fragment reads one step ahead of their MFMAs (hipcc placed every ds_read_b128 right in front of its use: a full LDS
        // round trip before each group of four MFMAs, SQ_WAIT_ANY 45-51 %); sched_barrier pins the order
        V a0 = w[(2 * p) * 64], a1 = has1 ? w[(2 * p + 1) * 64] : a0;
#pragma unroll
        for (int q = 0; q < KB; ++q) {
            V n0 = a0, n1 = a1;
            if (q + 1 < KB) {
                n0 = w[((q + 1) * NT + 2 * p) * 64];
                n1 = has1 ? w[((q + 1) * NT + 2 * p + 1) * 64] : n0;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mb = 0; mb < kMB; ++mb) {
                acc0[mb] = mfma16(a0, in[q][mb], acc0[mb]);
                if (has1) acc1[mb] = mfma16(a1, in[q][mb], acc1[mb]);
            }
            __builtin_amdgcn_sched_barrier(0);
            a0 = n0;
            a1 = n1;
        }
        V blk[kMB];
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) blk[mb] = act_pack<V, true>(acc0[mb], acc1[mb], has1);
        {
            V a = w2[(p * NT2) * 64];
#pragma unroll
            for (int t = 0; t < NT2; ++t) {
                V nx = a;
                if (t + 1 < NT2) nx = w2[(p * NT2 + t + 1) * 64];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int mb = 0; mb < kMB; ++mb) y[t][mb] = mfma16(a, blk[mb], y[t][mb]);
                __builtin_amdgcn_sched_barrier(0);
                a = nx;
            }
        }
    }
}

// DEC = false: z = encode(x).  DEC = true: out = decode(z) (+ un-normalise / int truncation), and with xref the
// squared-error partial of out against (normalised) xref rows (forward_loss).
// (The kernel keeps the name of its first element type; V = h8 is the BAMD_MODE_F16 sibling.)
template <class V, int F, int Z, bool DEC, int IN>
__global__ void __launch_bounds__(64 * kWaves) bf16_infer_kernel(const uint4 *__restrict__ wfrags, const v4 *__restrict__ bias_g,
                                                                 const void *__restrict__ xin, int64_t n,
                                                                 const double *__restrict__ feats, void *__restrict__ out, int out_f64,
                                                                 const uint8_t *__restrict__ imask, const void *__restrict__ xref,
                                                                 int xref_f64, const double *__restrict__ xref_feats,
                                                                 double *__restrict__ loss_part) {
    using N = BNet<F, Z>;
    constexpr int H = DEC ? 1 : 0;
    constexpr int NFR = N::half_frags(H), NB = N::half_bias(H);
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    uint4 *wl = (uint4 *)lds_raw;
    v4 *bias = (v4 *)(wl + NFR * 64);
    double *fl = (double *)(bias + NB);                 // [0..31] min, [32..63] range applied to rows READ here; [64..127]: to rows written
    __shared__ double red[64 * kWaves];
    for (int i = threadIdx.x; i < NFR * 64; i += 64 * kWaves) wl[i] = wfrags[i];
    for (int i = threadIdx.x; i < NB; i += 64 * kWaves) bias[i] = bias_g[i];
    const double *fsrc = DEC ? xref_feats : feats;     // features applied to rows READ by this kernel
    if (threadIdx.x < 128) {
        const int f = threadIdx.x & 31, which = (threadIdx.x >> 5) & 1;
        const double *src = threadIdx.x < 64 ? fsrc : (DEC ? feats : nullptr);
        fl[threadIdx.x] = (src && f < F) ? src[which * F + f] : (which ? 1.0 : 0.0);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, j = lane & 15;
    const int64_t npass = (n + kRowsPerPass - 1) / kRowsPerPass;
    double lacc = 0.0;
    int lane_off = lane;
    // The rows of the NEXT pass are requested while this pass computes (they used to be loaded at the top of the pass and used at
    // once: SQ_WAIT_ANY 45-51 %); requested BEFORE this pass's stores, so the in-order vmcnt makes the next pass wait for its
    // loads only, not for the stores to drain.
    constexpr int DIN = DEC ? Z : F;
    constexpr bool IN64 = IN == BAMD_F64;
    static_assert(DEC || IN <= BAMD_F64, "16-bit rows are latent codes: decode only");
    RawBlock<DIN, IN> raw[kMB];
    const int64_t pass0 = (int64_t)blockIdx.x * kWaves + wave, pstride = (int64_t)gridDim.x * kWaves;
    auto prefetch = [&](int64_t pass) {
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) {
            const int64_t r = pass * kRowsPerPass + 16 * mb + j;
            load_block_issue<DIN, IN>(raw[mb], xin, r, pass < npass && r < n, g);
        }
    };
    if (pass0 < npass) prefetch(pass0);
    for (int64_t pass = pass0; pass < npass; pass += pstride) {
        asm volatile("" : "+v"(lane_off));              // keep the LDS fragment reads inside the loop (LICM would spill the model)
        const V *w = (const V *)wl + lane_off;
        int64_t row[kMB];
        bool valid[kMB];
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) { row[mb] = pass * kRowsPerPass + 16 * mb + j; valid[mb] = row[mb] < n; }
        if (!DEC) {
            V a0[1][kMB], a2[N::kb(2)][kMB];
#pragma unroll
            for (int mb = 0; mb < kMB; ++mb) a0[0][mb] = load_block_finish<V, DIN, IN>(raw[mb], g, feats ? fl : nullptr);
            if (!IN64) prefetch(pass + pstride);          // float64 rows (16 registers per batch tile): after the widest layer pair
            blayer_pair<N::kb(0), N::nt(0), N::nt(1)>(a0, a2, w + N::f_off(0) * 64, bias + N::b_off(0), w + N::f_off(1) * 64,
                                                      bias + N::b_off(1), g);
            if (IN64) prefetch(pass + pstride);
            v4 z[N::nt(3)][kMB];
            blayer_then_last<N::kb(2), N::nt(2), N::nt(3)>(a2, z, w + N::f_off(2) * 64, bias + N::b_off(2), w + N::f_off(3) * 64,
                                                           bias + N::b_off(3), g);
            // one lane mask per batch tile, the output dtype test outside the element loops, a per-element feature test
            // only for registers that are padding on some lane group
#pragma unroll
            for (int mb = 0; mb < kMB; ++mb) {
                if (!valid[mb]) continue;
#pragma unroll
                for (int t = 0; t < N::nt(3); ++t) {
                    const int64_t i0 = row[mb] * Z + 16 * t + 4 * g;
                    if (out_f64 >= BAMD_F16) {      // (out_f64 is the latent's bamd_dtype here) 16-bit codes, rounded to nearest even
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (16 * t + 12 + r < Z || 16 * t + 4 * g + r < Z) ((uint16_t *)out)[i0 + r] = half_bits(out_f64, z[t][mb][r]);
                    } else if (out_f64) {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (16 * t + 12 + r < Z || 16 * t + 4 * g + r < Z) ((double *)out)[i0 + r] = (double)z[t][mb][r];
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (16 * t + 12 + r < Z || 16 * t + 4 * g + r < Z) ((float *)out)[i0 + r] = z[t][mb][r];
                    }
                }
            }
        } else {
            V a4[1][kMB], a5[N::kb(5)][kMB], a6[N::kb(6)][kMB];
#pragma unroll
            for (int mb = 0; mb < kMB; ++mb) a4[0][mb] = load_block_finish<V, DIN, IN>(raw[mb], g, nullptr);
            if (!IN64) prefetch(pass + pstride);
            blayer<N::kb(4), N::nt(4), true>(a4, a5, w + N::f_off(4) * 64, bias + N::b_off(4), g);
            blayer<N::kb(5), N::nt(5), true>(a5, a6, w + N::f_off(5) * 64, bias + N::b_off(5), g);
            v4 y[N::nt(7)][kMB];
            blayer_then_last<N::kb(6), N::nt(6), N::nt(7)>(a6, y, w + N::f_off(6) * 64, bias + N::b_off(6), w + N::f_off(7) * 64,
                                                           bias + N::b_off(7), g);
            if (IN64) prefetch(pass + pstride);           // still before this pass's stores
#pragma unroll
            for (int mb = 0; mb < kMB; ++mb)
#pragma unroll
                for (int t = 0; t < N::nt(7); ++t) {
                    const int f0 = 16 * t + 4 * g;                   // this lane's 4 consecutive output features of tile t
                    if (!valid[mb] || f0 >= F) continue;
                    const int64_t i0 = row[mb] * F + f0;
                    double d[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        d[r] = (double)y[t][mb][r];
                        if (feats && f0 + r < F) {   // norm*range + min with two roundings (numpy), trunc for "int" columns (baler.py:420-435)
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
                                if (xref_feats) xv = (xv - fl[f0 + r]) / fl[32 + f0 + r];
                                const double e = (double)y[t][mb][r] - (double)(float)xv;
                                lacc += e * e;
                            }
                    }
                }
        }
    }
    if (DEC && loss_part) {
        red[threadIdx.x] = lacc;
        __syncthreads();
        for (int st = 32 * kWaves; st > 0; st >>= 1) {
            if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
            __syncthreads();
        }
        if (threadIdx.x == 0) loss_part[blockIdx.x] = red[0];
    }
}

// params (fp32, state-dict order) -> 16-bit fragments (T: __bf16 or _Float16, round to nearest even) through precomputed index maps
// (the fp32 bias fragments: pack_bias_k, bf16_net.hpp)
template <class T>
__global__ void __launch_bounds__(256) pack16_k(const float *__restrict__ params, const int *__restrict__ src, int count,
                                                T *__restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) dst[i] = (T)(src[i] >= 0 ? params[src[i]] : 0.f);
}
// What Infer16Impl (bf16_net.hpp) asks of this file's kernels, for either element type
template <class V> struct Policy16 {
    using T = typename Elem<V>::T;
    static constexpr int rows_per_pass = kRowsPerPass, waves = kWaves;
    static constexpr size_t frag_bytes = sizeof(T);
    template <int F, int Z> static constexpr size_t lds_bytes(int half) { return BNet<F, Z>::lds_bytes(half); }
    template <int F, int Z, bool DEC, int IN> static constexpr Infer16Kernel kernel() { return bf16_infer_kernel<V, F, Z, DEC, IN>; }
    static void pack(const float *params, const int *src, int count, void *dst, hipStream_t s) {
        hipLaunchKernelGGL(pack16_k<T>, dim3((count + 255) / 256), dim3(256), 0, s, params, src, count, (T *)dst);
    }
};
Infer16State *state16(bamd_handle *h) { return (Infer16State *)h->infer16_state; }

}  // namespace

bool bf16_has_kernels(const bamd_handle *h) { return infer16_find<Policy16<bf8>>(h) != nullptr; }      // (the same shapes for both types)

// ---- the entry points of the three modes: everything mode-specific is behind the state's ops ----
int infer16_setup(bamd_handle *h) {
    const Infer16Ops *ops = h->mode == BAMD_MODE_F16X3 ? f16x3_find_ops(h)
                            : h->mode == BAMD_MODE_F16 ? infer16_find<Policy16<h8>>(h) : infer16_find<Policy16<bf8>>(h);
    if (!ops) {
        set_error("BAMD_MODE_BF16 / BAMD_MODE_F16 / BAMD_MODE_F16X3 are instantiated for the 24-column AE with LeakyReLU (latent "
                  "15/12/10/8/6/5/4/3/2) only; use BAMD_MODE_F32");
        return BAMD_ERR_UNSUPPORTED;
    }
    Infer16State *st = new Infer16State();
    st->ops = ops;
    h->infer16_state = st;
    return ops->setup(h, st);
}

void infer16_teardown(bamd_handle *h) {
    Infer16State *st = state16(h);
    if (!st) return;
    for (int i = 0; i < 2; ++i) { st->wsrc[i].release(); st->bsrc[i].release(); st->w[i].release(); st->b[i].release(); }
    st->zscratch.release();
    delete st;
    h->infer16_state = nullptr;
}

int infer16_pack(bamd_handle *h, hipStream_t s) { return state16(h)->ops->pack(h, state16(h), s); }

int infer16_encode(bamd_handle *h, const void *x, int x_dtype, int64_t n, const double *features, void *z, int z_dtype, hipStream_t s) {
    Infer16State *st = state16(h);
    return st->ops->run(h, st, false, x, x_dtype == BAMD_F64, n, features, z, z_dtype, nullptr, nullptr, 0, nullptr, nullptr, s);
}

int infer16_decode(bamd_handle *h, const void *z, int z_dtype, int64_t n, const double *features, const uint8_t *int_mask, void *out,
                   int out_dtype, hipStream_t s) {
    Infer16State *st = state16(h);
    return st->ops->run(h, st, true, z, z_dtype, n, features, out, out_dtype == BAMD_F64, int_mask, nullptr, 0, nullptr, nullptr, s);
}

int infer16_forward_loss(bamd_handle *h, const void *x, int x_dtype, int64_t n, const double *features, void *recon, int recon_dtype,
                         double *loss_sum, hipStream_t s) {
    Infer16State *st = state16(h);
    int rc = st->zscratch.ensure((size_t)n * st->ops->z_dim * sizeof(float));
    if (rc) return rc;
    rc = h->lossp.ensure(sizeof(double) * 1024);
    if (rc) return rc;
    rc = st->ops->run(h, st, false, x, x_dtype == BAMD_F64, n, features, st->zscratch.p, 0, nullptr, nullptr, 0, nullptr, nullptr, s);
    if (rc) return rc;
    return st->ops->run(h, st, true, st->zscratch.p, 0, n, nullptr, recon, recon_dtype == BAMD_F64, nullptr, x, x_dtype == BAMD_F64,
                        features, loss_sum, s);
}


namespace {
void sum_loss(const double *part, int n, double scale, double *dst, hipStream_t s) {      // behind every instantiation: see bf16_net.hpp
    hipLaunchKernelGGL(sum_partials_fixed_k<double>, dim3(1), dim3(256), 0, s, part, n, scale, dst, 0);
}
}  // namespace

}  // namespace bamd
