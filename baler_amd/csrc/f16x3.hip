// fp16x3 inference mode (BAMD_MODE_F16X3): encode / decode / forward_loss of AE(24, Z) at fp32 accuracy on v_mfma_f32_16x16x32_f16.
//
// Every fp32 operand a is SPLIT into two binary16 values, hi = binary16(a) and lo = binary16((a - hi) * 2^11), and a layer is three
// MFMA products with fp32 accumulation in two accumulators:
//     main = bias + sum hi_w * hi_h,     corr = sum (lo_w * hi_h + hi_w * lo_h),     a = main + corr * 2^-11
// (the lo * lo product, 2^-22 of the result, is not computed).  The contract is in include/baler_amd.h, its numpy text in
// tests/f16x3_ref.py, the measurements in DESIGN.md section 15.
//
// The transposed register chain, the BNet geometry, the row loaders and the store / loss epilogues are bf16.hip's (bf16_net.hpp);
// what differs:
//   * kMB = 2 batch tiles (32 rows) per wave per pass instead of 4: every output tile has two accumulators, and en1 -> en2 keeps
//     all 7 x kMB tiles of en2 live (2 x 56 registers here) beside a tile pair of en1 and the operand pairs.
//   * LDS: all hi fragments of the half-model (80 / 84 KiB) and the lo fragments of its three small layers (31 / 32 KiB).  The lo
//     fragments of the largest layer (en2: 49, de3: 52 KiB) do not fit beside them in 160 KiB; every wave reads those through
//     L1 / L2 with global loads, one fragment step ahead of the MFMAs that use them, like the LDS reads.  Plain pointer reads
//     (global_load_dwordx4), not buffer loads: the fragment address is a kernel-argument base plus a lane offset plus a compile-time
//     constant, which a global load takes as SGPR pair + VGPR + immediate; a buffer resource would add only a bounds check that a read of
//     the handle's own packed array has no use for.
//   * the epilogue of a tile pair: a = fma(corr, 2^-11, main) (the product is exact, so this is main + corr * 2^-11 rounded once),
//     LeakyReLU as max(a, 0.01f a) on the fp32 value, then the split: two conversions, one widening, one subtraction and one
//     multiplication per value -- every fp32 multiplication a plain v_mul_f32 (see mul_slope below).
#include "bf16.hpp"
#include "bf16_net.hpp"

namespace bamd {
namespace {

constexpr int kMB = 2;                    // 16-row batch tiles per wave per pass
constexpr int kWaves = 8;                 // waves per workgroup (2 per SIMD: at most 256 registers)
constexpr int kRowsPerPass = 16 * kMB;
constexpr float kLoScale = 2048.f;        // 2^11: the low part is stored scaled, so that it is a NORMAL binary16 wherever hi is
constexpr float kLoUnscale = 1.f / 2048.f;

// Where the fragments of a half-model live.  big(h): the layer whose lo fragments stay in global memory.
template <int F, int Z> struct XNet {
    using N = BNet<F, Z>;
    __host__ __device__ static constexpr int big(int h) { return h ? 6 : 1; }
    // offset (in fragments) of layer l's lo fragments inside the LDS lo area
    __host__ __device__ static constexpr int lo_off(int l) {
        int s = 0;
        for (int j = (l < 4 ? 0 : 4); j < l; ++j) s += j == big(l >= 4) ? 0 : N::frags(j);
        return s;
    }
    __host__ __device__ static constexpr int lo_lds_frags(int h) { return N::half_frags(h) - N::frags(big(h)); }
    static constexpr size_t lds_bytes(int h) {
        return (size_t)(N::half_frags(h) + lo_lds_frags(h)) * 1024 + (size_t)N::half_bias(h) * 16 + 4 * 32 * sizeof(double);
    }
    static_assert(lds_bytes(0) + 64 * kWaves * 8 <= 160 * 1024 && lds_bytes(1) + 64 * kWaves * 8 <= 160 * 1024, "one workgroup per CU");
};

__device__ __forceinline__ v4 mfma(h8 a, h8 b, v4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }

// fp32 -> (hi, lo): hi = binary16(a), nearest even, no clamp; lo = binary16((a - hi) * 2^11).  a - hi is exact in fp32 and the scale
// is a power of two.  |a| beyond 65504: hi = +-inf and lo = NaN / inf, so the row's outputs become non-finite.
// The fp32 multiplications and the subtraction of the epilogue are written as single instructions: left to itself hipcc pairs them into
// v_pk_mul_f32 / v_pk_add_f32 (77 of each per kernel), and a packed fp32 instruction does not overlap the MFMA of its own wave
// (bf16.hip, lrelu4; tools/probe/valu_beside_mfma_probe.hip).  Switching the pairing off for the file (-fno-slp-vectorize) costs 12 - 52
// bytes of scratch in 16 of the 54 kernels.  0x3c23d70a = 0.01f, 0x45000000 = 2^11.
__device__ __forceinline__ float mul_slope(float a) { float r; asm("v_mul_f32 %0, 0x3c23d70a, %1" : "=v"(r) : "v"(a)); return r; }
__device__ __forceinline__ float mul_2p11(float a) { float r; asm("v_mul_f32 %0, 0x45000000, %1" : "=v"(r) : "v"(a)); return r; }
__device__ __forceinline__ float sub_f32(float a, float b) { float r; asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
// main + corr * 2^-11, rounded once.  NOT inline assembly: this is the instruction that reads the MFMA's result registers, and hipcc
// counts the wait states an MFMA result needs before a VALU read only for instructions it knows -- an asm v_fma_f32 here read the
// last MFMAs' accumulators before they were written (encode error 5e-5 on the device).  The three helpers above read VALU results only,
// which settles the read-after-write case by construction.  Two cases it does NOT settle: the helpers WRITE a register, and hipcc
// inserts no wait states for asm either where that register is one an MFMA in flight still reads as its C operand (write after read:
// 3 wait states for this 4-pass MFMA) or still has to write (write after write: 7).  The register allocator decides whether a
// helper's result lands on such a dead accumulator; no constraint can forbid it ("=&v" and tied operands speak of the asm's own inputs
// only).  In this build the smallest distances over the 54 kernels are 6 and 10 wait states, so it is clean -- by allocation, not by
// construction: after a compiler update, recount them (tools/asm_mfma_gaps.py on the device assembly) and do
// not trust the accuracy tests alone.
__device__ __forceinline__ float fma_unscale(float corr, float main) { return __builtin_fmaf(corr, kLoUnscale, main); }
static_assert(kLoScale == 2048.f && kSlope == 0.01, "the literals above");
__device__ __forceinline__ float lrelu(float a) { return __builtin_elementwise_maximum(a, mul_slope(a)); }
__device__ __forceinline__ void split1(float a, _Float16 &hi, _Float16 &lo) {
    hi = (_Float16)a;
    lo = (_Float16)mul_2p11(sub_f32(a, (float)hi));
}
// The epilogue of a tile pair: main + corr * 2^-11, (LeakyReLU,) split into one k-block operand pair.  has1 = false: the second tile
// is zero padding.
template <bool ACT> __device__ __forceinline__ void act_split(const v4 &m0, const v4 &c0, const v4 &m1, const v4 &c1, bool has1, h8 &hi, h8 &lo) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float a = fma_unscale(c0[r], m0[r]);
        if (ACT) a = lrelu(a);
        _Float16 h, l;
        split1(a, h, l);
        hi[r] = h;
        lo[r] = l;
    }
    if (has1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float a = fma_unscale(c1[r], m1[r]);
            if (ACT) a = lrelu(a);
            _Float16 h, l;
            split1(a, h, l);
            hi[4 + r] = h;
            lo[4 + r] = l;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) { hi[4 + r] = (_Float16)0.f; lo[4 + r] = (_Float16)0.f; }
    }
}

// Output tiles (2p, 2p + 1) of one layer over all its k blocks, for kMB batch tiles: m = main accumulators (start: the bias),
// c = correction accumulators.  wh / wl: the layer's hi / lo fragments ([q][t], 64 lanes x 16 B, already offset by the lane); wl may
// point into LDS or into global memory.  Fragment reads run one k block ahead of their MFMAs and sched_barrier pins that order (as in
// bf16.hip).  Between the two MFMAs that write the same correction accumulator lie at least kMB others.
template <int KB, int NT>
__device__ __forceinline__ void tile_pair(int p, const h8 (&ih)[KB][kMB], const h8 (&il)[KB][kMB], const h8 *wh, const h8 *wl,
                                          const v4 *bias, int g, v4 (&m0)[kMB], v4 (&c0)[kMB], v4 (&m1)[kMB], v4 (&c1)[kMB]) {
    const bool has1 = 2 * p + 1 < NT;
    const v4 zero = {0.f, 0.f, 0.f, 0.f};
    const v4 b0 = bias[(2 * p) * 4 + g];
    const v4 b1 = has1 ? bias[(2 * p + 1) * 4 + g] : zero;
#pragma unroll
    for (int mb = 0; mb < kMB; ++mb) { m0[mb] = b0; m1[mb] = b1; c0[mb] = zero; c1[mb] = zero; }
    h8 ah0 = wh[(2 * p) * 64], al0 = wl[(2 * p) * 64];
    h8 ah1 = has1 ? wh[(2 * p + 1) * 64] : ah0, al1 = has1 ? wl[(2 * p + 1) * 64] : al0;
#pragma unroll
    for (int q = 0; q < KB; ++q) {
        h8 nh0 = ah0, nl0 = al0, nh1 = ah1, nl1 = al1;
        if (q + 1 < KB) {
            nh0 = wh[((q + 1) * NT + 2 * p) * 64];
            nl0 = wl[((q + 1) * NT + 2 * p) * 64];
            nh1 = has1 ? wh[((q + 1) * NT + 2 * p + 1) * 64] : nh0;
            nl1 = has1 ? wl[((q + 1) * NT + 2 * p + 1) * 64] : nl0;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) {
            m0[mb] = mfma(ah0, ih[q][mb], m0[mb]);
            c0[mb] = mfma(al0, ih[q][mb], c0[mb]);
            if (has1) {
                m1[mb] = mfma(ah1, ih[q][mb], m1[mb]);
                c1[mb] = mfma(al1, ih[q][mb], c1[mb]);
            }
        }
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) {
            c0[mb] = mfma(ah0, il[q][mb], c0[mb]);
            if (has1) c1[mb] = mfma(ah1, il[q][mb], c1[mb]);
        }
        __builtin_amdgcn_sched_barrier(0);
        ah0 = nh0; al0 = nl0; ah1 = nh1; al1 = nl1;
    }
}
// k block p of the NEXT layer (the operand pair bh / bl just produced) into all NT1 output tiles of that layer.
template <int NT1>
__device__ __forceinline__ void consume_block(int p, const h8 (&bh)[kMB], const h8 (&bl)[kMB], const h8 *wh, const h8 *wl,
                                              v4 (&m)[NT1][kMB], v4 (&c)[NT1][kMB]) {
    h8 ah = wh[(p * NT1) * 64], al = wl[(p * NT1) * 64];
#pragma unroll
    for (int t = 0; t < NT1; ++t) {
        h8 nh = ah, nl = al;
        if (t + 1 < NT1) { nh = wh[(p * NT1 + t + 1) * 64]; nl = wl[(p * NT1 + t + 1) * 64]; }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) {
            m[t][mb] = mfma(ah, bh[mb], m[t][mb]);
            c[t][mb] = mfma(al, bh[mb], c[t][mb]);
        }
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) c[t][mb] = mfma(ah, bl[mb], c[t][mb]);
        __builtin_amdgcn_sched_barrier(0);
        ah = nh;
        al = nl;
    }
}
template <int NT1> __device__ __forceinline__ void start_tiles(v4 (&m)[NT1][kMB], v4 (&c)[NT1][kMB], const v4 *bias, int g) {
    const v4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NT1; ++t) {
        const v4 b = bias[t * 4 + g];
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) { m[t][mb] = b; c[t][mb] = zero; }
    }
}

// One Linear + LeakyReLU layer: tile pairs out, each one k block of the next layer.
template <int KB, int NT>
__device__ __forceinline__ void xlayer(const h8 (&ih)[KB][kMB], const h8 (&il)[KB][kMB], h8 (&oh)[(NT + 1) / 2][kMB], h8 (&ol)[(NT + 1) / 2][kMB],
                                       const h8 *wh, const h8 *wl, const v4 *bias, int g) {
#pragma unroll
    for (int p = 0; p < (NT + 1) / 2; ++p) {
        v4 m0[kMB], c0[kMB], m1[kMB], c1[kMB];
        tile_pair<KB, NT>(p, ih, il, wh, wl, bias, g, m0, c0, m1, c1);
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) act_split<true>(m0[mb], c0[mb], m1[mb], c1[mb], 2 * p + 1 < NT, oh[p][mb], ol[p][mb]);
    }
}
// Two activated layers back to back with the roles swapped (bf16.hip, blayer_pair): every k block of the second layer's input is
// consumed as soon as the first layer has produced it, and ALL NT1 x kMB output tiles of the second layer are accumulators.
template <int KB, int NT, int NT1>
__device__ __forceinline__ void xlayer_pair(const h8 (&ih)[KB][kMB], const h8 (&il)[KB][kMB], h8 (&oh)[(NT1 + 1) / 2][kMB],
                                            h8 (&ol)[(NT1 + 1) / 2][kMB], const h8 *wh, const h8 *wl, const v4 *bias, const h8 *w1h,
                                            const h8 *w1l, const v4 *bias1, int g) {
    v4 m[NT1][kMB], c[NT1][kMB];
    start_tiles<NT1>(m, c, bias1, g);
#pragma unroll
    for (int p = 0; p < (NT + 1) / 2; ++p) {
        v4 m0[kMB], c0[kMB], m1[kMB], c1[kMB];
        tile_pair<KB, NT>(p, ih, il, wh, wl, bias, g, m0, c0, m1, c1);
        h8 bh[kMB], bl[kMB];
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) act_split<true>(m0[mb], c0[mb], m1[mb], c1[mb], 2 * p + 1 < NT, bh[mb], bl[mb]);
        consume_block<NT1>(p, bh, bl, w1h, w1l, m, c);
    }
    const v4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int p = 0; p < (NT1 + 1) / 2; ++p)
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) {
            if (2 * p + 1 < NT1) act_split<true>(m[2 * p][mb], c[2 * p][mb], m[2 * p + 1][mb], c[2 * p + 1][mb], true, oh[p][mb], ol[p][mb]);
            else act_split<true>(m[2 * p][mb], c[2 * p][mb], zero, zero, false, oh[p][mb], ol[p][mb]);
        }
}
// An activated layer fused with the LAST layer of the half (bf16.hip, blayer_then_last); y = the half's fp32 output tiles.
template <int KB, int NT, int NT2>
__device__ __forceinline__ void xlayer_then_last(const h8 (&ih)[KB][kMB], const h8 (&il)[KB][kMB], v4 (&y)[NT2][kMB], const h8 *wh,
                                                 const h8 *wl, const v4 *bias, const h8 *w2h, const h8 *w2l, const v4 *bias2, int g) {
    v4 c[NT2][kMB];
    start_tiles<NT2>(y, c, bias2, g);
#pragma unroll
    for (int p = 0; p < (NT + 1) / 2; ++p) {
        v4 m0[kMB], c0[kMB], m1[kMB], c1[kMB];
        tile_pair<KB, NT>(p, ih, il, wh, wl, bias, g, m0, c0, m1, c1);
        h8 bh[kMB], bl[kMB];
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) act_split<true>(m0[mb], c0[mb], m1[mb], c1[mb], 2 * p + 1 < NT, bh[mb], bl[mb]);
        consume_block<NT2>(p, bh, bl, w2h, w2l, y, c);
    }
#pragma unroll
    for (int t = 0; t < NT2; ++t)
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb)
#pragma unroll
            for (int r = 0; r < 4; ++r) y[t][mb][r] = fma_unscale(c[t][mb][r], y[t][mb][r]);
}

// rows -> the first operand pair: the loader's float32 values (normalised in float64, rounded once), then the split.  A binary16 or
// bfloat16 code widens exactly and has lo = 0.
template <int D, int IN>
__device__ __forceinline__ void load_block_split(const RawBlock<D, IN> &raw, int g, const double *feats_lds, h8 &hi, h8 &lo) {
    float v[8];
    load_block_values<D, IN>(raw, g, feats_lds, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        _Float16 h, l;
        split1(v[e], h, l);
        hi[e] = h;
        lo[e] = l;
    }
}

// DEC = false: z = encode(x).  DEC = true: out = decode(z) (+ un-normalise / int truncation), and with xref the squared-error partial
// of out against (normalised) xref rows (forward_loss).  Arguments, row ownership and epilogues are bf16_infer_kernel's.
// wfrags: [hi fragments of the half | lo fragments of the half], 64 x 16 B each.
template <int F, int Z, bool DEC, int IN>
__global__ void __launch_bounds__(64 * kWaves) f16x3_infer_kernel(const uint4 *__restrict__ wfrags, const v4 *__restrict__ bias_g,
                                                                  const void *__restrict__ xin, int64_t n,
                                                                  const double *__restrict__ feats, void *__restrict__ out, int out_f64,
                                                                  const uint8_t *__restrict__ imask, const void *__restrict__ xref,
                                                                  int xref_f64, const double *__restrict__ xref_feats,
                                                                  double *__restrict__ loss_part) {
    using N = BNet<F, Z>;
    using X = XNet<F, Z>;
    constexpr int H = DEC ? 1 : 0;
    constexpr int NFR = N::half_frags(H), NLO = X::lo_lds_frags(H), NB = N::half_bias(H), BIG = X::big(H);
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    uint4 *wl = (uint4 *)lds_raw;                       // hi fragments, then the lo fragments of the small layers
    v4 *bias = (v4 *)(wl + (NFR + NLO) * 64);
    double *fl = (double *)(bias + NB);                 // [0..31] min, [32..63] range applied to rows READ here; [64..127]: to rows written
    __shared__ double red[64 * kWaves];
    for (int i = threadIdx.x; i < NFR * 64; i += 64 * kWaves) wl[i] = wfrags[i];
#pragma unroll
    for (int l = 4 * H; l < 4 * H + 4; ++l) {
        if (l == BIG) continue;
        const uint4 *src = wfrags + (NFR + N::f_off(l)) * 64;
        uint4 *dst = wl + (NFR + X::lo_off(l)) * 64;
        for (int i = threadIdx.x; i < N::frags(l) * 64; i += 64 * kWaves) dst[i] = src[i];
    }
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
    constexpr int DIN = DEC ? Z : F;
    constexpr bool IN64 = IN == BAMD_F64;
    static_assert(DEC || IN <= BAMD_F64, "16-bit rows are latent codes: decode only");
    RawBlock<DIN, IN> raw[kMB];
    const int64_t pass0 = (int64_t)blockIdx.x * kWaves + wave, pstride = (int64_t)gridDim.x * kWaves;
    auto prefetch = [&](int64_t pass) {      // the NEXT pass's rows, requested before this pass's stores (bf16.hip)
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) {
            const int64_t r = pass * kRowsPerPass + 16 * mb + j;
            load_block_issue<DIN, IN>(raw[mb], xin, r, pass < npass && r < n, g);
        }
    };
    if (pass0 < npass) prefetch(pass0);
    for (int64_t pass = pass0; pass < npass; pass += pstride) {
        asm volatile("" : "+v"(lane_off));              // keep the fragment reads inside the loop (LICM would spill the model)
        const h8 *wh = (const h8 *)wl + lane_off;                              // hi fragments (LDS)
        const h8 *wo = (const h8 *)(wl + NFR * 64) + lane_off;                 // lo fragments of the small layers (LDS)
        const h8 *wg = (const h8 *)(wfrags + (NFR + N::f_off(BIG)) * 64) + lane_off;   // lo fragments of the big layer (global)
        int64_t row[kMB];
        bool valid[kMB];
#pragma unroll
        for (int mb = 0; mb < kMB; ++mb) { row[mb] = pass * kRowsPerPass + 16 * mb + j; valid[mb] = row[mb] < n; }
        if (!DEC) {
            h8 a0h[1][kMB], a0l[1][kMB], a2h[N::kb(2)][kMB], a2l[N::kb(2)][kMB];
#pragma unroll
            for (int mb = 0; mb < kMB; ++mb) load_block_split<DIN, IN>(raw[mb], g, feats ? fl : nullptr, a0h[0][mb], a0l[0][mb]);
            if (!IN64) prefetch(pass + pstride);          // float64 rows (16 registers per batch tile): after the widest layer pair
            xlayer_pair<N::kb(0), N::nt(0), N::nt(1)>(a0h, a0l, a2h, a2l, wh + N::f_off(0) * 64, wo + X::lo_off(0) * 64, bias + N::b_off(0),
                                                      wh + N::f_off(1) * 64, wg, bias + N::b_off(1), g);
            if (IN64) prefetch(pass + pstride);
            v4 z[N::nt(3)][kMB];
            xlayer_then_last<N::kb(2), N::nt(2), N::nt(3)>(a2h, a2l, z, wh + N::f_off(2) * 64, wo + X::lo_off(2) * 64, bias + N::b_off(2),
                                                           wh + N::f_off(3) * 64, wo + X::lo_off(3) * 64, bias + N::b_off(3), g);
#pragma unroll
            for (int mb = 0; mb < kMB; ++mb) {
                if (!valid[mb]) continue;
#pragma unroll
                for (int t = 0; t < N::nt(3); ++t) store_latent_tile<Z>(out, out_f64, row[mb], t, g, z[t][mb]);
            }
        } else {
            h8 a4h[1][kMB], a4l[1][kMB], a5h[N::kb(5)][kMB], a5l[N::kb(5)][kMB], a6h[N::kb(6)][kMB], a6l[N::kb(6)][kMB];
#pragma unroll
            for (int mb = 0; mb < kMB; ++mb) load_block_split<DIN, IN>(raw[mb], g, nullptr, a4h[0][mb], a4l[0][mb]);
            xlayer<N::kb(4), N::nt(4)>(a4h, a4l, a5h, a5l, wh + N::f_off(4) * 64, wo + X::lo_off(4) * 64, bias + N::b_off(4), g);
            xlayer<N::kb(5), N::nt(5)>(a5h, a5l, a6h, a6l, wh + N::f_off(5) * 64, wo + X::lo_off(5) * 64, bias + N::b_off(5), g);
            v4 y[N::nt(7)][kMB];
            xlayer_then_last<N::kb(6), N::nt(6), N::nt(7)>(a6h, a6l, y, wh + N::f_off(6) * 64, wg, bias + N::b_off(6), wh + N::f_off(7) * 64,
                                                           wo + X::lo_off(7) * 64, bias + N::b_off(7), g);
            // every code dtype after the chain (bf16.hip: float64 only): raw codes held across de3 -> de4 cost 12 - 52 bytes of scratch
            // in 16 instantiations.  Still before this pass's stores.
            prefetch(pass + pstride);
#pragma unroll
            for (int mb = 0; mb < kMB; ++mb)
#pragma unroll
                for (int t = 0; t < N::nt(7); ++t)
                    if (valid[mb] && 16 * t + 4 * g < F)
                        store_recon_tile<F>(out, out_f64, row[mb], t, g, y[t][mb], feats != nullptr, fl, imask, xref, xref_f64,
                                            xref_feats != nullptr, lacc);
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

// params (fp32, state-dict order) -> hi and lo binary16 fragments through bf16.hip's index maps
__global__ void __launch_bounds__(256) pack_split_k(const float *__restrict__ params, const int *__restrict__ src, int count,
                                                    _Float16 *__restrict__ hi, _Float16 *__restrict__ lo) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    _Float16 h, l;
    split1(src[i] >= 0 ? params[src[i]] : 0.f, h, l);
    hi[i] = h;
    lo[i] = l;
}

// What Infer16Impl (bf16_net.hpp) asks of this file's kernels
struct PolicyX3 {
    static constexpr int rows_per_pass = kRowsPerPass, waves = kWaves;
    static constexpr size_t frag_bytes = 2 * sizeof(_Float16);      // [hi | lo]
    template <int F, int Z> static constexpr size_t lds_bytes(int half) { return XNet<F, Z>::lds_bytes(half); }
    template <int F, int Z, bool DEC, int IN> static constexpr Infer16Kernel kernel() { return f16x3_infer_kernel<F, Z, DEC, IN>; }
    static void pack(const float *params, const int *src, int count, void *dst, hipStream_t s) {
        hipLaunchKernelGGL(pack_split_k, dim3((count + 255) / 256), dim3(256), 0, s, params, src, count, (_Float16 *)dst, (_Float16 *)dst + count);
    }
};

}  // namespace

const Infer16Ops *f16x3_find_ops(const bamd_handle *h) { return infer16_find<PolicyX3>(h); }


namespace {
void sum_loss(const double *part, int n, double scale, double *dst, hipStream_t s) {      // behind every instantiation: see bf16_net.hpp
    hipLaunchKernelGGL(sum_partials_fixed_k<double>, dim3(1), dim3(256), 0, s, part, n, scale, dst, 0);
}
}  // namespace

}  // namespace bamd
