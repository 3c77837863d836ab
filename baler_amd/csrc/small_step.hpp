// What the fp32 (fused.hip) and the fp64 (fused64.hip, fused64q.hip) small-batch training steps share, written once: the geometry of
// AE(F, Z), the [16-row block][slot][16 rows] images, the 15-GEMM fragment sequence of a chain wave, the parts of the one-tile
// weight-gradient kernels that do not depend on the MFMA's C/D map, and the host maps.  Everything is a template on the caller's element,
// vector and stream types; a translation unit includes this BEFORE it defines its own v4 / d4, WStream, frag_rt and mfma (anonymous
// namespace: nothing here has linkage), and the shared device code calls frag_rt(ws, idx) unqualified, so each file's own loader is
// found at instantiation.  No function here asks which precision called it.
// What stays per file, and why: the chain kernel bodies (C/D row 4 g + r against g + 4 r, buffer stores against plain stores, two
// interleaved accumulators against one), lat4_chain_kernel against chain64q_kernel (4x4x1 against 4x4x4), ISeq of fused64_infer.hpp
// (inference: forward GEMMs of a sub-range only) and bf16_train.hip's stream (another fragment size and order) differ in more than the type.
#pragma once
#include <utility>
#include <vector>

#include "bamd_internal.hpp"

namespace bamd {
namespace {

__host__ __device__ constexpr int tiles(int d) { return (d + 15) / 16; }
// MFMA steps needed for feature tile t of a dimension d (4 for full tiles, ceil(valid/4) for the last)
__host__ __device__ constexpr int tile_steps(int d, int t) { return d - 16 * t >= 16 ? 4 : (d - 16 * t + 3) / 4; }

// ---- compile-time description of AE(F, Z): 8 layers F-200-100-50-Z-50-100-200-F -----------------------
// The head of the packed buffer in vector units (float4 = 16 bytes / d4 = 32 bytes; a fragment = 64 lanes x one vector):
//   [ Wf(0..7) | Wb(7,6,..,1) | bias frags | the precision's own regions (Net / Net64) ]
// Wf = forward fragments, Wb = transposed fragments for the input-gradient chain, packed in the order the kernels consume
// them so that every kernel walks ONE linear stream.
template <int F, int Z> struct NetGeom {
    static constexpr int L = 8;
    __host__ __device__ static constexpr int dim(int i) {
        return i == 0 ? F : i == 1 ? 200 : i == 2 ? 100 : i == 3 ? 50 : i == 4 ? Z : i == 5 ? 50 : i == 6 ? 100 : i == 7 ? 200 : F;
    }
    __host__ __device__ static constexpr bool act(int l) { return !(l == 3 || l == 7); }
    __host__ __device__ static constexpr int wcount(int l) { return tiles(dim(l)) * tiles(dim(l + 1)) * 64; }
    __host__ __device__ static constexpr int wf_off(int l) { int s = 0; for (int j = 0; j < l; ++j) s += wcount(j); return s; }
    __host__ __device__ static constexpr int wb_off(int l) { int s = wf_off(L); for (int j = L - 1; j > l; --j) s += wcount(j); return s; }
    __host__ __device__ static constexpr int bf_off(int l) { int s = wb_off(0); for (int j = 0; j < l; ++j) s += tiles(dim(j + 1)) * 4; return s; }
    // weight-gradient tiles of layer l: tiles(N) x tiles(K + 1) (the extra slot carries db)
    __host__ __device__ static constexpr int dw_tiles(int l) { return tiles(dim(l + 1)) * tiles(dim(l) + 1); }
    __host__ __device__ static constexpr int slab_off(int l) { int s = 0; for (int j = 0; j < l; ++j) s += dw_tiles(j); return s; }
    // canonical (state-dict) offsets
    __host__ __device__ static constexpr int w_off(int l) { int s = 0; for (int j = 0; j < l; ++j) s += dim(j + 1) * dim(j) + dim(j + 1); return s; }
    __host__ __device__ static constexpr int b_off(int l) { return w_off(l) + dim(l + 1) * dim(l); }
    __host__ __device__ static constexpr int nparams() { return w_off(L); }
};

// global images of the chain: [16-row block][slot][16 rows]; X_l has 16 tiles(dim(l) + 1) slots (with the ones slot that carries db),
// dZ_l 16 tiles(dim(l + 1)); offsets in slots, `stride` elements per slot (= rows per block), `size` elements per block
constexpr int kImgStride = 16;   // (for the publishing helpers, which know a slot and not the net)
template <class N> struct StepImages {
    __host__ __device__ static constexpr int x_rows(int l) { return 16 * tiles(N::dim(l) + 1); }
    __host__ __device__ static constexpr int z_rows(int l) { return 16 * tiles(N::dim(l + 1)); }
    __host__ __device__ static constexpr int x_off(int l) { int s = 0; for (int j = 0; j < l; ++j) s += x_rows(j); return s; }
    __host__ __device__ static constexpr int z_off(int l) { int s = x_off(N::L); for (int j = 0; j < l; ++j) s += z_rows(j); return s; }
    static constexpr int stride = kImgStride;
    static constexpr int size = z_off(N::L) * stride;
};

// The 15 chain GEMMs of one training step as ONE fragment sequence per wave (forward layers 0..7, then the
// transposed fragments of layers 7..1): a register ring of D fragments runs D fragments AHEAD of the MFMAs across
// layer boundaries, one refill per consumed fragment, so the loads are spread between the MFMAs.  (Requesting whole
// layers at once stalls the wave: a 1-KiB fragment load occupies the CU's 64 B/clk L1 path for 16 cycles and a
// wave issues in order, so 28 loads x 4 waves in a row = 1800 cycles before the first MFMA of the layer.)
// W = waves that split a layer's output tiles (tile t -> wave t mod W; 1: a wave owns all tiles of its rows).
template <class N, int W, int D_> struct ChainSeq {
    static constexpr int D = D_, Wv = W, NG = 15;
    __host__ __device__ static constexpr int layer(int g) { return g < 8 ? g : 15 - g; }              // 0..7, 7..1
    __host__ __device__ static constexpr int kd(int g) { return g < 8 ? N::dim(g) : N::dim(layer(g) + 1); }
    __host__ __device__ static constexpr int nt(int g) { return tiles(g < 8 ? N::dim(g + 1) : N::dim(layer(g))); }
    __host__ __device__ static constexpr int base(int g) { return (g < 8 ? N::wf_off(g) : N::wb_off(layer(g))) / 64; }
    __host__ __device__ static constexpr int nl(int g) { return (nt(g) + W - 1) / W; }
    __host__ __device__ static constexpr int nf(int g) { return tiles(kd(g)) * nl(g); }
    __host__ __device__ static constexpr int start(int g) { int s = 0; for (int j = 0; j < g; ++j) s += nf(j); return s; }
    static constexpr int total = start(NG);
    __host__ __device__ static constexpr int gemm_of(int G) { int g = 0; for (int j = 1; j < NG; ++j) if (G >= start(j)) g = j; return g; }
};
// (every index below is a template constant: with loop variables hipcc left the ring in scratch memory)
template <class SQ, int G, class V, class WS>
__device__ __forceinline__ void seq_issue(V (&slot)[SQ::D], const WS &ws, int wave) {
    if constexpr (G < SQ::total) {
        constexpr int g = SQ::gemm_of(G), f = G - SQ::start(g), NL = SQ::nl(g), q = f / NL, i = f % NL, NT = SQ::nt(g);
        int t = wave + SQ::Wv * i;
        t = t < NT ? t : NT - 1;
        slot[G % SQ::D] = frag_rt(ws, SQ::base(g) + q * NT + t);
    }
}
template <class SQ, class V, class WS, int... G>
__device__ __forceinline__ void seq_prologue(V (&slot)[SQ::D], const WS &ws, int wave, std::integer_sequence<int, G...>) {
    (seq_issue<SQ, G>(slot, ws, wave), ...);
    __builtin_amdgcn_sched_barrier(0);
}
// all tiles of a layer from the LDS exchange buffer (C layout: tile t at xch[64 t + lane])
template <int NT, class V> __device__ __forceinline__ void collect(const V *xch, V (&all)[NT], int lane) {
#pragma unroll
    for (int t = 0; t < NT; ++t) all[t] = xch[t * 64 + lane];
}

// ---- the one-tile weight-gradient kernels (lat2_dw_kernel, dw64_kernel): one workgroup per [dW | db] tile, + one for the loss ------------
enum { DW_WRITE = 0, DW_ADAM = 1, DW_ACCUM = 2 };   // grads = g | Adam on g (+ grads = g) | grads += g (fp32 only)
// grid = 8 x ceil((dW tiles + 1) / 8).  Workgroups are dealt to the 8 XCDs round-robin and every XCD has its own L2, so XCD c takes the
// CONTIGUOUS tile range [c * per, (c + 1) * per): neighbouring tiles share their X / dZ image slices, each slice then crosses the
// fabric into (about) one L2 instead of eight.  Tile T = N::slab_off(N::L) is the loss; tiles beyond it do nothing.
template <class N> constexpr int dw_tile_grid() { return 8 * ((N::slab_off(N::L) + 1 + 7) / 8); }
template <class N> __device__ __forceinline__ int dw_tile_of_block() {
    constexpr int kPerXcd = (N::slab_off(N::L) + 1 + 7) / 8;
    return (blockIdx.x & 7) * kPerXcd + (blockIdx.x >> 3);
}
// the loss tile: fixed-order sum of the chain's per-block partials, / C.  256 strided sums, then a fixed tree (ONE thread adding
// 32 .. 128 partials one dependent L2 round trip after the other was the longest workgroup of the fp32 kernel: 6.5 us of its 6.5-9 us).
// np = index of the loss slot = the model's parameter count, inv_c = 1 / columns; sh: 256 doubles of LDS
template <int MODE, class T>
__device__ __forceinline__ void dw_loss_tile(const double *__restrict__ loss_part, int nloss, double inv_c, T *__restrict__ grads, int np,
                                             double *loss_accum, double *sh) {
    const double s = block_sum_fixed(loss_part, nloss, sh);
    if (threadIdx.x == 0) {
        const T gl = (T)(s * inv_c);
        if (grads) grads[np] = MODE == DW_ACCUM ? grads[np] + gl : gl;
        if (MODE == DW_ADAM && loss_accum) *loss_accum += (double)gl;
    }
}
// tile -> output tile nt x input tile kt (with the ones slot) of its layer, and that layer's first X / dZ image slots.  (dw64_kernel
// calls it; lat2_dw_kernel keeps the same lines as its own text, for a measured reason given there.)
struct DwTile { int kt, nt, xo, zo; };
template <class N> __device__ __forceinline__ DwTile dw_tile_decode(int tile) {
    using IM = StepImages<N>;
    int l = 0;
#pragma unroll
    for (int j = 1; j < N::L; ++j) if (tile >= N::slab_off(j)) l = j;
    int nt_count = tiles(N::dim(1)), soff = 0, xo = IM::x_off(0), zo = IM::z_off(0);
#pragma unroll
    for (int j = 1; j < N::L; ++j)
        if (l == j) { nt_count = tiles(N::dim(j + 1)); soff = N::slab_off(j); xo = IM::x_off(j); zo = IM::z_off(j); }
    const int idx = tile - soff, kt = idx / nt_count, nt = idx - kt * nt_count;
    return DwTile{kt, nt, xo, zo};
}
// element e of a tile from the four waves' accumulators in LDS ([wave][64 lanes][4]), in wave order
template <class T> __device__ __forceinline__ T dw_sum4(const T *rf, int e) { return ((rf[e] + rf[256 + e]) + rf[512 + e]) + rf[768 + e]; }
// the first four packed copies of a parameter (scatter entries [s0, s1)), requested ahead of the reduction; -1: none.  `sc` is declared
// in the kernel (an array declared inside an inlined function carries lifetime markers that cost scratch: profiles/dw_short_one_text.txt)
template <class T> __device__ __forceinline__ void dw_adam_slots(const AdamTargets<T> &ad, int s0, int s1, int (&sc)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) if (s0 + k < s1) sc[k] = ad.sc_idx[s0 + k];
}
// Adam on parameter p (gradient g, state pm / pv / pp loaded by the caller ahead of its image loop) and the refresh of its packed copies
template <class T>
__device__ __forceinline__ void dw_adam_finish(const AdamTargets<T> &ad, int p, T g, T pm, T pv, T pp, const int (&sc)[4], int s0, int s1) {
    const T pn = adam_update(ad.s, g, pm, pv, pp);
    ad.m[p] = pm;
    ad.v[p] = pv;
    ad.params[p] = pn;
    if (ad.pcopy) ad.pcopy[p] = pn;
#pragma unroll
    for (int k = 0; k < 4; ++k) if (sc[k] >= 0) ad.packed[sc[k]] = pn;
    for (int k = s0 + 4; k < s1; ++k) ad.packed[ad.sc_idx[k]] = pn;
}

// ---- host maps ------------------------------------------------------------------------------------------------------------------------
// src[packed element] = canonical parameter it copies (-1: zero) for the forward, transposed and bias fragments of every layer.
// Geometry (tiles, fragment order) from the instantiated N; which slots hold a parameter, and its canonical index, from the handle's
// REAL dimensions (identical for an exact instantiation; a class instantiation's slots beyond the real width map to nothing).
// FM, the precision's slot -> feature map (-1 = padding): row(d, t, i) = feature on A-operand row i of tile t, reg(d, t, g, r) =
// feature held by register r of tile t on lane group g (the MFMA's C/D map, hence the next layer's k order).
template <class N, class FM>
void fill_fragment_maps(std::vector<int> &src, const bamd_handle *h, FM fm) {
    for (int l = 0; l < N::L; ++l) {
        const int K = N::dim(l), NN = N::dim(l + 1), KT = tiles(K), NT = tiles(NN), Kr = h->dims[l], NNr = h->dims[l + 1];
        const int wo = (int)h->w_off[l], bo = (int)h->b_off[l];
        // forward fragment (q, t): lane (i, g) component r = W[row(t, i)][reg(q, g, r)]
        for (int q = 0; q < KT; ++q)
            for (int t = 0; t < NT; ++t)
                for (int lane = 0; lane < 64; ++lane)
                    for (int r = 0; r < 4; ++r) {
                        const int n = fm.row(NN, t, lane & 15), k = fm.reg(K, q, lane >> 4, r);
                        if (n >= 0 && k >= 0 && n < NNr && k < Kr) src[((size_t)N::wf_off(l) + (q * NT + t) * 64 + lane) * 4 + r] = wo + n * Kr + k;
                    }
        // backward fragment (tq, tk), layers 1..7: lane (i, g) component r = W[reg(tq, g, r)][row(tk, i)]
        for (int tq = 0; tq < NT && l >= 1; ++tq)
            for (int tk = 0; tk < KT; ++tk)
                for (int lane = 0; lane < 64; ++lane)
                    for (int r = 0; r < 4; ++r) {
                        const int n = fm.reg(NN, tq, lane >> 4, r), k = fm.row(K, tk, lane & 15);
                        if (n >= 0 && k >= 0 && n < NNr && k < Kr) src[((size_t)N::wb_off(l) + (tq * KT + tk) * 64 + lane) * 4 + r] = wo + n * Kr + k;
                    }
        // bias fragment (t, g) component r = b[reg(t, g, r)]
        for (int t = 0; t < NT; ++t)
            for (int g = 0; g < 4; ++g)
                for (int r = 0; r < 4; ++r) {
                    const int n = fm.reg(NN, t, g, r);
                    if (n >= 0 && n < NNr) src[((size_t)N::bf_off(l) + t * 4 + g) * 4 + r] = bo + n;
                }
    }
}
// inverse of the pack map, as CSR: the packed positions that hold a copy of parameter p are idx[off[p] .. off[p + 1]), ascending
inline void invert_pack_map(const std::vector<int> &src, int nparams, std::vector<int> &off, std::vector<int> &idx) {
    off.assign((size_t)nparams + 1, 0);
    for (int v : src) if (v >= 0) off[v + 1]++;
    for (int p = 0; p < nparams; ++p) off[p + 1] += off[p];
    idx.resize(off[nparams]);
    std::vector<int> cur(off.begin(), off.end() - 1);
    for (size_t i = 0; i < src.size(); ++i) if (src[i] >= 0) idx[cur[src[i]]++] = (int)i;
}

}  // namespace
}  // namespace bamd
