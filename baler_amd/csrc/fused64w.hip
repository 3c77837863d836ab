// fp64 inference of WIDE tables (128 .. 4096 columns, latent <= 63) in one launch: encode / decode / forward + loss of AE(n, z) with the
// reference's hidden widths on v_mfma_f64_16x16x4_f64, n and z as kernel arguments.  Until this file such handles ran layer by layer
// (generic.hip: every activation through HBM).  The structure is the fp32 wide class's (fused.hip ImplWide) in the f64
// accumulator layout of fused64_net.hpp:
//   * a wave owns 16 rows; a workgroup = 4 waves = 64 rows, persistent over 64-row groups;
//   * en1 is STREAMED: the wave keeps the 13 tiles of the 200-feature side in accumulators and walks the table 16 columns at a time (one
//     chunk = 13 fragments = 26 KiB = 52 MFMAs per wave); the four waves share a chunk's fragments through a double-buffered LDS stage
//     with a fixed load lead (chunk c + 2 travels global -> registers while chunk c is multiplied, chunk c + 1 registers -> the other
//     buffer in the middle of chunk c: one barrier per chunk);
//   * de4 mirrors it: per 16-column output chunk ONE tile from the 200-feature activation in registers (four accumulators, added in a
//     fixed order), finished and stored by the epilogue (bias, loss against the re-read input chunk, or un-normalisation);
//   * the six narrow layers between them are the register chain of fused64_infer.hpp (ISeq / ilayer, a fragment ring that wraps across
//     row groups) over the Net64<15, ZC> layout of the packed buffer (fused64w.hpp);
//   * the last chunk is partial when n is no multiple of 16: its padding slots read column 0 of the row (inside the row), are set to
//     zero and meet zero weights; nothing beyond column n - 1 is loaded or stored.
// Every sum of a row has a fixed order that depends on neither the grid nor the row's place in it, so results are bitwise repeatable
// and independent of BALER_AMD_F64_WIDE_WGS; the loss partials (one per workgroup) are added in index order.
#include "fused64_infer.hpp"
#include "fused64w.hpp"

namespace bamd {
namespace {

constexpr int kRing64W = 4;      // fragments of the narrow layers in flight per wave

// chunk (832 d4) global -> registers -> LDS, 256 threads: three full rounds and a quarter one
__device__ __forceinline__ void stage_load(d4 (&st)[4], const d4 *__restrict__ src) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = (int)threadIdx.x + 256 * i;
        st[i] = src[idx < kWide64ChunkD4 ? idx : 0];
    }
}
// A chunk in LDS: the lanes' first 16 bytes of every fragment, then their second 16 bytes (two planes), so that each ds_read_b128 of a wave
// covers 1 KiB without a gap (a lane's 32 bytes side by side put two lanes of a read's 16-lane group on the same banks)
typedef double d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void stage_store(d2 *dst, const d4 (&st)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = (int)threadIdx.x + 256 * i;
        if (idx < kWide64ChunkD4) {
            dst[idx] = (d2){st[i][0], st[i][1]};
            dst[kWide64ChunkD4 + idx] = (d2){st[i][2], st[i][3]};
        }
    }
}
// The 13 fragments of a chunk are multiplied in groups of 4, 3, 3 and 3 whose MFMAs interleave step by step: consecutive MFMAs of a wave
// then write different accumulators, and de4's single output tile has four to spread its 52 steps over.  (Measured on the 2,500-column
// model: en1 with four dependent steps per tile in a row ran within 5 % of this order -- one wave per SIMD issues an f64 MFMA every
// ~115 cycles either way)
__host__ __device__ constexpr int grp_at(int g) { return g == 0 ? 0 : 1 + 3 * g; }      // 0, 4, 7, 10, 13
template <int G>
__device__ __forceinline__ void frags_read(d4 (&f)[4], const d2 *buf, int lane) {
#pragma unroll
    for (int i = 0; i < grp_at(G + 1) - grp_at(G); ++i) {
        const d2 lo = buf[(grp_at(G) + i) * 64 + lane], hi = buf[kWide64ChunkD4 + (grp_at(G) + i) * 64 + lane];
        f[i] = (d4){lo[0], lo[1], hi[0], hi[1]};
    }
}

// Column chunk c of this lane's row as the B operand of the chunk's four MFMA steps: component r = column 16 c + 4 r + lg, normalised as
// (x - min) / range.  In two halves, so that the loads travel while the previous chunk is multiplied: the first half is loads only, with no
// branch on the call's options around any of them (a value merged behind a branch is waited for there, in front of the MFMAs) -- the row
// type is a template parameter, and `mnrg` is always a readable [min | range] array (without `features`: any 2 fr doubles; not used)
template <bool IN64> struct RawChunk64 {
    std::conditional_t<IN64, double, float> x[4];
    d4 mn, rg;
};
template <bool IN64>
__device__ __forceinline__ void chunk_request(RawChunk64<IN64> &raw, const void *__restrict__ xin, int64_t rbase, int c, int lg, int fr,
                                              const double *__restrict__ mnrg) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int f = 16 * c + 4 * r + lg;
        const int fc = f < fr ? f : 0;                                // padding slots read column 0 of the row (finite, meets zero weights)
        raw.x[r] = ((const std::conditional_t<IN64, double, float> *)xin)[rbase + fc];
        raw.mn[r] = mnrg[fc];
        raw.rg[r] = mnrg[fr + fc];
    }
}
template <bool IN64>
__device__ __forceinline__ d4 chunk_finish(const RawChunk64<IN64> &raw, int c, int lg, int fr, bool normalise) {
    d4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double x = (double)raw.x[r];
        if (normalise) x = (x - raw.mn[r]) / raw.rg[r];
        v[r] = 16 * c + 4 * r + lg < fr ? x : 0.0;
    }
    return v;
}

// en1, one chunk: the 13 accumulator tiles += fragment (c, t) x the chunk's columns, group by group; the next group's fragments leave LDS
// while this one multiplies.  mid(): the caller's work between the second and the third group (the stage's store of the next chunk)
template <int G, class Mid>
__device__ __forceinline__ void en1_group(d4 (&acc)[kWide64Frags], d4 (&f)[4], const d2 *buf, const d4 xb, int lane, Mid mid) {
    constexpr int t0 = grp_at(G), cnt = grp_at(G + 1) - t0;
    d4 fn[4];
    if constexpr (G + 1 < 4) frags_read<G + 1>(fn, buf, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < cnt; ++i) acc[t0 + i] = mfma(f[i][r], xb[r], acc[t0 + i]);
    if constexpr (G == 1) mid();
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (G + 1 < 4) {
#pragma unroll
        for (int i = 0; i < grp_at(G + 2) - grp_at(G + 1); ++i) f[i] = fn[i];
        en1_group<G + 1>(acc, f, buf, xb, lane, mid);
    }
}
template <class Mid>
__device__ __forceinline__ void en1_chunk(d4 (&acc)[kWide64Frags], const d2 *buf, const d4 xb, int lane, Mid mid) {
    d4 f[4];
    frags_read<0>(f, buf, lane);
    en1_group<0>(acc, f, buf, xb, lane, mid);
}
// de4, one output chunk: one tile over the 13 k tiles of the 200-feature activation, the k tiles of a group in an accumulator each
// (a[i]: k tiles i, 4 + i, 7 + i, 10 + i), added as (a0 + a1) + (a2 + a3)
template <int G, class Mid>
__device__ __forceinline__ void de4_group(d4 (&a)[4], const d4 (&s7)[kWide64Frags], d4 (&f)[4], const d2 *buf, int lane, Mid mid) {
    constexpr int q0 = grp_at(G), cnt = grp_at(G + 1) - q0;
    d4 fn[4];
    if constexpr (G + 1 < 4) frags_read<G + 1>(fn, buf, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < cnt; ++i) a[i] = mfma(f[i][r], s7[q0 + i][r], a[i]);
    if constexpr (G == 1) mid();
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (G + 1 < 4) {
#pragma unroll
        for (int i = 0; i < grp_at(G + 2) - grp_at(G + 1); ++i) f[i] = fn[i];
        de4_group<G + 1>(a, s7, f, buf, lane, mid);
    }
}
template <class Mid>
__device__ __forceinline__ d4 de4_chunk(const d4 (&s7)[kWide64Frags], const d2 *buf, int lane, Mid mid) {
    d4 a[4], f[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = (d4){0.0, 0.0, 0.0, 0.0};
    frags_read<0>(f, buf, lane);
    de4_group<0>(a, s7, f, buf, lane, mid);
    return (a[0] + a[1]) + (a[2] + a[3]);
}

// IN64: the table's rows are float64 (encode, forward + loss; the latent rows of a decode take either type at run time)
template <int ZC, int KIND, bool IN64>
__global__ void __launch_bounds__(256) wide64_kernel(const double *__restrict__ packed, const void *__restrict__ xin, int in_f64, int64_t n,
                                                     const double *__restrict__ feats, void *__restrict__ out, int out_f64,
                                                     const double *__restrict__ renorm, const uint8_t *__restrict__ imask,
                                                     double *__restrict__ loss_part, int fr, int zr) {
    using WL = Wide64<ZC>;
    using N = typename WL::N;
    constexpr int G0 = KIND == K_DECODE ? 4 : 1, NGM = KIND == K_FORWARD ? 6 : 3;
    using SQ = ISeq<N, G0, NGM, kRing64W>;
    constexpr int kNB = N::bf_off(N::L) - N::bf_off(0);
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    d2 *stage = (d2 *)lds_raw;                                  // two chunk buffers of 2 x 832 16-byte halves
    d4 *bias_lds = (d4 *)lds_raw + 2 * kWide64ChunkD4;
    __shared__ double red[256];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lg = lane >> 4;
    const d4 *narrow = (const d4 *)packed;
    const d4 *wen1 = (const d4 *)(packed + WL::en1_off()), *wde4 = (const d4 *)(packed + WL::de4_off(fr));
    const double *bias7 = packed + WL::bias_off(fr);
    const int nc = WL::chunks(fr);
    // always-readable stand-ins for the optional arrays (see chunk_request): 2 fr doubles / fr bytes of the fragments
    const double *mnrg = feats ? feats : (const double *)wen1, *rnrm = renorm ? renorm : (const double *)wde4;
    const uint8_t *imk = imask ? imask : (const uint8_t *)wde4;
    const bool normalise = feats != nullptr;
    for (int i = threadIdx.x; i < kNB; i += 256) bias_lds[i] = narrow[N::bf_off(0) + i];
    WStream ws;
    ws.rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)packed, 0, N::packed_d4() * 32, 0x00020000);
    ws.voff = lane * 32;
    d4 ring[SQ::D];
    iseq_span<SQ>(ring, ws, std::make_integer_sequence<int, SQ::D>{}, 0);
    __syncthreads();
    double lacc = 0.0;
    const int64_t ngroup = (n + 63) / 64;
    // every wave of the workgroup runs every group (the barriers of the stage are the workgroup's); a wave whose rows lie beyond n
    // computes on row 0 and stores nothing
    for (int64_t grp = blockIdx.x; grp < ngroup; grp += gridDim.x) {
        asm volatile("" : "+v"(ws.voff));      // keep the fragment loads inside the loop (LICM would hoist the narrow layers)
        const int64_t row = (grp * 4 + wave) * 16 + (lane & 15);
        const bool valid = row < n;
        const int64_t rbase = (valid ? row : 0) * fr;
        d4 st[4];
        d4 s7[kWide64Frags];
        if constexpr (KIND == K_DECODE) {
            d4 a4[tiles(ZC)], s5[4], s6[7];
            load_rows64<ZC, true>(a4, xin, in_f64, row, valid, lg, nullptr, zr);
            ilayer<N, SQ, 0, G0>(a4, s5, ring, ws, bias_lds, lg);
            ilayer<N, SQ, 1, G0>(s5, s6, ring, ws, bias_lds, lg);
            ilayer<N, SQ, 2, G0>(s6, s7, ring, ws, bias_lds, lg);
        } else {
            // ---------------- en1, streamed over the table's column chunks ----------------
            d4 s1[kWide64Frags], s2[7], s3[4], s4[tiles(ZC)];
#pragma unroll
            for (int t = 0; t < kWide64Frags; ++t) s1[t] = bias_lds[t * 4 + lg];
            // The stage runs a chunk and a half ahead, the rows two chunks: at the top of chunk c the fragments of chunk c + 2 and its
            // columns of the rows are requested; the fragments of chunk c + 1 (requested a chunk ago) go to the idle buffer between the
            // second and the third group, its columns are finished behind the MFMAs.  Two register sets take turns (the loop runs in
            // steps of two chunks: the chunk count is even, fused64w.hpp); the body has no branch, so that the compiler counts the
            // loads in flight exactly -- behind the last chunk the requests repeat that chunk and nothing uses them.
            RawChunk64<IN64> rawA, rawB;
            d4 stB[4];
            stage_load(st, wen1);
            chunk_request(rawA, xin, rbase, 0, lg, fr, mnrg);
            stage_store(stage, st);
            stage_load(st, wen1 + kWide64ChunkD4);
            d4 xb = chunk_finish(rawA, 0, lg, fr, normalise);
            chunk_request(rawA, xin, rbase, 1, lg, fr, mnrg);
            __syncthreads();
            auto step = [&](int c, d4 (&st_use)[4], d4 (&st_load)[4], RawChunk64<IN64> &raw_use, RawChunk64<IN64> &raw_load) __attribute__((always_inline)) {
                const int c1 = c + 1 < nc ? c + 1 : nc - 1, c2 = c + 2 < nc ? c + 2 : nc - 1;
                stage_load(st_load, wen1 + (size_t)c2 * kWide64ChunkD4);
                chunk_request(raw_load, xin, rbase, c2, lg, fr, mnrg);
                en1_chunk(s1, stage + (c & 1) * 2 * kWide64ChunkD4, xb, lane, [&] { stage_store(stage + ((c + 1) & 1) * 2 * kWide64ChunkD4, st_use); });
                xb = chunk_finish(raw_use, c1, lg, fr, normalise);
                __syncthreads();
            };
            for (int c = 0; c < nc; c += 2) {
                step(c, st, stB, rawA, rawB);
                step(c + 1, stB, st, rawB, rawA);
            }
            lrelu(s1);
            ilayer<N, SQ, 0, G0>(s1, s2, ring, ws, bias_lds, lg);
            ilayer<N, SQ, 1, G0>(s2, s3, ring, ws, bias_lds, lg);
            ilayer<N, SQ, 2, G0>(s3, s4, ring, ws, bias_lds, lg);
            if constexpr (KIND == K_ENCODE) {
                store_rows64<ZC, true>(s4, out, out_f64, row, valid, lg, nullptr, nullptr, zr);
            } else {
                d4 s5[4], s6[7];
                ilayer<N, SQ, 3, G0>(s4, s5, ring, ws, bias_lds, lg);
                ilayer<N, SQ, 4, G0>(s5, s6, ring, ws, bias_lds, lg);
                ilayer<N, SQ, 5, G0>(s6, s7, ring, ws, bias_lds, lg);
            }
        }
        if constexpr (KIND != K_ENCODE) {
            // ---------------- de4, streamed over the output's column chunks ----------------
            // The stage as in en1.  A chunk's epilogue (bias, loss or un-normalisation, the stores) runs between the second and the third
            // group of the NEXT chunk: its stores are then long on their way when the loop comes round, and what it needs of its own chunk
            // (bias, min / range / int mask or the rows' columns) is requested right behind it, a whole chunk before its use.
            // A decode of few rows deals the output chunks of a row group to gridDim.y workgroups (whole pairs of chunks, a contiguous range
            // each; every one of them runs the narrow layers of its rows itself: 2 % of the work): an output column is still summed by
            // one wave in the same order, so the result does not depend on the split.  Forward + loss: one range.
            int c_lo = 0, c_hi = nc;
            if constexpr (KIND == K_DECODE) {
                c_lo = 2 * ((nc / 2) * (int)blockIdx.y / (int)gridDim.y);
                c_hi = 2 * ((nc / 2) * ((int)blockIdx.y + 1) / (int)gridDim.y);
            }
            d4 stB[4], o_prev = (d4){0.0, 0.0, 0.0, 0.0}, b7, rmn, rrg;
            uint8_t int_col[4];
            RawChunk64<IN64> raw;
            auto request = [&](int c) __attribute__((always_inline)) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = 16 * c + 4 * r + lg;
                    const int fc = f < fr ? f : 0;
                    b7[r] = bias7[f];                                  // (padded to whole chunks)
                    if constexpr (KIND == K_DECODE) {
                        rmn[r] = rnrm[fc];
                        rrg[r] = rnrm[fr + fc];
                        int_col[r] = imk[fc];
                    }
                }
                if constexpr (KIND == K_FORWARD) chunk_request(raw, xin, rbase, c, lg, fr, mnrg);
            };
            auto epilogue = [&](int c) __attribute__((always_inline)) {      // of chunk c, whose sums are in o_prev; c = c_lo - 1: nothing
                const d4 o = o_prev + b7;
                d4 x0 = (d4){0.0, 0.0, 0.0, 0.0};
                if constexpr (KIND == K_FORWARD) x0 = chunk_finish(raw, c, lg, fr, normalise);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = 16 * c + 4 * r + lg;
                    if (!valid || f < 16 * c_lo || f >= fr) continue;
                    double v = o[r];
                    if constexpr (KIND == K_FORWARD) {
                        const double d = v - x0[r];
                        lacc += d * d;
                        if (!out) continue;
                    } else if (renorm) {      // norm * range + min with two roundings, then the int-column truncation (store_rows64)
                        v = __dadd_rn(__dmul_rn(v, rrg[r]), rmn[r]);
                        if (imask && int_col[r]) v = trunc(v);
                    }
                    if (out_f64) ((double *)out)[row * fr + f] = v;
                    else ((float *)out)[row * fr + f] = (float)v;
                }
            };
            stage_load(st, wde4 + (size_t)c_lo * kWide64ChunkD4);
            request(c_lo);
            stage_store(stage, st);
            stage_load(st, wde4 + (size_t)(c_lo + 1) * kWide64ChunkD4);
            __syncthreads();
            auto step = [&](int c, d4 (&st_use)[4], d4 (&st_load)[4]) __attribute__((always_inline)) {
                const int c2 = c + 2 < c_hi ? c + 2 : c_hi - 1;
                stage_load(st_load, wde4 + (size_t)c2 * kWide64ChunkD4);
                const d4 o = de4_chunk(s7, stage + (c & 1) * 2 * kWide64ChunkD4, lane, [&] {
                    stage_store(stage + ((c + 1) & 1) * 2 * kWide64ChunkD4, st_use);
                    epilogue(c - 1);      // (no branch here either: the chunk in front of the range has no column to store)
                    request(c);
                });
                o_prev = o;
                __syncthreads();
            };
            for (int c = c_lo; c < c_hi; c += 2) {
                step(c, st, stB);
                step(c + 1, stB, st);
            }
            epilogue(c_hi - 1);
        }
        iseq_tail<SQ, SQ::real>(ring, ws, std::make_integer_sequence<int, SQ::total - SQ::real>{});      // step over the padding
    }
    if constexpr (KIND == K_FORWARD) {      // per-workgroup loss partial, fixed order
        const double wsum = block_sum_tree(lacc, red);
        if (threadIdx.x == 0) loss_part[blockIdx.x] = wsum;
    }
}

template <int ZC> constexpr int lds_bytes() {
    using N = typename Wide64<ZC>::N;
    return (2 * kWide64ChunkD4 + (N::bf_off(N::L) - N::bf_off(0))) * 32;
}

template <int ZC, int KIND, bool IN64>
int wide64_grid(int *grid) {      // workgroups the chip holds at once (asked once per kernel: the library runs on gfx950 only)
    static int known = 0;
    if (known > 0) { *grid = known; return BAMD_OK; }
    int dev = 0, cus = 0, per_cu = 0;
    BAMD_HIP(hipGetDevice(&dev));
    BAMD_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    BAMD_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)wide64_kernel<ZC, KIND, IN64>, 256, lds_bytes<ZC>()));
    *grid = known = cus * (per_cu > 0 ? per_cu : 1);
    return BAMD_OK;
}

template <int ZC, int KIND, bool IN64>
int wide64_launch(bamd_handle *h, const double *packed, int grid_cap, const void *x, int x_dtype, int64_t n, const double *features, void *out,
                  int out_dtype, const double *renorm, const uint8_t *imask, double *loss_sum, hipStream_t s) {
    const int fr = h->dims[0], zr = h->dims[4];
    if (grid_cap <= 0)
        if (const int rc = wide64_grid<ZC, KIND, IN64>(&grid_cap)) return rc;
    const int64_t ngroup = (n + 63) / 64;
    const int grid = (int)(ngroup < grid_cap ? ngroup : grid_cap);
    // a decode that leaves most of the chip idle splits every row group's output chunks over up to 4 workgroups (see the kernel)
    const int split = KIND == K_DECODE ? (grid_cap / grid < 1 ? 1 : grid_cap / grid > 4 ? 4 : grid_cap / grid) : 1;
    if (KIND == K_FORWARD)
        if (const int rc = h->lossp.ensure(sizeof(double) * (size_t)(grid > 1024 ? grid : 1024))) return rc;      // one partial per workgroup
    hipLaunchKernelGGL((wide64_kernel<ZC, KIND, IN64>), dim3(grid, split), dim3(256), lds_bytes<ZC>(), s, packed, x, (int)(x_dtype == BAMD_F64), n, features,
                       out, (int)(out_dtype == BAMD_F64), renorm, imask, KIND == K_FORWARD ? (double *)h->lossp.p : (double *)nullptr, fr, zr);
    if (KIND == K_FORWARD)
        hipLaunchKernelGGL(sum_partials_fixed_k<double>, dim3(1), dim3(256), 0, s, (const double *)h->lossp.p, grid, 1.0 / fr, loss_sum, 0);
    BAMD_HIP(hipGetLastError());
    return BAMD_OK;
}

template <int ZC>
int wide64_run(bamd_handle *h, const double *packed, int grid_cap, InferKind kind, const void *x, int x_dtype, int64_t n, const double *features,
               void *out, int out_dtype, const double *renorm, const uint8_t *imask, double *loss_sum, hipStream_t s) {
#define W_ARGS h, packed, grid_cap, x, x_dtype, n, features, out, out_dtype, renorm, imask, loss_sum, s
    if (kind == K_DECODE) return wide64_launch<ZC, K_DECODE, true>(W_ARGS);      // (the latent rows' type is a kernel argument)
    if (kind == K_ENCODE) return x_dtype == BAMD_F64 ? wide64_launch<ZC, K_ENCODE, true>(W_ARGS) : wide64_launch<ZC, K_ENCODE, false>(W_ARGS);
    return x_dtype == BAMD_F64 ? wide64_launch<ZC, K_FORWARD, true>(W_ARGS) : wide64_launch<ZC, K_FORWARD, false>(W_ARGS);
#undef W_ARGS
}

template <int ZC, int KIND, bool IN64>
int wide64_lds_attr() {
    BAMD_HIP(hipFuncSetAttribute((const void *)wide64_kernel<ZC, KIND, IN64>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes<ZC>()));
    return BAMD_OK;
}
template <int ZC>
int wide64_setup() {
    int rc = wide64_lds_attr<ZC, K_ENCODE, true>();
    if (!rc) rc = wide64_lds_attr<ZC, K_ENCODE, false>();
    if (!rc) rc = wide64_lds_attr<ZC, K_DECODE, true>();
    if (!rc) rc = wide64_lds_attr<ZC, K_FORWARD, true>();
    if (!rc) rc = wide64_lds_attr<ZC, K_FORWARD, false>();
    return rc;
}

}  // namespace

int fused64w_setup(int zc) { return zc <= 31 ? wide64_setup<31>() : wide64_setup<63>(); }

int fused64w_infer_launch(int zc, bamd_handle *h, const double *packed, int grid_cap, InferKind kind, const void *x, int x_dtype, int64_t n,
                          const double *features, void *out, int out_dtype, const double *renorm, const uint8_t *imask, double *loss_sum,
                          hipStream_t s) {
    if (zc <= 31) return wide64_run<31>(h, packed, grid_cap, kind, x, x_dtype, n, features, out, out_dtype, renorm, imask, loss_sum, s);
    return wide64_run<63>(h, packed, grid_cap, kind, x, x_dtype, n, features, out, out_dtype, renorm, imask, loss_sum, s);
}

}  // namespace bamd
