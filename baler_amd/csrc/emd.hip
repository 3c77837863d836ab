// Per-row EMD of tables of 65 .. 4096 columns (utils.mse_loss_emd_l1's EMD term, reference utils.py:112-119):
//     *out = sum_rows mean_k | sort(x_row)_k - sort(recon_row)_k |
// Both sides of a row go into LDS in their own type, padded with +inf to M = the next power of two (one instantiation per M), and ONE
// bitonic network (pair indexing, direction rule and exchange of bitonic.hpp) sorts the two arrays side by side; |a_k - b_k| is
// formed in float64 after exact widening, over the first n_cols ranks only.  Who sorts a row:
//     65 .. 256 columns    a wave (G = 64): four rows per workgroup, the steps separated by a wave-level fence, no workgroup barrier;
//     257 .. 4096 columns  the workgroup (G = 256).
// Either way a thread has E = M / G keys of each side in registers: per step through LDS it reads its E / 2 pairs, exchanges and
// writes them back; the steps whose partners lie within E consecutive keys run in registers on the thread's own block (EmdShape).
// A NaN is unordered, so the network may leave it anywhere, the padding included: every thread notes the NaNs it loads and poisons
// its own term of the row's sum.  +-inf sort as values.
// Sums, all in a fixed order that depends on the table's shape only: a thread adds its ranks t, t + G, ... in order, the G threads are
// added in a tree, the row sums of ONE part (emd_rows_per_part(n_rows, G) consecutive rows) in row order per group and the groups in
// index order, and the parts by sum_partials_fixed_k (sum_partials_k of elementwise.hip is one thread's chain: 512 partials there, up
// to 8192 here).  The grid is persistent over the parts (BALER_AMD_EMD_WGS lowers its size), and no sum depends on it.
#include "bamd_internal.hpp"
#include "bitonic.hpp"

namespace bamd {
namespace {

constexpr int kEmdMaxParts = 8192;      // at most this many partial sums per call, whatever the row count

constexpr int emd_group(int m) { return m <= 256 ? 64 : 256; }      // threads that sort one row of padded size m
// rows per partial sum: the fewest that keep a call within kEmdMaxParts parts, in whole passes of a workgroup's 256 / G groups
inline int64_t emd_rows_per_part(int64_t n, int group_threads) {
    const int ng = 256 / group_threads;
    const int64_t rows = (n + kEmdMaxParts - 1) / kEmdMaxParts;
    return (rows + ng - 1) / ng * ng;
}

template <int G> __device__ __forceinline__ void group_sync() {
    if (G == 64) {      // one wave: its LDS instructions execute in order, the fences keep the compiler from moving them across
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

// the sum over the G threads of a group in a fixed tree; valid in the group's thread 0
template <int G> __device__ __forceinline__ double group_sum(double v, double *red) {
    if (G == 64) {
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        return v;
    }
    return block_sum_tree(v, red);
}

// Where the keys of one padded row live and who owns them.  Steps with partner distance j >= E exchange through LDS, pair by pair; the
// steps with j < E stay inside the E consecutive keys [tid E, tid E + E) that a thread takes into registers once per k (for k <= E
// once for all of them).  A thread's block is E sizeof(T) bytes, so a wave's 16-byte reads of its blocks would land S = E sizeof(T) / 16
// to a bank: the 16-byte slots of every 256-byte bank row are XOR-ed with the row's index (at() below), which keeps a slot whole, a
// block inside itself and consecutive keys on distinct banks.
template <typename T, int M>
struct EmdShape {
    static constexpr int G = emd_group(M), NG = 256 / G, E = M / G;
    static constexpr int ES = 16 / (int)sizeof(T);             // keys per 16-byte slot
    static constexpr int VE = E < ES ? E : ES;                 // keys per LDS access of a thread's block
    static constexpr int S = E / VE;                           // such accesses per block
    static constexpr int RE = 256 / (int)sizeof(T);            // keys per bank row
    static_assert(S <= 8, "the slot bits and the row bits of at() must not overlap");
    typedef T vec __attribute__((ext_vector_type(VE)));
    static __device__ __forceinline__ int at(int i) { return i ^ (((i / RE) & (S - 1)) * ES); }
};

// all steps with j < E of the phases k = 2 .. E (FIRST), or of one phase k > E, on the block that starts at key `base`
template <bool FIRST, int E, typename T>
__device__ __forceinline__ void emd_block_steps(T (&v)[E], int base, int k) {
#pragma unroll
    for (int kk = FIRST ? 2 : E; kk <= E; kk <<= 1)
#pragma unroll
        for (int j = kk >> 1; j > 0; j >>= 1)
#pragma unroll
            for (int t = 0; t < E / 2; ++t) {
                const int lo = bitonic_lo(t, j);
                bitonic_cmpx(v[lo], v[lo + j], FIRST ? bitonic_up(base + lo, kk) : bitonic_up(base, k));
            }
}

template <typename T, int M>
__global__ void __launch_bounds__(256, 2) emd_sort_k(const T *__restrict__ x, const T *__restrict__ r, int64_t n, int c, int64_t part_rows,
                                                  int n_part, double *__restrict__ part) {
    typedef EmdShape<T, M> Sh;
    typedef typename Sh::vec vec;
    constexpr int G = Sh::G, NG = Sh::NG, E = Sh::E, VE = Sh::VE;
    __shared__ __attribute__((aligned(16))) T lds[NG * 2 * M];
    __shared__ double red[256];
    const int grp = threadIdx.x / G, tid = threadIdx.x % G;
    T *a = lds + grp * 2 * M, *b = a + M;
    for (int p = blockIdx.x; p < n_part; p += gridDim.x) {
        const int64_t r0 = (int64_t)p * part_rows, r1 = r0 + part_rows < n ? r0 + part_rows : n;
        double acc = 0.0;
        for (int64_t row = r0 + grp; row < r1; row += NG) {
            const T *xr = x + row * c, *rr = r + row * c;
            T va[E], vb[E];
#pragma unroll
            for (int u = 0; u < E; ++u) {      // all loads of the row in flight before the first use
                const int i = tid + u * G;
                va[u] = vb[u] = pos_inf<T>();
                if (i < c) { va[u] = xr[i]; vb[u] = rr[i]; }
            }
            bool nan = false;
#pragma unroll
            for (int u = 0; u < E; ++u) {
                nan |= va[u] != va[u] || vb[u] != vb[u];
                a[Sh::at(tid + u * G)] = va[u]; b[Sh::at(tid + u * G)] = vb[u];
            }
            group_sync<G>();
            for (int k = E; k <= M; k <<= 1) {
                for (int j = k >> 1; j >= E; j >>= 1) {      // (none while k = E)
                    int lo[E / 2], hi[E / 2];
#pragma unroll
                    for (int u = 0; u < E / 2; ++u) {      // the step's reads first, then the exchanges and the writes
                        const int l = bitonic_lo(tid + u * G, j);
                        lo[u] = Sh::at(l); hi[u] = Sh::at(l + j);
                        va[2 * u] = a[lo[u]]; va[2 * u + 1] = a[hi[u]];
                        vb[2 * u] = b[lo[u]]; vb[2 * u + 1] = b[hi[u]];
                        const bool up = bitonic_up(l, k);
                        bitonic_cmpx(va[2 * u], va[2 * u + 1], up);
                        bitonic_cmpx(vb[2 * u], vb[2 * u + 1], up);
                    }
#pragma unroll
                    for (int u = 0; u < E / 2; ++u) {
                        a[lo[u]] = va[2 * u]; a[hi[u]] = va[2 * u + 1];
                        b[lo[u]] = vb[2 * u]; b[hi[u]] = vb[2 * u + 1];
                    }
                    group_sync<G>();
                }
                const int base = tid * E;
#pragma unroll
                for (int u = 0; u < Sh::S; ++u) {
                    const vec wa = *(const vec *)&a[Sh::at(base + u * VE)], wb = *(const vec *)&b[Sh::at(base + u * VE)];
#pragma unroll
                    for (int e = 0; e < VE; ++e) { va[u * VE + e] = wa[e]; vb[u * VE + e] = wb[e]; }
                }
                if (k == E) { emd_block_steps<true>(va, base, k); emd_block_steps<true>(vb, base, k); }
                else { emd_block_steps<false>(va, base, k); emd_block_steps<false>(vb, base, k); }
#pragma unroll
                for (int u = 0; u < Sh::S; ++u) {
                    vec wa, wb;
#pragma unroll
                    for (int e = 0; e < VE; ++e) { wa[e] = va[u * VE + e]; wb[e] = vb[u * VE + e]; }
                    *(vec *)&a[Sh::at(base + u * VE)] = wa; *(vec *)&b[Sh::at(base + u * VE)] = wb;
                }
                group_sync<G>();
            }
            double s = 0.0;
            for (int k = tid; k < c; k += G) s += fabs((double)a[Sh::at(k)] - (double)b[Sh::at(k)]);
            if (nan) s = __builtin_nan("");
            s = group_sum<G>(s, red);
            acc += s / (double)c;
            group_sync<G>();      // the next row's stores overwrite what this row's sum has read
        }
        if (NG > 1) {
            if (tid == 0) red[grp] = acc;
            __syncthreads();
            if (threadIdx.x == 0) {
                double s = red[0];
                for (int g = 1; g < NG; ++g) s += red[g];
                part[p] = s;
            }
            __syncthreads();
        } else if (threadIdx.x == 0) {
            part[p] = acc;
        }
    }
}

// workgroups of emd_sort_k<T, M> the chip holds at once (asked once per kernel: the library runs on gfx950 only)
template <typename T, int M>
int emd_grid(int *grid) {
    static int known = 0;
    if (known > 0) { *grid = known; return BAMD_OK; }
    int dev = 0, cus = 0, per_cu = 0;
    BAMD_HIP(hipGetDevice(&dev));
    BAMD_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    BAMD_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)emd_sort_k<T, M>, 256, 0));
    *grid = known = cus * (per_cu > 0 ? per_cu : 1);
    return BAMD_OK;
}

template <typename T, int M>
int emd_wide_M(const void *x, const void *r, int64_t n, int c, double *out, hipStream_t s) {
    const int64_t part_rows = emd_rows_per_part(n, emd_group(M));
    const int n_part = (int)((n + part_rows - 1) / part_rows);
    int cap = 0;
    if (const int rc = emd_grid<T, M>(&cap)) return rc;
    const long long env = env_ll("BALER_AMD_EMD_WGS", 0);      // tests: a workgroup takes several parts at small sizes
    if (env > 0 && env < cap) cap = (int)env;
    DevBuf &scratch = scratch_for(1, s);
    if (const int rc = scratch.ensure(sizeof(double) * (size_t)n_part)) return rc;
    double *part = (double *)scratch.p;
    hipLaunchKernelGGL((emd_sort_k<T, M>), dim3(n_part < cap ? n_part : cap), dim3(256), 0, s, (const T *)x, (const T *)r, n, c, part_rows,
                       n_part, part);
    hipLaunchKernelGGL(sum_partials_fixed_k<double>, dim3(1), dim3(256), 0, s, (const double *)part, n_part, 1.0, out, 0);
    BAMD_HIP(hipGetLastError());
    return BAMD_OK;
}

template <typename T>
int emd_wide_T(const void *x, const void *r, int64_t n, int c, double *out, hipStream_t s) {
    if (c <= 128) return emd_wide_M<T, 128>(x, r, n, c, out, s);
    if (c <= 256) return emd_wide_M<T, 256>(x, r, n, c, out, s);
    if (c <= 512) return emd_wide_M<T, 512>(x, r, n, c, out, s);
    if (c <= 1024) return emd_wide_M<T, 1024>(x, r, n, c, out, s);
    if (c <= 2048) return emd_wide_M<T, 2048>(x, r, n, c, out, s);
    return emd_wide_M<T, 4096>(x, r, n, c, out, s);
}

}  // namespace

int launch_emd_rows_wide(const void *x, const void *r, int dtype, int64_t n, int c, double *out, hipStream_t s) {
    if (dtype == BAMD_F64) return emd_wide_T<double>(x, r, n, c, out, s);
    return emd_wide_T<float>(x, r, n, c, out, s);
}

}  // namespace bamd
