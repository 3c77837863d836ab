// Column residual / response statistics of a (before, after) table pair: the data path of plotting.plot_1D
// (plotting.py:101-239).  Two HBM-streaming passes, each reading each table once: bamd_column_moments (counts, sums,
// extrema) and bamd_column_hist (four histograms per column with numpy's bin rule; the residual's bins may differ per column).
// gfx950 only.
#include "bamd_internal.hpp"

namespace bamd {
namespace {

constexpr int kStats = 13;          // rows of bamd_column_moments' output (include/baler_amd.h)
constexpr int kMaxCols = 128;
constexpr int kMaxEdges = 1025;

// ---- how a workgroup walks the tables -------------------------------------------------------------------------------------------
// Both tables are read as FLAT arrays with V-element (16-byte) loads, consecutive lanes on consecutive vectors.  A workgroup of BS
// threads uses its first T of them, T = the largest multiple of c / gcd(c, V) that fits: a tile of T * V elements is then a whole
// number of rows, so slot j of thread t sees ONE column, (t * V + j) % c, in every tile it visits, and its row is
// tile * rows_per_tile + (t * V + j) / c -- no 64-bit division in the loop, and per-column accumulators can live in registers.
// V = 1 (scalar loads) serves tables whose two base addresses are not both 16-byte aligned.
struct Walk {
    int T, rows_per_tile;
    int64_t tiles;
};
int gcd_i(int a, int b) { return b ? gcd_i(b, a % b) : a; }
Walk make_walk(int bs, int c, int V, int64_t n) {
    const int cp = c / gcd_i(c, V);
    Walk w;
    w.T = (bs / cp) * cp;
    const int64_t tile = (int64_t)w.T * V;
    w.rows_per_tile = (int)(tile / c);
    w.tiles = (n * c + tile - 1) / tile;
    return w;
}

template <typename T, int V>
__device__ __forceinline__ void load_vec(const T *__restrict__ p, int64_t e, int64_t total, T (&out)[V]) {
    if (e + V <= total) {
        if constexpr (V == 1) {
            out[0] = p[e];
        } else {
            typedef T vec_t __attribute__((ext_vector_type(V)));
            const vec_t v = *reinterpret_cast<const vec_t *>(p + e);
#pragma unroll
            for (int j = 0; j < V; ++j) out[j] = v[j];
        }
    } else {                                    // the table's last, partial vector
#pragma unroll
        for (int j = 0; j < V; ++j) out[j] = e + j < total ? p[e + j] : (T)0;
    }
}

// What slot j of this thread is, for the whole launch
template <int V>
struct Slots {
    int col[V], rowoff[V];
    __device__ __forceinline__ void init(int t, int c) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int off = t * V + j;
            col[j] = off % c;
            rowoff[j] = off / c;
        }
    }
};

// keep[j]: the row of slot j is inside the table and passes the cut `before[row][cut_col] >= cut` (a NaN there keeps the row, as
// numpy's `<` does).  Slots of one row share the load.
template <typename T, int V>
__device__ __forceinline__ void row_keep(const T *__restrict__ before, int64_t row0, const Slots<V> &sl, int64_t n, int c, int cut_col,
                                         double cut, bool (&keep)[V]) {
    bool prev = true;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int64_t row = row0 + sl.rowoff[j];
        bool k = row < n;
        if (k && cut_col >= 0) {
            if (j > 0 && sl.rowoff[j] == sl.rowoff[j - 1]) k = prev;
            else k = !((double)before[row * c + cut_col] < cut);
        }
        keep[j] = k;
        prev = k;
    }
}

// ---- pass A: moments ------------------------------------------------------------------------------------------------------------
template <int OP>   // 0 sum, 1 min, 2 max
__device__ __forceinline__ double comb(double a, double b) {
    if constexpr (OP == 0) return a + b;
    else if constexpr (OP == 1) return b < a ? b : a;      // a NaN never wins: extrema skip NaN
    else return b > a ? b : a;
}
template <int OP>
__device__ __forceinline__ double ident() { return OP == 0 ? 0.0 : (OP == 1 ? (double)INFINITY : -(double)INFINITY); }

// One statistic of the workgroup: the T * V slot values (slot i belongs to column i % c) folded per column in a FIXED order -- G
// threads per column take every G-th slot of it, then one thread per column adds the G partial results in order.
// (block_sum_tree sums ONE scalar per nine barriers; 5 c of them per workgroup would cost more than the stream they finish.)
template <int OP, int V>
__device__ __forceinline__ void fold_stat(const double (&v)[V], int T, int c, int G, double *sh, double *sh2, double *dst) {
    const int t = threadIdx.x;
    if (t < T) {
#pragma unroll
        for (int j = 0; j < V; ++j) sh[t * V + j] = v[j];
    }
    __syncthreads();
    const int K = T * V / c;
    if (t < G * c) {
        const int g = t / c, col = t - g * c;
        double acc = ident<OP>();
        for (int k = g; k < K; k += G) acc = comb<OP>(acc, sh[k * c + col]);
        sh2[t] = acc;
    }
    __syncthreads();
    if (t < c) {
        double r = sh2[t];
        for (int g = 1; g < G; ++g) r = comb<OP>(r, sh2[g * c + t]);
        dst[t] = r;
    }
    __syncthreads();
}

template <typename T, int V>
__global__ void __launch_bounds__(256) colmom_partial_k(const T *__restrict__ before, const T *__restrict__ after, int64_t n, int c,
                                                        int cut_col, double cut, int Tn, int rows_per_tile, int64_t tiles,
                                                        double *__restrict__ part) {
    __shared__ double sh[256 * V], sh2[256];
    const int t = threadIdx.x;
    const int64_t total = n * c;
    Slots<V> sl;
    sl.init(t, c);
    double cnt[V], s_rd[V], s_rd2[V], mn_rd[V], mx_rd[V], s_rp[V], s_rp2[V], mn_b[V], mx_b[V], mn_a[V], mx_a[V], mn_s[V], mx_s[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        cnt[j] = s_rd[j] = s_rd2[j] = s_rp[j] = s_rp2[j] = 0.0;
        mn_rd[j] = mn_b[j] = mn_a[j] = mn_s[j] = INFINITY;
        mx_rd[j] = mx_b[j] = mx_a[j] = mx_s[j] = -INFINITY;
    }
    if (t < Tn) {
        for (int64_t q = blockIdx.x; q < tiles; q += gridDim.x) {
            const int64_t e = (q * Tn + t) * V;
            if (e >= total) break;
            T b[V], a[V];
            load_vec<T, V>(before, e, total, b);
            load_vec<T, V>(after, e, total, a);
            bool keep[V];
            row_keep<T, V>(before, q * rows_per_tile, sl, n, c, cut_col, cut, keep);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                if (!keep[j]) continue;
                // numpy's ufuncs: the input dtype, one rounding per operation (plotting.py:122-123, 143-147)
                const T rd = a[j] - b[j];
                const T rp = (rd / b[j]) * (T)100;
                const T sm = b[j] + a[j];
                const double drd = (double)rd, db = (double)b[j], da = (double)a[j], ds = (double)sm;
                cnt[j] += 1.0;
                s_rd[j] += drd;
                s_rd2[j] += (double)(rd * rd);
                s_rp[j] += (double)rp;
                s_rp2[j] += (double)(rp * rp);
                mn_rd[j] = comb<1>(mn_rd[j], drd); mx_rd[j] = comb<2>(mx_rd[j], drd);
                mn_b[j] = comb<1>(mn_b[j], db);    mx_b[j] = comb<2>(mx_b[j], db);
                mn_a[j] = comb<1>(mn_a[j], da);    mx_a[j] = comb<2>(mx_a[j], da);
                mn_s[j] = comb<1>(mn_s[j], ds);    mx_s[j] = comb<2>(mx_s[j], ds);
            }
        }
    }
    int G = 256 / c;
    G = G > 16 ? 16 : G;
    double *dst = part + (int64_t)blockIdx.x * kStats * c;
    fold_stat<0, V>(cnt, Tn, c, G, sh, sh2, dst + 0 * c);
    fold_stat<0, V>(s_rd, Tn, c, G, sh, sh2, dst + 1 * c);
    fold_stat<0, V>(s_rd2, Tn, c, G, sh, sh2, dst + 2 * c);
    fold_stat<1, V>(mn_rd, Tn, c, G, sh, sh2, dst + 3 * c);
    fold_stat<2, V>(mx_rd, Tn, c, G, sh, sh2, dst + 4 * c);
    fold_stat<0, V>(s_rp, Tn, c, G, sh, sh2, dst + 5 * c);
    fold_stat<0, V>(s_rp2, Tn, c, G, sh, sh2, dst + 6 * c);
    fold_stat<1, V>(mn_b, Tn, c, G, sh, sh2, dst + 7 * c);
    fold_stat<2, V>(mx_b, Tn, c, G, sh, sh2, dst + 8 * c);
    fold_stat<1, V>(mn_a, Tn, c, G, sh, sh2, dst + 9 * c);
    fold_stat<2, V>(mx_a, Tn, c, G, sh, sh2, dst + 10 * c);
    fold_stat<1, V>(mn_s, Tn, c, G, sh, sh2, dst + 11 * c);
    fold_stat<2, V>(mx_s, Tn, c, G, sh, sh2, dst + 12 * c);
}

__device__ __forceinline__ int stat_op(int s) { return (s <= 2 || s == 5 || s == 6) ? 0 : ((s & 1) ? 1 : 2); }

template <int OP>
__device__ __forceinline__ double block_extreme_tree(double v, double *sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) sh[threadIdx.x] = comb<OP>(sh[threadIdx.x], sh[threadIdx.x + st]);
        __syncthreads();
    }
    return sh[0];
}

// The finishing launch: one workgroup per column over the per-workgroup slabs in workgroup order (strided partial sums, then the
// fixed tree).  nblk = 0 leaves the neutral elements (or, with accumulate, `out` as it is).
__global__ void __launch_bounds__(256) colmom_final_k(const double *__restrict__ part, int nblk, int c, double *__restrict__ out,
                                                      int accumulate) {
    __shared__ double sh[256];
    const int col = blockIdx.x;
    for (int s = 0; s < kStats; ++s) {
        const int op = stat_op(s);
        double v = op == 0 ? 0.0 : (op == 1 ? (double)INFINITY : -(double)INFINITY);
        for (int b = threadIdx.x; b < nblk; b += 256) {
            const double p = part[((int64_t)b * kStats + s) * c + col];
            v = op == 0 ? v + p : (op == 1 ? comb<1>(v, p) : comb<2>(v, p));
        }
        __syncthreads();           // sh of the previous statistic has been read
        const double r = op == 0 ? block_sum_tree(v, sh) : (op == 1 ? block_extreme_tree<1>(v, sh) : block_extreme_tree<2>(v, sh));
        if (threadIdx.x == 0) {
            double *o = out + (int64_t)s * c + col;
            if (!accumulate) *o = r;
            else *o = op == 0 ? *o + r : (op == 1 ? comb<1>(*o, r) : comb<2>(*o, r));
        }
    }
}

// ---- pass B: histograms ---------------------------------------------------------------------------------------------------------
struct HistArgs {
    const double *edges_resp, *edges_resid, *edges_val;     // device; null: that histogram is skipped (its n is then 0)
    int n_er, n_ed, n_ev;                                   // EDGE counts
    unsigned long long *counts_resp, *counts_resid, *counts_before, *counts_after;
    int cols_per_group;                                     // a workgroup with blockIdx.y = g counts columns [g * cpg, (g + 1) * cpg)
};

// np.histogram's rule for an explicit bin array: bin k holds e[k] <= v < e[k+1], the last bin also v == e[nb]; NaN and values outside
// [e[0], e[nb]] are not counted.  A multiply guesses the bin and the edge array itself decides: exact for any non-decreasing edges,
// zero to two steps for evenly spaced ones.  -> bin, or -1.
__device__ __forceinline__ int find_bin(double v, const double *e, int nb, double scale) {
    const double e0 = e[0];
    if (!(v >= e0 && v <= e[nb])) return -1;
    const double g = (v - e0) * scale;
    int k = !(g >= 0.0) ? 0 : (g > (double)(nb - 1) ? nb - 1 : (int)g);
    while (k > 0 && v < e[k]) --k;
    while (k < nb - 1 && v >= e[k + 1]) ++k;
    return k;
}

// Workgroup-private 32-bit counters in LDS ([column of the group][resp | resid | before | after bins]) beside the edges; a tile adds
// at most T * V <= 4096 to a counter, so the counters are flushed (64-bit integer atomics: order-free, hence repeatable) every
// kFlushTiles tiles, before one could wrap.
constexpr int64_t kFlushTiles = (int64_t)1 << 19;

template <typename T, int V>
__global__ void __launch_bounds__(1024) colhist_k(const T *__restrict__ before, const T *__restrict__ after, int64_t n, int c,
                                                  int cut_col, double cut, int Tn, int rows_per_tile, int64_t tiles, HistArgs ha) {
    extern __shared__ double lds[];
    const int t = threadIdx.x;
    const int col0 = blockIdx.y * ha.cols_per_group;
    const int ncol = min(ha.cols_per_group, c - col0);
    const int nbr = ha.n_er ? ha.n_er - 1 : 0, nbd = ha.n_ed ? ha.n_ed - 1 : 0, nbv = ha.n_ev ? ha.n_ev - 1 : 0;
    const int bins_per_col = nbr + nbd + 2 * nbv;
    double *e_resp = lds;
    double *e_resid = e_resp + ha.n_er;
    double *e_val = e_resid + ha.n_ed;                                    // [ncol][n_ev]
    unsigned *cnts = reinterpret_cast<unsigned *>(e_val + (size_t)ha.cols_per_group * ha.n_ev);   // [ncol][bins_per_col]
    for (int i = t; i < ha.n_er; i += 1024) e_resp[i] = ha.edges_resp[i];
    for (int i = t; i < ha.n_ed; i += 1024) e_resid[i] = ha.edges_resid[i];
    for (int i = t; i < ncol * ha.n_ev; i += 1024) e_val[i] = ha.edges_val[(int64_t)col0 * ha.n_ev + i];
    __syncthreads();
    const double sc_resp = nbr ? (double)nbr / (e_resp[nbr] - e_resp[0]) : 0.0;
    const double sc_resid = nbd ? (double)nbd / (e_resid[nbd] - e_resid[0]) : 0.0;

    const int64_t total = n * c;
    Slots<V> sl;
    sl.init(t, c);
    int lc[V];                      // the slot's column inside this group, or -1
    double sc_val[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        lc[j] = (t < Tn && sl.col[j] >= col0 && sl.col[j] < col0 + ncol) ? sl.col[j] - col0 : -1;
        sc_val[j] = 0.0;
        if (lc[j] >= 0 && nbv) {
            const double *ev = e_val + lc[j] * ha.n_ev;
            sc_val[j] = (double)nbv / (ev[nbv] - ev[0]);
        }
    }
    const int ncnt = ncol * bins_per_col;
    for (int64_t q0 = blockIdx.x; q0 < tiles; q0 += kFlushTiles * gridDim.x) {
        for (int i = t; i < ncnt; i += 1024) cnts[i] = 0u;
        __syncthreads();
        int64_t q_end = q0 + kFlushTiles * gridDim.x;
        q_end = q_end < tiles ? q_end : tiles;
        if (t < Tn) {
            for (int64_t q = q0; q < q_end; q += gridDim.x) {
                const int64_t e = (q * Tn + t) * V;
                if (e >= total) break;
                T b[V], a[V];
                load_vec<T, V>(before, e, total, b);
                load_vec<T, V>(after, e, total, a);
                bool keep[V];
                row_keep<T, V>(before, q * rows_per_tile, sl, n, c, cut_col, cut, keep);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    if (!keep[j] || lc[j] < 0) continue;
                    const T rd = a[j] - b[j];
                    const T rp = (rd / b[j]) * (T)100;
                    unsigned *cc = cnts + lc[j] * bins_per_col;
                    if (nbr) {
                        const int k = find_bin((double)rp, e_resp, nbr, sc_resp);
                        if (k >= 0) atomicAdd(cc + k, 1u);
                    }
                    if (nbd) {
                        const int k = find_bin((double)rd, e_resid, nbd, sc_resid);
                        if (k >= 0) atomicAdd(cc + nbr + k, 1u);
                    }
                    if (nbv) {
                        const double *ev = e_val + lc[j] * ha.n_ev;
                        int k = find_bin((double)b[j], ev, nbv, sc_val[j]);
                        if (k >= 0) atomicAdd(cc + nbr + nbd + k, 1u);
                        k = find_bin((double)a[j], ev, nbv, sc_val[j]);
                        if (k >= 0) atomicAdd(cc + nbr + nbd + nbv + k, 1u);
                    }
                }
            }
        }
        __syncthreads();
        for (int i = t; i < ncnt; i += 1024) {
            const unsigned v = cnts[i];
            if (!v) continue;
            const int l = i / bins_per_col, col = col0 + l;
            int r = i - l * bins_per_col;
            unsigned long long *dst;
            if (r < nbr) dst = ha.counts_resp + (int64_t)col * nbr + r;
            else if ((r -= nbr) < nbd) dst = ha.counts_resid + (int64_t)col * nbd + r;
            else if ((r -= nbd) < nbv) dst = ha.counts_before + (int64_t)col * nbv + r;
            else dst = ha.counts_after + (int64_t)col * nbv + (r - nbv);
            atomicAdd(dst, (unsigned long long)v);
        }
        __syncthreads();
    }
}

// ---- pass B': the residual histogram with per-column, unevenly spaced edges (bamd_column_hist with n_ed < 0) -----------------------
// The edges of one call may run from -1e-3 through the subnormals to +1e-3 (a selection bracket in key space, baler_amd/colbox.py),
// so there is no scale to guess a bin with: the bin is found by bisection over the column's edges in LDS, values and edges compared
// as float64 and no arithmetic on an edge -- a first edge of -inf or a last one of +inf needs no special case.  np.histogram's rule
// as in find_bin.  -> bin, or -1.
__device__ __forceinline__ int bisect_bin(double v, const double *e, int nb) {
    if (!(v >= e[0] && v <= e[nb])) return -1;
    int lo = 0, hi = nb;                // e[lo] <= v, and v < e[hi] or hi == nb
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (v >= e[mid]) lo = mid;
        else hi = mid;
    }
    return lo;
}

// LDS: [cols_per_group][n_edges] edges, then [cols_per_group][n_edges - 1] 32-bit counters: the walk, the column groups of blockIdx.y
// and the flush of colhist_k.
template <typename T, int V>
__global__ void __launch_bounds__(1024) colhist_percol_k(const T *__restrict__ before, const T *__restrict__ after, int64_t n, int c,
                                                         int cut_col, double cut, int Tn, int rows_per_tile, int64_t tiles,
                                                         const double *__restrict__ edges, int n_edges,
                                                         unsigned long long *__restrict__ counts, int cols_per_group) {
    extern __shared__ double lds[];
    const int t = threadIdx.x;
    const int col0 = blockIdx.y * cols_per_group;
    const int ncol = min(cols_per_group, c - col0);
    const int nb = n_edges - 1;
    double *e_col = lds;                                                                           // [ncol][n_edges]
    unsigned *cnts = reinterpret_cast<unsigned *>(e_col + (size_t)cols_per_group * n_edges);      // [ncol][nb]
    for (int i = t; i < ncol * n_edges; i += 1024) e_col[i] = edges[(int64_t)col0 * n_edges + i];

    const int64_t total = n * c;
    Slots<V> sl;
    sl.init(t, c);
    int lc[V];                      // the slot's column inside this group, or -1
#pragma unroll
    for (int j = 0; j < V; ++j) lc[j] = (t < Tn && sl.col[j] >= col0 && sl.col[j] < col0 + ncol) ? sl.col[j] - col0 : -1;
    const int ncnt = ncol * nb;
    for (int64_t q0 = blockIdx.x; q0 < tiles; q0 += kFlushTiles * gridDim.x) {
        for (int i = t; i < ncnt; i += 1024) cnts[i] = 0u;
        __syncthreads();            // (the first round: the edges are in place too)
        int64_t q_end = q0 + kFlushTiles * gridDim.x;
        q_end = q_end < tiles ? q_end : tiles;
        if (t < Tn) {
            for (int64_t q = q0; q < q_end; q += gridDim.x) {
                const int64_t e = (q * Tn + t) * V;
                if (e >= total) break;
                T b[V], a[V];
                load_vec<T, V>(before, e, total, b);
                load_vec<T, V>(after, e, total, a);
                bool keep[V];
                row_keep<T, V>(before, q * rows_per_tile, sl, n, c, cut_col, cut, keep);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    if (!keep[j] || lc[j] < 0) continue;
                    const T rd = a[j] - b[j];
                    const int k = bisect_bin((double)rd, e_col + lc[j] * n_edges, nb);
                    if (k >= 0) atomicAdd(cnts + lc[j] * nb + k, 1u);
                }
            }
        }
        __syncthreads();
        for (int i = t; i < ncnt; i += 1024) {
            const unsigned v = cnts[i];
            if (v) atomicAdd(counts + (int64_t)col0 * nb + i, (unsigned long long)v);      // [col0 + i / nb][i % nb]
        }
        __syncthreads();
    }
}

bool aligned16(const void *a, const void *b) { return (((uintptr_t)a | (uintptr_t)b) & 15u) == 0; }

int check_tables(const char *fn, int dtype, int n_cols, int cut_col) {
    if (dtype != BAMD_F32 && dtype != BAMD_F64) {
        set_error(std::string(fn) + ": dtype must be BAMD_F32 or BAMD_F64 (BAMD_F16 / BAMD_BF16 are latent codes: z_dtype of bamd_encode / bamd_decode only)");
        return BAMD_ERR_INVALID;
    }
    if (n_cols < 1) {
        set_error(std::string(fn) + ": n_cols must be positive");
        return BAMD_ERR_INVALID;
    }
    if (n_cols > kMaxCols) {
        set_error(std::string(fn) + ": tables of more than 128 columns are not served");
        return BAMD_ERR_UNSUPPORTED;
    }
    if (cut_col >= n_cols) {
        set_error(std::string(fn) + ": cut_col must be below n_cols (or negative: no cut)");
        return BAMD_ERR_INVALID;
    }
    return BAMD_OK;
}

}  // namespace
}  // namespace bamd

using namespace bamd;

extern "C" {

int bamd_column_moments(const void *before, const void *after, int dtype, int64_t n_rows, int n_cols, int cut_col, double cut,
                        double *out, int accumulate, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    int rc = check_tables(__func__, dtype, n_cols, cut_col);
    if (rc) return rc;
    BAMD_REQUIRE(out, "null output");
    BAMD_REQUIRE(n_rows >= 0, "negative n_rows");
    const int c = n_cols;
    if (n_rows == 0) {
        if (!accumulate) hipLaunchKernelGGL(colmom_final_k, dim3(c), dim3(256), 0, s, (const double *)nullptr, 0, c, out, 0);
        BAMD_HIP(hipGetLastError());
        return BAMD_OK;
    }
    BAMD_REQUIRE(before && after, "null table");
    const int V = aligned16(before, after) ? (dtype == BAMD_F64 ? 2 : 4) : 1;
    const Walk w = make_walk(256, c, V, n_rows);
    const int nblk = (int)(w.tiles < 1024 ? w.tiles : 1024);
    DevBuf &scratch = scratch_for(3, s);
    rc = scratch.ensure((size_t)nblk * kStats * c * sizeof(double));
    if (rc) return rc;
    double *part = (double *)scratch.p;
#define BAMD_LAUNCH_MOM(TT, VV)                                                                                                    \
    hipLaunchKernelGGL((colmom_partial_k<TT, VV>), dim3(nblk), dim3(256), 0, s, (const TT *)before, (const TT *)after, n_rows, c,  \
                       cut_col, cut, w.T, w.rows_per_tile, w.tiles, part)
    if (dtype == BAMD_F64) {
        if (V == 2) BAMD_LAUNCH_MOM(double, 2); else BAMD_LAUNCH_MOM(double, 1);
    } else {
        if (V == 4) BAMD_LAUNCH_MOM(float, 4); else BAMD_LAUNCH_MOM(float, 1);
    }
#undef BAMD_LAUNCH_MOM
    hipLaunchKernelGGL(colmom_final_k, dim3(c), dim3(256), 0, s, part, nblk, c, out, accumulate ? 1 : 0);
    BAMD_HIP(hipGetLastError());
    return BAMD_OK;
}

int bamd_column_hist(const void *before, const void *after, int dtype, int64_t n_rows, int n_cols, int cut_col, double cut,
                     const double *edges_resp, int n_er, int64_t *counts_resp, const double *edges_resid, int n_ed,
                     int64_t *counts_resid, const double *edges_val, int n_ev, int64_t *counts_before, int64_t *counts_after,
                     int accumulate, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    int rc = check_tables(__func__, dtype, n_cols, cut_col);
    if (rc) return rc;
    BAMD_REQUIRE(n_rows >= 0, "negative n_rows");
    const int c = n_cols;
    HistArgs ha{};
    if (edges_resp) {
        BAMD_REQUIRE(n_er >= 2 && n_er <= kMaxEdges, "edges_resp needs 2 .. 1025 edges");
        BAMD_REQUIRE(counts_resp, "edges_resp without counts_resp");
        ha.edges_resp = edges_resp; ha.n_er = n_er; ha.counts_resp = (unsigned long long *)counts_resp;
    }
    int n_pc = 0;                   // n_ed < 0: edges_resid is (n_cols, n_pc), one edge array per column, and has a launch of its own
    if (edges_resid) {
        BAMD_REQUIRE((n_ed >= 2 && n_ed <= kMaxEdges) || (n_ed <= -2 && n_ed >= -kMaxEdges),
                     "edges_resid needs 2 .. 1025 edges (n_ed), or -n_ed = 2 .. 1025 edges per column (n_ed < 0)");
        BAMD_REQUIRE(counts_resid, "edges_resid without counts_resid");
        if (n_ed > 0) {
            ha.edges_resid = edges_resid; ha.n_ed = n_ed; ha.counts_resid = (unsigned long long *)counts_resid;
        } else {
            n_pc = -n_ed;
        }
    }
    if (edges_val) {
        BAMD_REQUIRE(n_ev >= 2 && n_ev <= kMaxEdges, "edges_val needs 2 .. 1025 edges per column");
        BAMD_REQUIRE(counts_before && counts_after, "edges_val without counts_before / counts_after");
        ha.edges_val = edges_val; ha.n_ev = n_ev;
        ha.counts_before = (unsigned long long *)counts_before; ha.counts_after = (unsigned long long *)counts_after;
    }
    BAMD_REQUIRE(edges_resp || edges_resid || edges_val, "no histogram asked for");
    BAMD_REQUIRE(n_rows == 0 || (before && after), "null table");      // every refusal comes before the first write to counts_*
    if (!accumulate) {
        if (ha.n_er) BAMD_HIP(hipMemsetAsync(counts_resp, 0, (size_t)c * (n_er - 1) * sizeof(int64_t), s));
        if (ha.n_ed) BAMD_HIP(hipMemsetAsync(counts_resid, 0, (size_t)c * (n_ed - 1) * sizeof(int64_t), s));
        if (n_pc) BAMD_HIP(hipMemsetAsync(counts_resid, 0, (size_t)c * (n_pc - 1) * sizeof(int64_t), s));
        if (ha.n_ev) {
            BAMD_HIP(hipMemsetAsync(counts_before, 0, (size_t)c * (n_ev - 1) * sizeof(int64_t), s));
            BAMD_HIP(hipMemsetAsync(counts_after, 0, (size_t)c * (n_ev - 1) * sizeof(int64_t), s));
        }
    }
    if (n_rows == 0) return BAMD_OK;

    int dev = 0, lds_max = 0, cus = 0;
    BAMD_HIP(hipGetDevice(&dev));
    BAMD_HIP(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    BAMD_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const int V = aligned16(before, after) ? (dtype == BAMD_F64 ? 2 : 4) : 1;
    const Walk w = make_walk(1024, c, V, n_rows);
    const int64_t want = w.tiles < (int64_t)(cus > 0 ? cus : 256) ? w.tiles : (int64_t)(cus > 0 ? cus : 256);
    // both LDS checks come before the first launch: every refusal comes before the first count is added
    const bool shared = ha.n_er || ha.n_ed || ha.n_ev;
    const size_t shared_bytes = (size_t)(ha.n_er + ha.n_ed) * sizeof(double);
    const int bins_per_col = (ha.n_er ? ha.n_er - 1 : 0) + (ha.n_ed ? ha.n_ed - 1 : 0) + 2 * (ha.n_ev ? ha.n_ev - 1 : 0);
    const size_t col_bytes = (size_t)ha.n_ev * sizeof(double) + (size_t)bins_per_col * sizeof(unsigned);
    const size_t pc_col_bytes = (size_t)n_pc * sizeof(double) + (size_t)(n_pc ? n_pc - 1 : 0) * sizeof(unsigned);
    BAMD_REQUIRE(!shared || (size_t)lds_max >= shared_bytes + col_bytes, "the device's LDS does not hold one column's histograms");
    BAMD_REQUIRE(!n_pc || (size_t)lds_max >= pc_col_bytes, "the device's LDS does not hold one column's histogram");
    if (n_pc) {
        // LDS of a workgroup: per column its edges and its counters (12 KiB at 1025 edges)
        const size_t col_bytes = pc_col_bytes;
        int cpg = (int)((size_t)lds_max / col_bytes);
        cpg = cpg > c ? c : cpg;
        const int groups = (c + cpg - 1) / cpg;
        cpg = (c + groups - 1) / groups;                  // even column ranges
        const size_t lds_bytes = (size_t)cpg * col_bytes;
        const dim3 grid((unsigned)want, (unsigned)groups);
#define BAMD_LAUNCH_PERCOL(TT, VV)                                                                                                 \
    do {                                                                                                                           \
        BAMD_HIP(hipFuncSetAttribute((const void *)colhist_percol_k<TT, VV>, hipFuncAttributeMaxDynamicSharedMemorySize,           \
                                     (int)lds_bytes));                                                                             \
        hipLaunchKernelGGL((colhist_percol_k<TT, VV>), grid, dim3(1024), lds_bytes, s, (const TT *)before, (const TT *)after,      \
                           n_rows, c, cut_col, cut, w.T, w.rows_per_tile, w.tiles, edges_resid, n_pc,                              \
                           (unsigned long long *)counts_resid, cpg);                                                               \
    } while (0)
        if (dtype == BAMD_F64) {
            if (V == 2) BAMD_LAUNCH_PERCOL(double, 2); else BAMD_LAUNCH_PERCOL(double, 1);
        } else {
            if (V == 4) BAMD_LAUNCH_PERCOL(float, 4); else BAMD_LAUNCH_PERCOL(float, 1);
        }
#undef BAMD_LAUNCH_PERCOL
        BAMD_HIP(hipGetLastError());
        if (!shared) return BAMD_OK;                      // (the shared-edge histograms of the same call: the launch below)
    }
    // LDS of a workgroup: the two shared edge arrays, then per column its value edges and its counters
    int cpg = (int)(((size_t)lds_max - shared_bytes) / col_bytes);
    cpg = cpg > c ? c : cpg;
    const int groups = (c + cpg - 1) / cpg;
    cpg = (c + groups - 1) / groups;                      // even column ranges
    ha.cols_per_group = cpg;
    const size_t lds_bytes = shared_bytes + (size_t)cpg * col_bytes;

    const dim3 grid((unsigned)want, (unsigned)groups);
#define BAMD_LAUNCH_HIST(TT, VV)                                                                                                   \
    do {                                                                                                                           \
        BAMD_HIP(hipFuncSetAttribute((const void *)colhist_k<TT, VV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes)); \
        hipLaunchKernelGGL((colhist_k<TT, VV>), grid, dim3(1024), lds_bytes, s, (const TT *)before, (const TT *)after, n_rows, c,  \
                           cut_col, cut, w.T, w.rows_per_tile, w.tiles, ha);                                                       \
    } while (0)
    if (dtype == BAMD_F64) {
        if (V == 2) BAMD_LAUNCH_HIST(double, 2); else BAMD_LAUNCH_HIST(double, 1);
    } else {
        if (V == 4) BAMD_LAUNCH_HIST(float, 4); else BAMD_LAUNCH_HIST(float, 1);
    }
#undef BAMD_LAUNCH_HIST
    BAMD_HIP(hipGetLastError());
    return BAMD_OK;
}

}  // extern "C"
