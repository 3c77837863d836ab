// Per-frame and per-pixel statistics of a (before, after) pair of 2-D tables (n_frames, frame_elems): the data path of
// plotting.plot_2D (plotting.py:370-437) -- the colour scale and the difference image of every frame -- plus the per-frame error sums
// and the per-pixel error map over all frames.  Two HBM-streaming passes, each reading each table once: bamd_frame_stats (row
// reductions, any frame length) and bamd_pixel_moments (column reductions, any frame length).  d = before - after in the input dtype,
// every square and sum in float64, extrema skip NaN, every sum in a fixed order: no float atomics.  gfx950 only.
#include "bamd_internal.hpp"

namespace bamd {
namespace {

constexpr int kFrameRows = 10;              // rows of bamd_frame_stats' output (include/baler_amd_frames.h)
constexpr int kPixelRows = 5;               // rows of bamd_pixel_moments' output
constexpr int64_t kSeg = 4096;              // elements of one segment of a frame: the work of one wave
constexpr int kFly = 2;                     // vector pairs a lane of frame_stats_k loads ahead
constexpr int kFrameGrid = 8192;            // workgroups of a frame launch at the most (the rest by stride)
constexpr int kPixelWgs = 2048;             // workgroups bamd_pixel_moments aims at: 8 per CU

// Extrema skip NaN: the running value is never NaN, and IEEE minNum / maxNum (v_min_f64 / v_max_f64) return the operand that is not.
// (Compare-and-select keeps a 64-bit lane mask in SGPRs per comparison: forty of them per vector pair made frame_stats_k spill.)
__device__ __forceinline__ double min_skip(double a, double b) { return __builtin_fmin(a, b); }
__device__ __forceinline__ double max_skip(double a, double b) { return __builtin_fmax(a, b); }

// ---- bamd_frame_stats -----------------------------------------------------------------------------------------------------------
// The order rule.  A frame's elements are cut into vectors of V (16 bytes: 4 float32, 2 float64) counted from the FRAME's first
// element, and into segments of kSeg elements.  A segment is the work of one wave: lane l accumulates the segment's vectors l,
// l + 64, ... element by element; the 64 accumulators are folded by the fixed tree of wave_fold; the segments of a frame are folded
// in an order that depends on their number alone by frame_final_k.  Nothing in that order knows the frame's index, the table's
// length, the grid or an address: a frame whose two bases (and `diff`) are 16-byte aligned is read with vector loads, any other
// with scalar loads of the same elements.  (A workgroup per frame with a barrier-and-LDS fold read the 262,144 x 2,500 float32
// table at 3.3 TB/s, and one 4M-element frame in 64 segments of 65,536 at 0.9 TB/s: too few loads in flight, too few workgroups.)
// Rows 0..5 are extrema (even: min, odd: max), rows 6..9 sums.
__device__ __forceinline__ void acc_init(double (&v)[kFrameRows]) {
#pragma unroll
    for (int r = 0; r < kFrameRows; ++r) v[r] = r >= 6 ? 0.0 : ((r & 1) ? -(double)INFINITY : (double)INFINITY);
}
template <int R>
__device__ __forceinline__ double fold_row(double a, double b) {
    if constexpr (R >= 6) return a + b;
    else if constexpr (R & 1) return max_skip(a, b);
    else return min_skip(a, b);
}
template <int R = 0>
__device__ __forceinline__ void fold_rows(double (&v)[kFrameRows], const double (&o)[kFrameRows]) {
    if constexpr (R < kFrameRows) {
        v[R] = fold_row<R>(v[R], o[R]);
        fold_rows<R + 1>(v, o);
    }
}
template <typename T>
__device__ __forceinline__ void acc_elem(double (&v)[kFrameRows], T b, T a, T d) {
    const double db = (double)b, da = (double)a, dd = (double)d;
    const double o[kFrameRows] = {db, db, da, da, dd, dd, dd, dd * dd, db * db, (b != b || a != a) ? 1.0 : 0.0};
    fold_rows(v, o);
}
// lane 0 of every wave ends with the wave's fold: ((0 + 32) + (16 + 48)) + ... (a fixed tree; the other lanes' values are not used)
__device__ __forceinline__ void wave_fold(double (&v)[kFrameRows]) {
#pragma unroll
    for (int st = 32; st > 0; st >>= 1) {
        double o[kFrameRows];
#pragma unroll
        for (int r = 0; r < kFrameRows; ++r) o[r] = __shfl_down(v[r], st, 64);
        fold_rows(v, o);
    }
}

// A unit is one segment of one frame, unit u = frame * nseg + segment, and belongs to ONE wave (four units per workgroup; no
// barrier, no LDS).  nseg == 1: the unit's ten values go to `out` (10, n_frames); else to part[u][10] for frame_final_k.
// Where the frame is aligned a lane keeps kFly of its vector pairs in flight; it still accumulates them in vector order.
template <typename T, int V>
__device__ __forceinline__ void acc_vec(double (&v)[kFrameRows], const T (&bb)[V], const T (&aa)[V], T (&dd)[V], int valid) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
        dd[j] = bb[j] - aa[j];                              // the input dtype, one rounding (plotting.py:415)
        if (j < valid) acc_elem<T>(v, bb[j], aa[j], dd[j]);
    }
}

template <typename T, int V>
__global__ void __launch_bounds__(256) frame_stats_k(const T *__restrict__ before, const T *__restrict__ after, int64_t n_frames,
                                                     int64_t F, int nseg, double *__restrict__ out, double *__restrict__ part,
                                                     T *__restrict__ diff) {
    typedef T vec_t __attribute__((ext_vector_type(V)));
    constexpr int64_t S = 64 * V;                           // elements between two vectors of a lane
    const int l = threadIdx.x & 63;
    const int64_t units = n_frames * nseg;
    for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += (int64_t)gridDim.x * 4) {
        const int64_t f = u / nseg;
        const int64_t e0 = (u - f * nseg) * kSeg;
        const int64_t e1 = F < e0 + kSeg ? F : e0 + kSeg;
        const T *b = before + f * F, *a = after + f * F;
        T *dst = diff ? diff + f * F : nullptr;
        const bool vec = (((uintptr_t)b | (uintptr_t)a | (uintptr_t)dst) & 15u) == 0;
        double v[kFrameRows];
        acc_init(v);
        int64_t e = e0 + (int64_t)l * V;
        if (vec) {
            for (; e + (kFly - 1) * S + V <= e1; e += kFly * S) {
                vec_t vb[kFly], va[kFly];
#pragma unroll
                for (int k = 0; k < kFly; ++k) {
                    vb[k] = *reinterpret_cast<const vec_t *>(b + e + k * S);
                    va[k] = *reinterpret_cast<const vec_t *>(a + e + k * S);
                }
#pragma unroll
                for (int k = 0; k < kFly; ++k) {
                    T bb[V], aa[V], dd[V];
#pragma unroll
                    for (int j = 0; j < V; ++j) { bb[j] = vb[k][j]; aa[j] = va[k][j]; }
                    acc_vec<T, V>(v, bb, aa, dd, V);
                    if (dst) {
                        vec_t vd;
#pragma unroll
                        for (int j = 0; j < V; ++j) vd[j] = dd[j];
                        *reinterpret_cast<vec_t *>(dst + e + k * S) = vd;
                    }
                }
            }
        }
        for (; e < e1; e += S) {                            // the rest, the segment's last (partial) vector, and frames that are not aligned
            T bb[V], aa[V], dd[V];
            const int valid = e + V <= e1 ? V : (int)(e1 - e);
            if (valid == V && vec) {
                const vec_t vb = *reinterpret_cast<const vec_t *>(b + e), va = *reinterpret_cast<const vec_t *>(a + e);
#pragma unroll
                for (int j = 0; j < V; ++j) { bb[j] = vb[j]; aa[j] = va[j]; }
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    bb[j] = j < valid ? b[e + j] : (T)0;
                    aa[j] = j < valid ? a[e + j] : (T)0;
                }
            }
            acc_vec<T, V>(v, bb, aa, dd, valid);
            if (dst) {
                if (valid == V && vec) {
                    vec_t vd;
#pragma unroll
                    for (int j = 0; j < V; ++j) vd[j] = dd[j];
                    *reinterpret_cast<vec_t *>(dst + e) = vd;
                } else {
#pragma unroll
                    for (int j = 0; j < V; ++j)
                        if (j < valid) dst[e + j] = dd[j];
                }
            }
        }
        wave_fold(v);
        if (l == 0) {
#pragma unroll
            for (int r = 0; r < kFrameRows; ++r) {
                if (nseg == 1) out[(int64_t)r * n_frames + f] = v[r];
                else part[u * kFrameRows + r] = v[r];
            }
        }
    }
}

// The finishing launch of frames longer than a segment: a wave per frame folds the frame's nseg partials -- lane l takes segments
// l, l + 64, ... in order, then the tree of wave_fold: an order that depends on nseg alone.
__global__ void __launch_bounds__(256) frame_final_k(const double *__restrict__ part, int64_t n_frames, int nseg,
                                                     double *__restrict__ out) {
    const int l = threadIdx.x & 63;
    for (int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); f < n_frames; f += (int64_t)gridDim.x * 4) {
        double v[kFrameRows];
        acc_init(v);
        for (int sg = l; sg < nseg; sg += 64) {
            double o[kFrameRows];
#pragma unroll
            for (int r = 0; r < kFrameRows; ++r) o[r] = part[(f * nseg + sg) * kFrameRows + r];
            fold_rows(v, o);
        }
        wave_fold(v);
        if (l == 0) {
#pragma unroll
            for (int r = 0; r < kFrameRows; ++r) out[(int64_t)r * n_frames + f] = v[r];
        }
    }
}

// ---- bamd_pixel_moments ---------------------------------------------------------------------------------------------------------
// Lanes run along the pixels.  F >= 256: workgroup (x, y) owns pixels [256 x, 256 x + 256) of the frames of range y, one pixel per
// thread.  F < 256: a workgroup uses its first PY * F threads, PY = 256 / F: thread t is pixel t % F of sub-row t / F and reads
// element t of every PY frames -- contiguous --, then thread p < F folds the PY sub-rows of pixel p in sub-row order.  Range y is
// frames [y L, y L + L).  One range: the workgroup finishes into `out` itself; else its five values go to part[y][5][F] and
// pixel_final_k adds the ranges in range order.  PY, L and the number of ranges depend on (n_frames, frame_elems) alone.
struct PixAcc {
    double s, s2, mn, mx, nan;
};
__device__ __forceinline__ PixAcc pix_init() { return {0.0, 0.0, (double)INFINITY, -(double)INFINITY, 0.0}; }
template <typename T>
__device__ __forceinline__ void pix_elem(PixAcc &p, T b, T a) {
    const T d = b - a;
    const double dd = (double)d;
    p.s += dd;
    p.s2 += dd * dd;
    p.mn = min_skip(p.mn, dd);
    p.mx = max_skip(p.mx, dd);
    p.nan += (b != b || a != a) ? 1.0 : 0.0;
}
__device__ __forceinline__ void pix_fold(PixAcc &p, const PixAcc &o) {
    p.s += o.s;
    p.s2 += o.s2;
    p.mn = min_skip(p.mn, o.mn);
    p.mx = max_skip(p.mx, o.mx);
    p.nan += o.nan;
}
__device__ __forceinline__ void pix_finish(const PixAcc &p, double *__restrict__ out, int64_t F, int64_t pix, int accumulate) {
    PixAcc r = p;
    if (accumulate) {
        r = {out[pix], out[F + pix], out[2 * F + pix], out[3 * F + pix], out[4 * F + pix]};
        pix_fold(r, p);
    }
    out[pix] = r.s;
    out[F + pix] = r.s2;
    out[2 * F + pix] = r.mn;
    out[3 * F + pix] = r.mx;
    out[4 * F + pix] = r.nan;
}

template <typename T>
__global__ void __launch_bounds__(256) pixel_partial_k(const T *__restrict__ before, const T *__restrict__ after, int64_t n, int64_t F,
                                                       int PY, int64_t L, double *__restrict__ part, double *__restrict__ out,
                                                       int accumulate) {
    __shared__ double sh[kPixelRows][256];
    const int t = threadIdx.x;
    const bool narrow = F < 256;
    const int Fi = narrow ? (int)F : 256;
    const int py = narrow ? t / Fi : 0;
    const int64_t pix = narrow ? t - py * Fi : (int64_t)blockIdx.x * 256 + t;
    const bool active = narrow ? py < PY : pix < F;
    const int64_t lo = (int64_t)blockIdx.y * L;
    const int64_t hi = n < lo + L ? n : lo + L;
    PixAcc p = pix_init();
    if (active) {
        int64_t f = lo + py;
        for (; f + 3 * (int64_t)PY < hi; f += 4 * (int64_t)PY) {      // four frames' loads in flight, accumulated in frame order
            T b[4], a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                b[k] = before[(f + (int64_t)k * PY) * F + pix];
                a[k] = after[(f + (int64_t)k * PY) * F + pix];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) pix_elem<T>(p, b[k], a[k]);
        }
        for (; f < hi; f += PY) pix_elem<T>(p, before[f * F + pix], after[f * F + pix]);
    }
    bool writer = active;
    if (PY > 1) {                                           // (the same in every thread of the launch)
        sh[0][t] = p.s; sh[1][t] = p.s2; sh[2][t] = p.mn; sh[3][t] = p.mx; sh[4][t] = p.nan;
        __syncthreads();
        writer = t < Fi;
        if (writer) {
            for (int y = 1; y < PY; ++y) {
                const int o = y * Fi + t;
                pix_fold(p, PixAcc{sh[0][o], sh[1][o], sh[2][o], sh[3][o], sh[4][o]});
            }
        }
    }
    if (!writer) return;
    if (gridDim.y == 1) {
        pix_finish(p, out, F, pix, accumulate);
    } else {
        double *dst = part + (int64_t)blockIdx.y * kPixelRows * F + pix;
        dst[0] = p.s; dst[F] = p.s2; dst[2 * F] = p.mn; dst[3 * F] = p.mx; dst[4 * F] = p.nan;
    }
}

// The finishing launch: a thread per pixel adds the R ranges in range order.  R = 0 leaves the neutral elements.
__global__ void __launch_bounds__(256) pixel_final_k(const double *__restrict__ part, int R, int64_t F, double *__restrict__ out,
                                                     int accumulate) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= F) return;
    PixAcc p = pix_init();
    for (int r = 0; r < R; ++r) {
        const double *src = part + (int64_t)r * kPixelRows * F + pix;
        pix_fold(p, PixAcc{src[0], src[F], src[2 * F], src[3 * F], src[4 * F]});
    }
    pix_finish(p, out, F, pix, accumulate);
}

// The refusals both exports share, before anything is launched
int check_frames(const char *fn, const void *before, const void *after, int dtype, int64_t n_frames, int64_t frame_elems,
                 const double *out) {
    if (dtype != BAMD_F32 && dtype != BAMD_F64) {
        set_error(std::string(fn) + ": dtype must be BAMD_F32 or BAMD_F64 (BAMD_F16 / BAMD_BF16 are latent codes: z_dtype of bamd_encode / bamd_decode only)");
        return BAMD_ERR_INVALID;
    }
    BAMD_REQUIRE_AS(fn, frame_elems >= 1, "frame_elems must be positive");
    BAMD_REQUIRE_AS(fn, n_frames >= 0, "negative n_frames");
    BAMD_REQUIRE_AS(fn, out, "null output");
    BAMD_REQUIRE_AS(fn, n_frames == 0 || (before && after), "null table");
    BAMD_REQUIRE_AS(fn, n_frames == 0 || frame_elems <= INT64_MAX / 8 / n_frames, "the table's byte count overflows int64");
    return BAMD_OK;
}

}  // namespace
}  // namespace bamd

using namespace bamd;

extern "C" {

int bamd_frame_stats(const void *before, const void *after, int dtype, int64_t n_frames, int64_t frame_elems, double *out, void *diff,
                     void *stream) {
    hipStream_t s = (hipStream_t)stream;
    int rc = check_frames(__func__, before, after, dtype, n_frames, frame_elems, out);
    if (rc) return rc;
    if (n_frames == 0) return BAMD_OK;                      // `out` is (10, 0)
    const int64_t F = frame_elems;
    const int64_t nseg64 = (F + kSeg - 1) / kSeg;
    BAMD_REQUIRE(nseg64 <= INT32_MAX && n_frames <= INT64_MAX / nseg64, "too many segments");
    const int nseg = (int)nseg64;
    const int64_t units = n_frames * nseg;
    double *part = nullptr;
    if (nseg > 1) {
        BAMD_REQUIRE(units <= INT64_MAX / (int64_t)(kFrameRows * sizeof(double)), "too many segments");
        DevBuf &scratch = scratch_for(4, s);
        rc = scratch.ensure((size_t)units * kFrameRows * sizeof(double));
        if (rc) return rc;
        part = (double *)scratch.p;
    }
    const int64_t blocks = (units + 3) / 4;
    const dim3 grid((unsigned)(blocks < kFrameGrid ? blocks : kFrameGrid));
    if (dtype == BAMD_F64)
        hipLaunchKernelGGL((frame_stats_k<double, 2>), grid, dim3(256), 0, s, (const double *)before, (const double *)after, n_frames, F,
                           nseg, out, part, (double *)diff);
    else
        hipLaunchKernelGGL((frame_stats_k<float, 4>), grid, dim3(256), 0, s, (const float *)before, (const float *)after, n_frames, F,
                           nseg, out, part, (float *)diff);
    if (nseg > 1) {
        const int64_t fb = (n_frames + 3) / 4;
        hipLaunchKernelGGL(frame_final_k, dim3((unsigned)(fb < kFrameGrid ? fb : kFrameGrid)), dim3(256), 0, s, part, n_frames, nseg,
                           out);
    }
    BAMD_HIP(hipGetLastError());
    return BAMD_OK;
}

int bamd_pixel_moments(const void *before, const void *after, int dtype, int64_t n_frames, int64_t frame_elems, double *out,
                       int accumulate, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    int rc = check_frames(__func__, before, after, dtype, n_frames, frame_elems, out);
    if (rc) return rc;
    const int64_t F = frame_elems, n = n_frames;
    const int64_t tiles = (F + 255) / 256;
    BAMD_REQUIRE(tiles <= INT32_MAX, "frame_elems is too large");
    const dim3 fgrid((unsigned)tiles);
    if (n == 0) {
        if (!accumulate) hipLaunchKernelGGL(pixel_final_k, fgrid, dim3(256), 0, s, (const double *)nullptr, 0, F, out, 0);
        BAMD_HIP(hipGetLastError());
        return BAMD_OK;
    }
    // the frame ranges: enough workgroups to fill the chip, at least eight frames per thread -- of (n_frames, frame_elems) alone
    const int PY = F < 256 ? (int)(256 / F) : 1;
    int64_t R = (kPixelWgs + tiles - 1) / tiles;
    const int64_t r_max = (n + 8 * PY - 1) / (8 * PY);
    R = R < r_max ? R : r_max;
    const int64_t L = (n + R - 1) / R;
    R = (n + L - 1) / L;
    double *part = nullptr;
    if (R > 1) {
        DevBuf &scratch = scratch_for(5, s);
        rc = scratch.ensure((size_t)R * kPixelRows * (size_t)F * sizeof(double));
        if (rc) return rc;
        part = (double *)scratch.p;
    }
    const dim3 grid((unsigned)(F < 256 ? 1 : tiles), (unsigned)R);
    if (dtype == BAMD_F64)
        hipLaunchKernelGGL(pixel_partial_k<double>, grid, dim3(256), 0, s, (const double *)before, (const double *)after, n, F, PY, L,
                           part, out, accumulate ? 1 : 0);
    else
        hipLaunchKernelGGL(pixel_partial_k<float>, grid, dim3(256), 0, s, (const float *)before, (const float *)after, n, F, PY, L,
                           part, out, accumulate ? 1 : 0);
    if (R > 1) hipLaunchKernelGGL(pixel_final_k, fgrid, dim3(256), 0, s, part, (int)R, F, out, accumulate ? 1 : 0);
    BAMD_HIP(hipGetLastError());
    return BAMD_OK;
}

}  // extern "C"
