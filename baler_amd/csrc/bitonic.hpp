// The bitonic compare-exchange network of the library's two families of sorting kernels: swd.hip (a batch per projection, (value, row)
// pairs beside plain values) and emd.hip (the two sides of a table row).  ONE definition of the pair indexing, of the direction rule and
// of the exchange; what a step exchanges (which arrays, with or without a payload) is the caller's `cx`.  bitonic_network is the loop
// over all steps for arrays that live in LDS (swd.hip); emd.hip keeps its keys in registers and writes its own loop over the same parts.
//   element count n = 2^p; step (k, j): pair t (0 <= t < n/2) is (lo, lo + j) with lo = (t / j) * 2j + t % j, sorted ascending when
//   bit k of lo's GLOBAL index is clear.  Keys are only ever compared and moved, never computed on: the sort is exact.  Two orders:
//   * bitonic_cmpx (emd.hip): the plain `>`.  An unordered compare (NaN) is false either way, so a NaN stays in the array but nothing
//     orders it and the network is no sort around it -- it may end anywhere, the padding included, and push padding in among the
//     real ranks.  A caller of this rule looks for NaNs itself (emd.hip flags them at load) and must not use a payload as an index.
//     Padding is +inf (equal to a real +inf, which is harmless: equal keys are interchangeable).
//   * bitonic_cmpx_total (swd.hip): a TOTAL order.  NaN is the greatest key (after +inf; all NaNs are equal keys), equal keys are
//     ordered by the payload (the row: a stable sort).  Padding is NaN with a payload above every real row (nan_key), so after the
//     sort ranks 0 .. n-1 hold exactly the n real elements -- a NaN among them last -- and every payload there is a real row.
#pragma once
#include <hip/hip_runtime.h>

namespace bamd {

template <typename T> __device__ __forceinline__ T pos_inf();
template <> __device__ __forceinline__ float pos_inf<float>() { return __int_as_float(0x7f800000); }
template <> __device__ __forceinline__ double pos_inf<double>() { return __longlong_as_double(0x7ff0000000000000LL); }

// lower element of pair t at partner distance j (a power of two): t = q j + r  ->  2 q j + r = 2 t - r, without the division
__device__ __forceinline__ int bitonic_lo(int t, int j) { return 2 * t - (t & (j - 1)); }
__device__ __forceinline__ bool bitonic_up(int global_lo, int k) { return (global_lo & k) == 0; }

template <typename T> __device__ __forceinline__ void bitonic_cmpx(T &x, T &y, bool up) {
    if ((x > y) == up) { const T t = x; x = y; y = t; }
}
// (key, payload) pairs: ties are ordered by the payload, so the order of the pairs is total and the sort reproducible
template <typename T> __device__ __forceinline__ void bitonic_cmpx(T &x, T &y, int &xi, int &yi, bool up) {
    const bool gt = x > y || (x == y && xi > yi);
    if (gt == up) { const T t = x; x = y; y = t; const int ti = xi; xi = yi; yi = ti; }
}

// The total order: x after y when x > y, or when x is a NaN and y is not (`!(x <= y)` is "greater or unordered").
template <typename T> __device__ __forceinline__ T nan_key();
template <> __device__ __forceinline__ float nan_key<float>() { return __int_as_float(0x7fc00000); }
template <> __device__ __forceinline__ double nan_key<double>() { return __longlong_as_double(0x7ff8000000000000LL); }
template <typename T> __device__ __forceinline__ bool key_after(T x, T y) { return !(x <= y) && y == y; }

template <typename T> __device__ __forceinline__ void bitonic_cmpx_total(T &x, T &y, bool up) {
    if (key_after(x, y) == up) { const T t = x; x = y; y = t; }
}
template <typename T> __device__ __forceinline__ void bitonic_cmpx_total(T &x, T &y, int &xi, int &yi, bool up) {
    const bool gt = key_after(x, y) || (!key_after(y, x) && xi > yi);      // (neither after the other: equal keys)
    if (gt == up) { const T t = x; x = y; y = t; const int ti = xi; xi = yi; yi = ti; }
}

// Every step (k, j) with k = k_lo .. k_hi and j = min(k / 2, n / 2) .. 1 over the n elements that `nthr` threads hold in LDS;
// g0: the global index of element 0 (a chunk of a longer array takes its directions from there).  cx(lo, hi, up) exchanges,
// sync() separates two steps (a workgroup barrier, or less where one wave owns the array).
template <class CX, class Sync>
__device__ __forceinline__ void bitonic_network(int n, int g0, int k_lo, int k_hi, int tid, int nthr, CX &&cx, Sync &&sync) {
    for (int k = k_lo; k <= k_hi; k <<= 1)
        for (int j = (k >> 1) < n ? (k >> 1) : (n >> 1); j > 0; j >>= 1) {
            for (int t = tid; t < n / 2; t += nthr) {
                const int lo = bitonic_lo(t, j);
                cx(lo, lo + j, bitonic_up(g0 + lo, k));
            }
            sync();
        }
}

}  // namespace bamd
