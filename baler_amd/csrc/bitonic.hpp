// The bitonic compare-exchange network of the library's two families of sorting kernels: swd.hip (a batch per projection, (value, row)
// pairs beside plain values) and emd.hip (the two sides of a table row).  ONE definition of the pair indexing, of the direction rule and
// of the exchange; what a step exchanges (which arrays, with or without a payload) is the caller's `cx`.  bitonic_network is the loop
// over all steps for arrays that live in LDS (swd.hip); emd.hip keeps its keys in registers and writes its own loop over the same parts.
//   element count n = 2^p; step (k, j): pair t (0 <= t < n/2) is (lo, lo + j) with lo = (t / j) * 2j + t % j, sorted ascending when
//   bit k of lo's GLOBAL index is clear.  Keys are only ever compared and moved, never computed on: the sort is exact, an unordered
//   compare (NaN) is false either way, so a NaN stays in the array but nothing orders it -- callers that must see it look for it
//   themselves.  Padding is +inf (equal to a real +inf, which is harmless: equal keys are interchangeable).
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
