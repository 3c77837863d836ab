// The fp64 wide inference class (fused64w.hip): AE(n, z) with the reference's hidden widths, 128 <= n <= 4096 columns, z <= 63, n and z as
// kernel arguments.  Shared by fused64w.hip (kernels, launch) and fused64.hip (the handle's state, the pack map, the dispatch).
#pragma once
#include "fused64_net.hpp"

namespace bamd {
namespace {

// Packed buffer of a wide fp64 handle, in doubles:
//   [ narrow | en1 chunks | de4 chunks | de4 bias ]
// narrow: the layout of Net64<15, ZC> (ZC = 31 | 63: the latent class) -- the forward fragments of layers 1 .. 6 and the bias fragments of
//   layers 0 .. 6 are filled, everything else in it (a one-tile layer 0 / 7, the transposed fragments) stays zero and is never read;
// en1: per 16-column chunk c of the table the 13 fragments (c, t) of the 200 output features, fragment (c, t) lane (i, g) component
//   r = W_0[16 t + i][16 c + 4 r + g] (A operand of step r; zero beyond the table's width);
// de4: per 16-column OUTPUT chunk c the 13 fragments (c, q) over the 200 inputs, lane (i, g) component r = W_7[16 c + i][16 q + 4 r + g];
// de4 bias: 16 doubles per chunk in natural order (zero beyond the width).  The chunk count is rounded up to an even number.
constexpr int kWide64Min = 128, kWide64Max = 4096, kWide64Frags = 13, kWide64ChunkD4 = kWide64Frags * 64;
template <int ZC> struct Wide64 {
    using N = Net64<15, ZC>;
    // (an EVEN number of chunks: the kernels walk them two at a time; a table of an odd number gets one more chunk of zero fragments)
    __host__ __device__ static constexpr int chunks(int f) { return ((f + 15) / 16 + 1) & ~1; }
    __host__ __device__ static constexpr size_t en1_off() { return (size_t)N::packed_d4() * 4; }
    __host__ __device__ static constexpr size_t de4_off(int f) { return en1_off() + (size_t)chunks(f) * kWide64ChunkD4 * 4; }
    __host__ __device__ static constexpr size_t bias_off(int f) { return de4_off(f) + (size_t)chunks(f) * kWide64ChunkD4 * 4; }
    __host__ __device__ static constexpr size_t doubles(int f) { return bias_off(f) + (size_t)chunks(f) * 16; }
};

}  // namespace

// fused64w.hip: wide64_kernel<ZC, KIND> on a persistent grid of at most `grid_cap` workgroups (<= 0: as many as the chip holds at once);
// zc: 31 | 63.  `packed`: the layout above, made from the handle's current parameters.
int fused64w_infer_launch(int zc, bamd_handle *h, const double *packed, int grid_cap, InferKind kind, const void *x, int x_dtype, int64_t n,
                          const double *features, void *out, int out_dtype, const double *renorm, const uint8_t *imask, double *loss_sum,
                          hipStream_t s);
int fused64w_setup(int zc);      // once per handle: the kernels' LDS attribute
}  // namespace bamd
