// Latent codes in caller memory: the ONE definition of how a latent element is stored and loaded for every bamd_dtype
// (float, double, IEEE binary16, bfloat16).  Every inference family's encode epilogue and decode prologue goes through
// latent_store / latent_load (or their 16-bit halves where the float32 / float64 path of a kernel stays as it was).
//
// Rounding rule (include/baler_amd.h, bamd_dtype): a 16-bit code is the round-to-nearest-even conversion of the value the
// handle would have stored as FLOAT32 -- a float64 latent is rounded to float32 first, then to 16 bits, which is what
// t.to(float32).to(float16 / bfloat16) does.  NaN stays NaN, +-inf stays +-inf, float16 overflow gives +-inf (no saturation)
// and float16 subnormals are produced.  Widening a 16-bit code is exact.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/baler_amd.h"

namespace bamd {

inline bool dtype_wide(int d) { return d == BAMD_F32 || d == BAMD_F64; }        // legal for every dtype argument
inline bool dtype_half(int d) { return d == BAMD_F16 || d == BAMD_BF16; }       // legal as the latent of bamd_encode / bamd_decode only
inline bool dtype_code8(int d) { return d == BAMD_U8; }                         // 8-bit codes (bamd_code8): the same two places, always through the float32 workspace
inline size_t dtype_bytes(int d) { return d == BAMD_F64 ? 8 : d == BAMD_F32 ? 4 : d == BAMD_U8 ? 1 : 2; }
// packed b-bit codes, b = 1 .. 7 (bamd_codeb, 0x100 | b): the same two places and the same workspace route as 8-bit codes.  An
// element of a packed row has no size in bytes, so dtype_bytes() has no answer for them; a ROW has one: latent_row_bytes().
inline bool dtype_codeb(int d) { return d >= BAMD_U1 && d <= BAMD_U7; }
inline int codeb_bits(int d) { return d & 0xff; }
inline size_t latent_row_bytes(int64_t z_dim, int d) {      // bytes of one latent row of z_dim codes: rows are byte-aligned
    return dtype_codeb(d) ? (size_t)((z_dim * codeb_bits(d) + 7) / 8) : (size_t)z_dim * dtype_bytes(d);
}

#if defined(__HIPCC__)
// float32 -> binary16 bits: v_cvt_f16_f32, round to nearest even (the truncating pack conversion is NOT used anywhere)
__device__ __forceinline__ uint16_t f16_bits(float v) { return __builtin_bit_cast(uint16_t, (_Float16)v); }
__device__ __forceinline__ float f16_widen(uint16_t u) { return (float)__builtin_bit_cast(_Float16, u); }
// float32 -> bfloat16 bits: round to nearest even on the integer pattern; NaN -> the canonical quiet NaN 0x7fc0 (torch's)
__device__ __forceinline__ uint16_t bf16_bits(float v) {
    uint32_t u = __builtin_bit_cast(uint32_t, v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)0x7fc0;
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
__device__ __forceinline__ float bf16_widen(uint16_t u) { return __builtin_bit_cast(float, (uint32_t)u << 16); }

// BF: the code is bfloat16 (else binary16)
template <bool BF> __device__ __forceinline__ uint16_t half_bits(float v) { return BF ? bf16_bits(v) : f16_bits(v); }
template <bool BF> __device__ __forceinline__ float half_widen(uint16_t u) { return BF ? bf16_widen(u) : f16_widen(u); }
__device__ __forceinline__ uint16_t half_bits(int dtype, float v) { return dtype == BAMD_BF16 ? bf16_bits(v) : f16_bits(v); }
__device__ __forceinline__ float half_widen(int dtype, uint16_t u) { return dtype == BAMD_BF16 ? bf16_widen(u) : f16_widen(u); }
// element i of a latent buffer of `dtype`; S is the kernel's compute scalar (float or double)
template <typename S> __device__ __forceinline__ void latent_store(void *base, int dtype, int64_t i, S v) {
    if (dtype == BAMD_F64) ((double *)base)[i] = (double)v;
    else if (dtype == BAMD_F32) ((float *)base)[i] = (float)v;
    else ((uint16_t *)base)[i] = half_bits(dtype, (float)v);
}
template <typename S> __device__ __forceinline__ S latent_load(const void *base, int dtype, int64_t i) {
    if (dtype == BAMD_F64) return (S)((const double *)base)[i];
    if (dtype == BAMD_F32) return (S)((const float *)base)[i];
    return (S)half_widen(dtype, ((const uint16_t *)base)[i]);
}
// 8-bit codes (include/baler_amd.h, bamd_code8): the ONE definition of their store and load.  Deliberately NOT a case of
// latent_store / latent_load / half_bits above: those inline into the encode / decode kernels, whose register budgets stay as
// they are; only the row-conversion kernels of elementwise.hip use these two.
// float32 latent -> code: rintf (half to even), clamped to [0, 255]; NaN fails both comparisons' "keep" side and gives 0.
__device__ __forceinline__ uint8_t code8_store(float v) {
    float r = rintf(v);
    r = r > 0.0f ? r : 0.0f;          // NaN, -inf, negatives, -0 -> 0
    r = r < 255.0f ? r : 255.0f;      // +inf -> 255
    return (uint8_t)r;
}
__device__ __forceinline__ float code8_load(uint8_t q) { return (float)q; }      // exact
// Packed b-bit codes (include/baler_amd.h, bamd_codeb), b = 1 .. 7: the ONE definition of their store and load, and as above no
// case of latent_store / latent_load.  The store rule is code8_store's with 2^b - 1 in the place of 255.
__device__ __forceinline__ uint32_t codeb_store(float v, int bits) {
    const float top = (float)((1u << bits) - 1u);
    float r = rintf(v);
    r = r > 0.0f ? r : 0.0f;          // NaN, -inf, negatives, -0 -> 0
    r = r < top ? r : top;            // +inf -> 2^b - 1
    return (uint32_t)r;
}
// code k of the packed row `row`: bits [k b, (k + 1) b) of the row's bit string, bit i being bit i % 8 of byte i / 8.  The second
// byte is read only when the code reaches into it, and then it is a byte of the row: (k + 1) b <= z b <= 8 S.
__device__ __forceinline__ float codeb_load(const uint8_t *__restrict__ row, int k, int bits) {
    const int bit = k * bits, j = bit >> 3, sh = bit & 7;
    uint32_t w = row[j];
    if (sh + bits > 8) w |= (uint32_t)row[j + 1] << 8;
    return (float)((w >> sh) & ((1u << bits) - 1u));      // exact; padding bits are never part of a code
}
#endif

}  // namespace bamd
