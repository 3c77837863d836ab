// valu_beside_mfma_probe.hip for the fp16 inference mode: what does ONE extra instruction cost a wave that issues
// v_mfma_f32_16x16x32_f16 back to back -- for the instructions of the two candidate epilogues of bf16.hip's binary16 kernels?
//   (a) v_cvt_pk_f16_f32, then v_pk_mul_f16 + v_pk_maximum3_f16 on the packed pair           (1.5 VALU instructions per value)
//   (b) v_mul_f32 + v_maximum3_f32 per value as the bf16 kernels do, then v_cvt_pk_f16_f32   (2.5 per value)
// Loop body: 4 MFMAs (independent accumulators) + K instructions of one type on registers the MFMAs do not touch; cycles per MFMA
// slot by s_memtime, K = 0, 1, 2, 4, with one and with two waves per SIMD (the inference kernels run two).
// hipcc --offload-arch=gfx950 -O3 -o valu_f16_probe tools/probe/valu_beside_f16_mfma_probe.hip && ./valu_f16_probe
#include <hip/hip_runtime.h>
#include <cstdio>
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
using v4 = float __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));

template <int OP> __device__ __forceinline__ void op(float &x, float &y, v2f &p, v2f &q, unsigned &u, unsigned &w) {
    if (OP == 0) asm volatile("v_mul_f32 %0, %0, %1" : "+v"(x) : "v"(y));
    if (OP == 1) asm volatile("v_maximum3_f32 %0, %0, %1, %1" : "+v"(x) : "v"(y));
    if (OP == 2) asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(u) : "v"(x), "v"(y));
    if (OP == 3) asm volatile("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(u) : "v"(x), "v"(y));
    if (OP == 4) asm volatile("v_pk_mul_f16 %0, %0, %1" : "+v"(u) : "v"(w));
    if (OP == 5) asm volatile("v_pk_maximum3_f16 %0, %0, %1, %1" : "+v"(u) : "v"(w));
    if (OP == 6) asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(p) : "v"(q));
    if (OP == 7) asm volatile("s_nop 0");
}
template <int OP, int K, int NM>
__global__ void probe(unsigned long long *out, int iters, float seed) {
    const int lane = threadIdx.x & 63;
    h8 a, b;
    for (int e = 0; e < 8; ++e) { a[e] = (_Float16)(0.001f * (lane + e) + seed); b[e] = (_Float16)(0.002f * (lane - e)); }
    v4 c[4];
    for (int i = 0; i < 4; ++i) c[i] = (v4){0.f, 0.f, 0.f, 0.f};
    float x = seed + lane, y = 0.99f;
    v2f p = {x, y}, q = {0.5f, 0.25f};
    unsigned u = 0x3c003c00u + lane, w = 0x3bff3bffu;      // packed binary16 pairs near 1.0
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int i = 0; i < NM; ++i) {
                asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(c[i & 3]) : "v"(a), "v"(b));
#pragma unroll
                for (int k = 0; k < K; ++k) op<OP>(x, y, p, q, u, w);
            }
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    float s = x + p[0] + q[1] + (float)u;
    for (int i = 0; i < 4; ++i) s += c[i][0];
    if (s == 12345.678f) out[1] = 1;
    if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = t1 - t0;
}
template <int OP, int K, int NM> double run(unsigned long long *d, int threads) {
    const int iters = 2000;
    hipLaunchKernelGGL((probe<OP, K, NM>), dim3(256), dim3(threads), 0, 0, d, iters, 0.5f);
    hipLaunchKernelGGL((probe<OP, K, NM>), dim3(256), dim3(threads), 0, 0, d, iters, 0.5f);
    if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); exit(1); }
    unsigned long long t;
    hipMemcpy(&t, d, 8, hipMemcpyDeviceToHost);
    return (double)t / (iters * 4.0 * NM);          // cycles per MFMA slot
}
const char *names[] = {"v_mul_f32", "v_maximum3_f32", "v_cvt_pk_bf16_f32", "v_cvt_pk_f16_f32", "v_pk_mul_f16", "v_pk_maximum3_f16",
                       "v_pk_mul_f32", "s_nop 0"};
template <int OP> void row(unsigned long long *d) {
    for (int threads : {256, 512}) {
        const double k0 = run<OP, 0, 4>(d, threads), k1 = run<OP, 1, 4>(d, threads), k2 = run<OP, 2, 4>(d, threads), k4 = run<OP, 4, 4>(d, threads);
        printf("%-20s %d waves/SIMD: cycles per MFMA slot with 0 / 1 / 2 / 4 of them per MFMA: %6.1f %6.1f %6.1f %6.1f   -> %5.1f per instruction (from 4)\n",
               names[OP], threads / 256, k0, k1, k2, k4, (k4 - k0) / 4);
    }
}
int main() {
    unsigned long long *d;
    if (hipMalloc(&d, 64) != hipSuccess) { printf("hipMalloc failed\n"); return 1; }
    printf("beside v_mfma_f32_16x16x32_f16:\n");
    row<0>(d); row<1>(d); row<2>(d); row<3>(d); row<4>(d); row<5>(d); row<6>(d); row<7>(d);
    return 0;
}
