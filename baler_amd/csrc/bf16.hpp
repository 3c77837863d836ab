// The 16-bit MFMA inference modes: encode / decode / forward_loss of the 24-column AE with LDS-resident weights on
// v_mfma_f32_16x16x32_bf16 (BAMD_MODE_BF16) / _f16 (BAMD_MODE_F16), both bf16.hip, and at fp32 accuracy on three _f16 products per tile with
// every fp32 operand split into two binary16 values (BAMD_MODE_F16X3, f16x3.hip).  One state per handle (h->infer16_state) and one set
// of entry points (defined in bf16.hip); h->mode decides at infer16_setup whose kernels the state's ops launch (bf16_net.hpp).
#pragma once
#include "bamd_internal.hpp"

namespace bamd {
struct Infer16Ops;
bool bf16_has_kernels(const bamd_handle *h);     // this shape has a bf16 (and an f16) inference instantiation in bf16.hip
const Infer16Ops *f16x3_find_ops(const bamd_handle *h);   // the fp16x3 instantiation for this shape (f16x3.hip), or null
inline bool f16x3_has_kernels(const bamd_handle *h) { return f16x3_find_ops(h) != nullptr; }      // (the shapes of bf16_has_kernels)
int infer16_setup(bamd_handle *h);               // BAMD_ERR_UNSUPPORTED for shapes without an instantiation in h->mode
int infer16_pack(bamd_handle *h, hipStream_t s); // h->params (fp32) -> the mode's 16-bit fragments + fp32 bias fragments
void infer16_teardown(bamd_handle *h);
int infer16_encode(bamd_handle *h, const void *x, int x_dtype, int64_t n, const double *features, void *z, int z_dtype,
                   hipStream_t s);
int infer16_decode(bamd_handle *h, const void *z, int z_dtype, int64_t n, const double *features, const uint8_t *int_mask,
                   void *out, int out_dtype, hipStream_t s);
int infer16_forward_loss(bamd_handle *h, const void *x, int x_dtype, int64_t n, const double *features, void *recon,
                         int recon_dtype, double *loss_sum, hipStream_t s);
// bf16 training (bf16_train.hip): fwd + loss + bwd on bf16 MFMA for the shapes it is instantiated for
int bf16_train_setup(bamd_handle *h);            // leaves h->bf16_train_state null when the shape has no instantiation
void bf16_train_teardown(bamd_handle *h);
bool bf16_train_ok(const bamd_handle *h);
int bf16_train_pack(bamd_handle *h, hipStream_t s);   // h->params (fp32) -> the training kernels' bf16 fragments
int bf16_fwd_bwd(bamd_handle *h, const void *x, int x_dtype, int64_t n, const double *features, void *grads, hipStream_t s);
}  // namespace bamd
