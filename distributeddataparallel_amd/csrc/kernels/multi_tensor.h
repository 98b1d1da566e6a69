// Host-side API of the multi-tensor HIP kernels (gfx950).
//
// These replace the per-parameter ATen launches of the reference stack's DDP hot path
// (SURVEY.md §2.6 K12 `reducer::mul_out`, K13 `copy_bucket_to_grad`, K14 buffer
// pack/unpack, K15 `_foreach_add_`, K19 NaN check) with one launch per tensor list.
#pragma once

#include <ATen/ATen.h>
#include <c10/util/Optional.h>
#include <hip/hip_runtime.h>

#include <vector>

namespace xddp {
namespace kernels {

// dst[i] = cast(src[i] * scale * (*scale_ptr if given)). src[i]/dst[i] must have equal numel and
// be dense in the same memory order (checked). All srcs share one dtype, all dsts share one.
void mt_scale_copy(const std::vector<at::Tensor>& src, const std::vector<at::Tensor>& dst, double scale,
                   const c10::optional<at::Tensor>& scale_tensor, hipStream_t stream);

// Pack a list of dense tensors into consecutive slices of `flat` at `offsets` (elements) and back.
// Raw byte copies (dtype-agnostic, bit-exact) of up to any number of (src, dst, nbytes) regions.
void mt_copy_bytes(const std::vector<const void*>& src, const std::vector<void*>& dst,
                   const std::vector<int64_t>& nbytes, hipStream_t stream);
void mt_pack(const std::vector<at::Tensor>& src, const at::Tensor& flat, const std::vector<int64_t>& offsets,
             double scale, hipStream_t stream);
void mt_unpack(const at::Tensor& flat, const std::vector<int64_t>& offsets, const std::vector<at::Tensor>& dst,
               double scale, hipStream_t stream);

// out[0] = total L2 norm of all elements of all tensors (device scalar), summed in fp32 (fp64 tensors:
// in fp64, so squares beyond fp32's range do not overflow). out[1] = the clip coefficient
// min(1, max_norm / (out[0] + 1e-6)) if max_norm > 0, else 1. `out` must be a float32 tensor with
// >= 2 elements.
void mt_l2norm(const std::vector<at::Tensor>& tensors, const at::Tensor& out, double max_norm, hipStream_t stream);

// out[0] (int32) becomes 1 if any element of any tensor is NaN/Inf; 0 otherwise (zeroed here). fp64
// tensors are tested as fp64: a finite value beyond fp32's range is finite.
void mt_nonfinite(const std::vector<at::Tensor>& tensors, const at::Tensor& out, hipStream_t stream);

// Replica checksum of a list of dense device tensors (any dtypes): float64 [3] = (fp64 sum of the
// values, low / high 32 bits of an XOR of per-element position-mixed raw-bit hashes). Bit-equal
// inputs give bit-equal outputs (fixed-order merge); the DDP replica check compares it across ranks.
at::Tensor mt_checksum(const std::vector<at::Tensor>& tensors, hipStream_t stream);

// Fused SGD over a tensor list (torch.optim.SGD semantics).
void fused_sgd_master(const std::vector<at::Tensor>& masters, const std::vector<at::Tensor>& grads,
                      const std::vector<at::Tensor>& momentum_bufs, const std::vector<at::Tensor>& model_params,
                      double lr, double momentum, double dampening, double weight_decay, bool nesterov, bool maximize,
                      bool first_step, const c10::optional<at::Tensor>& grad_scale, hipStream_t stream);
void fused_sgd(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
               const std::vector<at::Tensor>& momentum_bufs, double lr, double momentum, double dampening,
               double weight_decay, bool nesterov, bool maximize, bool first_step,
               const c10::optional<at::Tensor>& grad_scale, hipStream_t stream);

// Fused Adam/AdamW over a tensor list (torch.optim.AdamW / Adam semantics, no amsgrad).
// If `masters` is non-empty, fp32 master weights are updated and params receive the cast.
void fused_adam(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
                const std::vector<at::Tensor>& exp_avgs, const std::vector<at::Tensor>& exp_avg_sqs,
                const std::vector<at::Tensor>& masters, double lr, double beta1, double beta2, double eps,
                double weight_decay, int64_t step, bool decoupled, bool maximize,
                const c10::optional<at::Tensor>& grad_scale, hipStream_t stream);

// fused_adam with 8-bit moments: per parameter (or 128-aligned range of one) uint8 e4m3 codes of
// exp_avg and of sqrt(exp_avg_sq) (numel each, memory order) and one fp32 scale per 128 elements
// (= group max / 448). The moments are dequantised, updated exactly as in fused_adam, and
// re-quantised with stochastic rounding whose random bits hash (seed, ordinals[i], step, element
// index within the parameter = group_offsets[i] * 128 + position, moment). A range must start at a
// group boundary of its parameter and may end short only at the parameter's end. With
// `stochastic_params` (bf16 parameters, no masters) the parameters are written with the rounding of
// stochastic_round_bf16, keyed by the same tuple.
void fused_adam8(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
                 const std::vector<at::Tensor>& m_q, const std::vector<at::Tensor>& m_scale,
                 const std::vector<at::Tensor>& s_q, const std::vector<at::Tensor>& s_scale,
                 const std::vector<at::Tensor>& masters, const std::vector<int64_t>& ordinals,
                 const std::vector<int64_t>& group_offsets, double lr, double beta1, double beta2, double eps,
                 double weight_decay, int64_t step, int64_t seed, bool decoupled, bool maximize,
                 const c10::optional<at::Tensor>& grad_scale, bool stochastic_params, hipStream_t stream);

// out (bf16) = x (fp32, dense, same memory order) rounded stochastically: per element the upper half
// of bits(x) + r, r the top 16 bits of a hash of (seed, ordinal, step, offset + index in memory
// order); a finite value saturates instead of becoming inf, +-inf stay, NaN gives 0x7fc0.
void stochastic_round_bf16(const at::Tensor& x, const at::Tensor& out, int64_t seed, int64_t ordinal, int64_t step,
                           int64_t offset, hipStream_t stream);

// fused_adam for bf16 parameters without masters (fp32 moments), the parameters written with the
// rounding of stochastic_round_bf16 keyed by (seed, ordinals[i], step, offsets[i] + position):
// offsets[i] is the element offset of the i-th range within its parameter.
void fused_adam_sr(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
                   const std::vector<at::Tensor>& exp_avgs, const std::vector<at::Tensor>& exp_avg_sqs,
                   const std::vector<int64_t>& ordinals, const std::vector<int64_t>& offsets, double lr, double beta1,
                   double beta2, double eps, double weight_decay, int64_t step, int64_t seed, bool decoupled,
                   bool maximize, const c10::optional<at::Tensor>& grad_scale, hipStream_t stream);

// Layer-wise trust-ratio optimizers. Both return the fp32 [N] device tensor of the step's per-tensor
// ratios (1 for a zero-numel tensor, and where a norm is exactly zero; a non-finite norm is not
// masked). All norms are L2 over one whole tensor, of w = the fp32 master (if `masters` is
// non-empty; the parameter then receives the rounded master) or the parameter. Three stream-ordered
// launches per segment table, no host synchronisation; scratch comes from at::empty.
//
// LAMB: m, v as Adam on g' = g * grad_scale * (maximize ? -1 : 1);
//   u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + weight_decay * w   (bc = 1 without bias_correction)
//   w -= lr * r * u,  r = |w| / |u| if `adapt`, else 1.
at::Tensor fused_lamb(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
                      const std::vector<at::Tensor>& exp_avgs, const std::vector<at::Tensor>& exp_avg_sqs,
                      const std::vector<at::Tensor>& masters, double lr, double beta1, double beta2, double eps,
                      double weight_decay, int64_t step, bool bias_correction, bool adapt, bool maximize,
                      const c10::optional<at::Tensor>& grad_scale, hipStream_t stream);

// LARS: lam = trust_coefficient * |w| / (|g'| + weight_decay * |w| + eps), then torch.optim.SGD on
// d = lam * (g' + weight_decay * w). |g'| is |grad_scale| * |g|.
at::Tensor fused_lars(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
                      const std::vector<at::Tensor>& momentum_bufs, const std::vector<at::Tensor>& masters, double lr,
                      double momentum, double dampening, double weight_decay, bool nesterov, bool maximize,
                      bool first_step, double trust_coefficient, double eps,
                      const c10::optional<at::Tensor>& grad_scale, hipStream_t stream);

}  // namespace kernels
}  // namespace xddp
