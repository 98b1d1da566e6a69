// Fused PowerSGD (kernels/powersgd.hip): one power-iteration step of the low-rank gradient
// compression of Vogels et al. 2019 on a list of row-major matrices, the compressible gradients of
// one bucket. With M' = G + E (E the fp32 error memory, never written as a sum):
//   project          P = M' Q
//   orthonormalize   P <- P L^-T twice, L L^T = P^T P + (max(eps, 0) + 1e-10 max diag + 1e-30) I
//   backproject      Q = M'^T P
//   reconstruct      A = inv_world P Q^T rounded to the bucket dtype, E <- (G + E) - A, G <- A
// P [n, r], Q [m, r] and E are fp32 whatever the bucket dtype (fp32 / bf16 / fp16); 1 <= r <= 32.
#pragma once

#include <ATen/ATen.h>

#include <memory>
#include <vector>

namespace xddp {
namespace kernels {

// The launch tables and the partial-sum workspace of one list of matrices, built once: a step that
// reuses a plan allocates nothing and does no work on the host beyond the launches. The plan keeps
// its tensors alive. `errors` may be empty (no error feedback: E = 0 and is not written).
class PsgdPlan {
 public:
  PsgdPlan(const std::vector<at::Tensor>& mats, const std::vector<at::Tensor>& errors,
           const std::vector<at::Tensor>& ps, const std::vector<at::Tensor>& qs);
  ~PsgdPlan();
  void project();
  void backproject();
  void reconstruct(double inv_world);
  void orthonormalize_p(double epsilon);
  void orthonormalize_q(double epsilon);
  int64_t workspace_floats() const;

 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
};

// CholeskyQR2 of every [n, r] fp32 matrix of the list, in place (r <= min(n, 32))
void psgd_orthonormalize(const std::vector<at::Tensor>& mats, double epsilon);

}  // namespace kernels
}  // namespace xddp
