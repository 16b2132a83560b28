// Backward of a bias-free linear y = x @ weight^T with the weight gradient
// written straight into its destination (the parameter's slice of the flat
// gradient buffer) by the GEMM itself.
//
// Autograd's own backward computes dw into a temporary and AccumulateGrad
// then runs grad += dw: three more passes over every weight per step, into a
// buffer that a fourth pass had to zero. Here the wgrad GEMM's output IS the
// grad slice for the first write of a step (beta 0: nothing to zero
// beforehand). A later write in the same step (a module used twice) adds a
// dw of its own to it, as autograd does. Letting that GEMM accumulate with
// beta 1 would save the temporary but round once less than autograd, and
// training would no longer reproduce autograd's parameters bit for bit
// (measured: 3.9e-5 max abs after two steps of a twice-used 64x64 linear).
//
// No kernel of our own: both GEMMs are the ATen calls autograd's mm backward
// issues for linear's forward x.mm(weight.t()), in the same operand forms, so
// the library picks the same (tuned) algorithms:
//   dx = dy.mm(weight)                          the "nn" form
//   dw = dy.t().mm(x)                           the "nt" form, [N, K] row-major

#include <torch/extension.h>

#include <ATen/ops/mm.h>

// dy [T, N], x [T, K], weight [N, K] -> (dx [T, K] or undefined, dw).
// dw_out given: a contiguous [N, K] tensor of weight's dtype; it receives
// dw (accumulate false) or dw_out + dw (accumulate true) and is returned.
// dw_out absent: dw is a new tensor.
std::tuple<torch::Tensor, torch::Tensor> linear_bwd(torch::Tensor dy, torch::Tensor x,
                                                    torch::Tensor weight,
                                                    std::optional<torch::Tensor> dw_out,
                                                    bool accumulate, bool need_dx) {
  TORCH_CHECK(dy.dim() == 2 && x.dim() == 2 && weight.dim() == 2 &&
                  dy.size(0) == x.size(0) && dy.size(1) == weight.size(0) &&
                  x.size(1) == weight.size(1),
              "linear_bwd: need dy [T, N], x [T, K], weight [N, K]");
  TORCH_CHECK(dy.dtype() == weight.dtype() && x.dtype() == weight.dtype() &&
                  dy.device() == weight.device() && x.device() == weight.device(),
              "linear_bwd: dy, x and weight must share dtype and device");
  torch::Tensor dx;
  if (need_dx) dx = at::mm(dy, weight);
  if (!dw_out.has_value()) return {dx, at::mm(dy.t(), x)};
  torch::Tensor& out = *dw_out;
  TORCH_CHECK(out.sizes() == weight.sizes() && out.dtype() == weight.dtype() &&
                  out.device() == weight.device() && out.is_contiguous(),
              "linear_bwd: dw_out must be a contiguous tensor like weight");
  if (accumulate)
    out.add_(at::mm(dy.t(), x));  // autograd's own sum: both terms rounded to bf16 first
  else
    at::mm_out(out, dy.t(), x);  // beta 0: out's old contents are never read
  return {dx, out};
}
