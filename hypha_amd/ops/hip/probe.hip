// MFMA fragment-layout probes: tiny single-wave GEMMs used by GPU tests to
// verify the lane->element maps this codebase assumes (guide §3 + G9:
// asymmetric-B transpose-detecting checks).
//
// Assumed maps (gfx950):
//   v_mfma_f32_32x32x16_bf16: A[m][k]: m=l&31, k=8*(l>>5)+j (j=0..7)
//                             B[k][n]: n=l&31, k=8*(l>>5)+j
//                             D[m][n]: n=l&31, m=(r&3)+8*(r>>2)+4*(l>>5), r=0..15
//   v_mfma_f32_16x16x32_bf16: A[m][k]: m=l&15, k=8*(l>>4)+j
//                             B[k][n]: n=l&15, k=8*(l>>4)+j
//                             D[m][n]: n=l&15, m=(l>>4)*4+r, r=0..3

#include <torch/extension.h>

#include "hip_common.h"

__global__ void probe32_kernel(const short* __restrict__ a, const short* __restrict__ b,
                               float* __restrict__ d) {
  const int l = threadIdx.x;  // one wave
  s16x8 af, bf;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int k = 8 * (l >> 5) + j;
    af[j] = a[(l & 31) * 16 + k];
    bf[j] = b[k * 32 + (l & 31)];
  }
  f32x16 acc = {};
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int m = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
    d[m * 32 + (l & 31)] = acc[r];
  }
}

__global__ void probe16_kernel(const short* __restrict__ a, const short* __restrict__ b,
                               float* __restrict__ d) {
  const int l = threadIdx.x;
  s16x8 af, bf;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int k = 8 * (l >> 4) + j;
    af[j] = a[(l & 15) * 32 + k];
    bf[j] = b[k * 16 + (l & 15)];
  }
  f32x4 acc = {};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int m = (l >> 4) * 4 + r;
    d[m * 16 + (l & 15)] = acc[r];
  }
}

// An accumulator tile as the next MFMA's B operand: X = M1 * M2 (32x16 by
// 16x32) stays in the 16 accumulator registers (rows in registers, column on
// the lane); registers 8s .. 8s+7 packed to bf16 are the B fragment of k-step
// s of Y = A * X (A 32x32), whose k order inside a step is permuted: element
// j of lane half h is row 16s + 8(j>>2) + 4h + (j&3) of X, so A is read in
// that order. The attention backward feeds P and dS to its dV^T and dK^T
// products this way.
__global__ void probe_acc_operand_kernel(const short* __restrict__ a,
                                         const short* __restrict__ m1,
                                         const short* __restrict__ m2,
                                         float* __restrict__ y) {
  const int l = threadIdx.x;  // one wave
  const int h = l >> 5, n = l & 31;
  s16x8 af, bf;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    af[j] = m1[n * 16 + 8 * h + j];
    bf[j] = m2[(8 * h + j) * 32 + n];
  }
  f32x16 x = {};
  x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, x, 0, 0, 0);
  f32x16 acc = {};
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    s16x8 xa, xb;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      xb[j] = f2bf(x[8 * s + j]);
      xa[j] = a[n * 32 + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3)];
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa, xb, acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) y[((r & 3) + 8 * (r >> 2) + 4 * h) * 32 + n] = acc[r];
}

torch::Tensor mfma_probe_32x32x16(torch::Tensor a, torch::Tensor b) {
  TORCH_CHECK(a.sizes() == torch::IntArrayRef({32, 16}) &&
              b.sizes() == torch::IntArrayRef({16, 32}));
  TORCH_CHECK(a.dtype() == torch::kBFloat16 && a.is_contiguous() && b.is_contiguous());
  auto d = torch::empty({32, 32}, a.options().dtype(torch::kFloat32));
  hipLaunchKernelGGL(probe32_kernel, dim3(1), dim3(64), 0, hypha_stream(),
                     (const short*)a.data_ptr(), (const short*)b.data_ptr(),
                     d.data_ptr<float>());
  return d;
}

torch::Tensor mfma_probe_16x16x32(torch::Tensor a, torch::Tensor b) {
  TORCH_CHECK(a.sizes() == torch::IntArrayRef({16, 32}) &&
              b.sizes() == torch::IntArrayRef({32, 16}));
  auto d = torch::empty({16, 16}, a.options().dtype(torch::kFloat32));
  hipLaunchKernelGGL(probe16_kernel, dim3(1), dim3(64), 0, hypha_stream(),
                     (const short*)a.data_ptr(), (const short*)b.data_ptr(),
                     d.data_ptr<float>());
  return d;
}

torch::Tensor mfma_probe_acc_operand(torch::Tensor a, torch::Tensor m1, torch::Tensor m2) {
  auto ok = [](const torch::Tensor& t, int r, int c) {
    return t.is_cuda() && t.dtype() == torch::kBFloat16 && t.is_contiguous() &&
           t.sizes() == torch::IntArrayRef({r, c});
  };
  TORCH_CHECK(ok(a, 32, 32) && ok(m1, 32, 16) && ok(m2, 16, 32),
              "mfma_probe_acc_operand: a [32,32], m1 [32,16], m2 [16,32], bf16 on the GPU");
  auto y = torch::empty({32, 32}, a.options().dtype(torch::kFloat32));
  hipLaunchKernelGGL(probe_acc_operand_kernel, dim3(1), dim3(64), 0, hypha_stream(),
                     (const short*)a.data_ptr(), (const short*)m1.data_ptr(),
                     (const short*)m2.data_ptr(), y.data_ptr<float>());
  return y;
}
