// Weight-only fp8 linear for decode-sized batches:
//
//   out[M, N] = bf16((x[M, K] . w8[N, K]^T) * scale[N]),
//   x bf16, w8 e4m3 codes (one byte per weight), scale fp32 per output row.
//
// Every finite e4m3 value is a bf16 value, so the kernel is a bf16 MFMA GEMM
// on exact operands with fp32 accumulation, followed by one fp32 multiply per
// output row; the scale never touches an element.
//
// linear_fp8w_kernel is a weight-streaming kernel (the shape moe_expert_kernel
// has, with the k geometry of 1-byte weights). A workgroup owns two 32-row
// weight tiles (64 output features) and streams them from global memory once,
// straight into registers. Weight rows sit on M of v_mfma_f32_32x32x16_bf16,
// up to 32 tokens on N. The tokens' activations are staged through LDS in
// chunks of 512 k, double buffered, one barrier per chunk. The four waves
// split every chunk by k: wave w takes k in [128 w, 128 w + 128), which is one
// whole 128-byte line of each of its 64 weight rows, fetched by four 16-byte
// loads per lane per tile. Lane (m, hi) of load j holds the 16 codes
// k = 32 j + 16 hi .. + 16: bytes 0-7 become the A operand of MFMA step 2 j,
// bytes 8-15 that of step 2 j + 1, and the B fragments are read from LDS at
// the same k offsets, so A and B share one k order and nothing is shuffled.
// Codes become bf16 in registers: v_cvt_pk_f32_fp8 gives two exact fp32, and
// one v_perm_b32 keeps their high halves (sign, subnormals and -0 included).
// The next chunk's 8 weight loads and up to 8 activation loads per lane are
// issued before the current chunk's MFMAs, so a wave keeps 8 KiB of weights in
// flight. Token slots past M are zeroed in LDS once per token tile and are
// neither loaded nor stored afterwards. The waves' partial accumulators meet
// in LDS (aliasing the staging buffers) and are added in wave order.
//
// M > 32 loops over token tiles and re-reads the weight tile from L2. A
// workgroup whose second tile lies past N neither loads nor stores it.
//
// Split-K is chosen on the host from (M, N, K) alone (graph-safe): split z
// takes the chunks [z cps, (z + 1) cps) and writes fp32 partials [S, M, N];
// linear_fp8w_reduce_kernel adds them in split order, applies the scale and
// casts. No float atomics anywhere: two calls give the same bits.

#include <torch/extension.h>

#include <algorithm>
#include <cstdint>

#include "hip_common.h"

namespace {

constexpr int NT = 32;         // tokens per MFMA N tile
constexpr int KW = 128;        // k per wave per chunk: one 128-byte line of a weight row
constexpr int KC = 4 * KW;     // k per LDS chunk
constexpr int PITCH = KC + 8;  // LDS row pitch (1040 B = 65 x 16 B: conflict-free b128 reads)
constexpr int XL = KC * NT / (256 * 8);  // 16-byte activation loads per thread per chunk

// SPLIT = false: outp = out bf16 [M, N], scaled. gridDim.y == 1.
// SPLIT = true : outp = part fp32 [gridDim.y, M, N], unscaled.
template <bool SPLIT>
__global__ __launch_bounds__(256, 2) void linear_fp8w_kernel(
    const short* __restrict__ x, const unsigned char* __restrict__ w8,
    const float* __restrict__ scale, void* __restrict__ outp, int M, int N, int K, int cps) {
  __shared__ __attribute__((aligned(16))) short xs[2 * NT * PITCH];
  float* red = reinterpret_cast<float*>(xs);  // [4 waves][2 tiles][16][64] after the k loop
  static_assert(4 * 2 * 16 * 64 * sizeof(float) <= sizeof(short) * 2 * NT * PITCH,
                "reduction image must fit the staging buffers");

  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int ln = lane & 31, hi = lane >> 5;
  const int rows0 = blockIdx.x * 64;
  const bool two = rows0 + 32 < N;  // N % 32 == 0: the second tile is whole or absent
  const unsigned char* a0 = w8 + (long long)(rows0 + ln) * K + w * KW + 16 * hi;
  const unsigned char* a1 = a0 + 32ll * K;
  const int nc = (K + KC - 1) / KC;
  const int c0 = blockIdx.y * cps;
  const int c1 = min(nc, c0 + cps);
  const int xk = lane * 8;  // staging: k inside the chunk; wave w stages slots w + 4 i

  for (int t0 = 0; t0 < M; t0 += NT) {
    const int live = min(NT, M - t0);  // token slots of this tile that exist
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      if (w + 4 * i >= live) {  // wave-uniform
        *reinterpret_cast<s16x8*>(xs + (w + 4 * i) * PITCH + xk) = s16x8{};
        *reinterpret_cast<s16x8*>(xs + (NT + w + 4 * i) * PITCH + xk) = s16x8{};
      }
    }
    const short* xrow = x + (long long)(t0 + w) * K + xk;
    auto load_x = [&](int c, s16x8(&xr)[XL]) {
      const int k = c * KC + xk;
#pragma unroll
      for (int i = 0; i < XL; ++i) {
        xr[i] = s16x8{};
        if (w + 4 * i < live && k < K)
          xr[i] = *reinterpret_cast<const s16x8*>(xrow + 4ll * i * K + c * KC);
      }
    };
    auto store_x = [&](int buf, const s16x8(&xr)[XL]) {
#pragma unroll
      for (int i = 0; i < XL; ++i)
        if (w + 4 * i < live)
          *reinterpret_cast<s16x8*>(xs + (buf * NT + w + 4 * i) * PITCH + xk) = xr[i];
    };
    // this wave's 128 k of chunk c: one 128-byte line of each weight row
    auto load_w = [&](int c, u32x4(&wr)[2][4]) {
      if (c * KC + w * KW < K) {  // K % 128 == 0, so a started line is whole
        const long long kb = (long long)c * KC;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          wr[0][j] = *reinterpret_cast<const u32x4*>(a0 + kb + 32 * j);
        if (two) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            wr[1][j] = *reinterpret_cast<const u32x4*>(a1 + kb + 32 * j);
        }
      }
    };

    f32x16 acc0 = {}, acc1 = {};
    u32x4 wcur[2][4] = {}, wnxt[2][4] = {};
    s16x8 xr[XL];
    load_x(c0, xr);
    load_w(c0, wcur);
    store_x(0, xr);
    __syncthreads();
    for (int c = c0; c < c1; ++c) {
      const int buf = (c - c0) & 1;
      const bool more = c + 1 < c1;
      if (more) {
        load_x(c + 1, xr);
        load_w(c + 1, wnxt);
      }
      if (c * KC + w * KW < K) {
        const short* bp = xs + (buf * NT + ln) * PITCH + w * KW + 16 * hi;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const s16x8 b0 = *reinterpret_cast<const s16x8*>(bp + 32 * j);
          const s16x8 b1 = *reinterpret_cast<const s16x8*>(bp + 32 * j + 8);
          acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              e4m3x8_to_bf16x8(wcur[0][j][0], wcur[0][j][1]), b0, acc0, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              e4m3x8_to_bf16x8(wcur[0][j][2], wcur[0][j][3]), b1, acc0, 0, 0, 0);
          if (two) {
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                e4m3x8_to_bf16x8(wcur[1][j][0], wcur[1][j][1]), b0, acc1, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                e4m3x8_to_bf16x8(wcur[1][j][2], wcur[1][j][3]), b1, acc1, 0, 0, 0);
          }
        }
      }
      if (more) store_x(buf ^ 1, xr);
      __syncthreads();
      if (more) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          wcur[0][j] = wnxt[0][j];
          wcur[1][j] = wnxt[1][j];
        }
      }
    }

    // the four waves' partial sums meet in LDS and are added in wave order
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      red[((w * 2 + 0) * 16 + r) * 64 + lane] = acc0[r];
      red[((w * 2 + 1) * 16 + r) * 64 + lane] = acc1[r];
    }
    __syncthreads();
    // thread (n, q): token n, tile rows 8 (q >> 1) + 4 (q & 1) .. + 4, which
    // are registers 4 (q >> 1) .. + 4 of MFMA lane 32 (q & 1) + n
    const int n = tid & 31, q = tid >> 5;
    f32x4 s0, s1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * (q >> 1) + i, src = 32 * (q & 1) + n;
      s0[i] = 0.f;
      s1[i] = 0.f;
#pragma unroll
      for (int ww = 0; ww < 4; ++ww) {
        s0[i] += red[((ww * 2 + 0) * 16 + r) * 64 + src];
        s1[i] += red[((ww * 2 + 1) * 16 + r) * 64 + src];
      }
    }
    if (n < live) {
      const int m = rows0 + 8 * (q >> 1) + 4 * (q & 1);
      if (!SPLIT) {
        short* o = static_cast<short*>(outp) + (long long)(t0 + n) * N + m;
        const f32x4 sc0 = *reinterpret_cast<const f32x4*>(scale + m);
        s16x4 o0;
#pragma unroll
        for (int i = 0; i < 4; ++i) o0[i] = f2bf(s0[i] * sc0[i]);
        *reinterpret_cast<s16x4*>(o) = o0;
        if (two) {
          const f32x4 sc1 = *reinterpret_cast<const f32x4*>(scale + m + 32);
          s16x4 o1;
#pragma unroll
          for (int i = 0; i < 4; ++i) o1[i] = f2bf(s1[i] * sc1[i]);
          *reinterpret_cast<s16x4*>(o + 32) = o1;
        }
      } else {
        float* y = static_cast<float*>(outp) + ((long long)blockIdx.y * M + t0 + n) * N + m;
        *reinterpret_cast<f32x4*>(y) = s0;
        if (two) *reinterpret_cast<f32x4*>(y + 32) = s1;
      }
    }
    __syncthreads();  // red aliases the next token tile's staging buffers
  }
}

// out[t, c .. c + 8] = bf16((sum_s part[s, t, c .. c + 8]) * scale[c .. c + 8])
__global__ __launch_bounds__(256) void linear_fp8w_reduce_kernel(
    const float* __restrict__ part, const float* __restrict__ scale, short* __restrict__ out,
    long long n_vec, int N, int S, long long MN) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_vec) return;
  const int nv = N / 8;
  const long long t = idx / nv;
  const int c = (int)(idx % nv) * 8;
  float acc[8] = {};
  for (int s = 0; s < S; ++s) {
    const float* y = part + (long long)s * MN + t * N + c;
    const f32x4 lo = *reinterpret_cast<const f32x4*>(y);
    const f32x4 hi = *reinterpret_cast<const f32x4*>(y + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[j] += lo[j];
      acc[4 + j] += hi[j];
    }
  }
  const f32x4 sl = *reinterpret_cast<const f32x4*>(scale + c);
  const f32x4 sh = *reinterpret_cast<const f32x4*>(scale + c + 4);
  s16x8 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    o[j] = f2bf(acc[j] * sl[j]);
    o[4 + j] = f2bf(acc[4 + j] * sh[j]);
  }
  *reinterpret_cast<s16x8*>(out + t * N + c) = o;
}

}  // namespace

// x bf16 [M, K], w8 e4m3 [N, K], scale fp32 [N] -> out bf16 [M, N]
torch::Tensor linear_fp8w(torch::Tensor x, torch::Tensor w8, torch::Tensor scale) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.dtype() == torch::kBFloat16 &&
                  x.is_contiguous(),
              "linear_fp8w: x must be contiguous bf16 [M, K] on the GPU");
  const long long M = x.size(0), K = x.size(1);
  TORCH_CHECK(w8.is_cuda() && w8.dim() == 2 && w8.dtype() == torch::kFloat8_e4m3fn &&
                  w8.is_contiguous() && w8.size(1) == K,
              "linear_fp8w: w8 must be contiguous e4m3 [N, K] on the GPU");
  const long long N = w8.size(0);
  TORCH_CHECK(scale.is_cuda() && scale.dim() == 1 && scale.dtype() == torch::kFloat32 &&
                  scale.is_contiguous() && scale.size(0) == N,
              "linear_fp8w: scale must be contiguous fp32 [N] on the GPU");
  TORCH_CHECK(K >= 128 && K % 128 == 0 && N >= 32 && N % 32 == 0 && K < (1 << 24) &&
                  N < (1 << 24) && M < (1 << 24),
              "linear_fp8w: K must be a multiple of 128 and N a multiple of 32");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(w8.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(scale.data_ptr()) % 16 == 0,
              "linear_fp8w: operands must be 16-byte aligned");
  auto out = torch::empty({M, N}, x.options());
  if (M == 0) return out;

  // Split k over workgroups until the grid gives about two workgroups per CU,
  // while the fp32 partials (written and read once) stay under a quarter of
  // the weight bytes: 8 S M / K <= 1/4. A function of the shapes only.
  const int nc = (int)((K + KC - 1) / KC);
  const long long wgs = (N + 63) / 64;
  long long want = std::min<long long>((512 + wgs - 1) / wgs, K / (32 * M));
  want = std::max<long long>(1, std::min<long long>(want, nc));
  const int cps = (int)((nc + want - 1) / want);
  const int S = (nc + cps - 1) / cps;

  hipStream_t stream = hypha_stream();
  const short* xp = (const short*)x.data_ptr();
  const unsigned char* wp = (const unsigned char*)w8.data_ptr();
  const float* sp = scale.data_ptr<float>();
  if (S == 1) {
    hipLaunchKernelGGL(linear_fp8w_kernel<false>, dim3((unsigned)wgs, 1), dim3(256), 0, stream,
                       xp, wp, sp, out.data_ptr(), (int)M, (int)N, (int)K, cps);
    return out;
  }
  auto part = torch::empty({(long long)S, M, N}, x.options().dtype(torch::kFloat32));
  hipLaunchKernelGGL(linear_fp8w_kernel<true>, dim3((unsigned)wgs, (unsigned)S), dim3(256), 0,
                     stream, xp, wp, sp, part.data_ptr(), (int)M, (int)N, (int)K, cps);
  const long long n_vec = M * (N / 8);
  hipLaunchKernelGGL(linear_fp8w_reduce_kernel, dim3((unsigned)((n_vec + 255) / 256)),
                     dim3(256), 0, stream, part.data_ptr<float>(), sp, (short*)out.data_ptr(),
                     n_vec, (int)N, S, M * N);
  return out;
}
