// Weight-only MXFP4 linear for decode-sized batches:
//
//   out[M, N] = bf16(sum_k x[m, k] * e2m1(codes[n, k]) * 2^(scales[n, k / 32] - 127)),
//   x bf16, codes two e2m1 per byte (element 2 i in the low nibble of byte i),
//   scales one E8M0 byte per 32 consecutive k of a row (OCP microscaling).
//
// Every e2m1 value {0, 0.5, 1, 1.5, 2, 3, 4, 6} times a power of two is a
// bf16 value, so the kernel is a bf16 MFMA GEMM on exact operands with fp32
// accumulation. The scale belongs to a 32-k block, not to a row, so it cannot
// wait for the epilogue: it enters at the conversion, inside the k loop, and
// the epilogue does no scaling.
//
// linear_mxfp4w_kernel is a weight-streaming kernel. A workgroup owns two
// 32-row weight tiles (64 output features) and streams them from global
// memory once, straight into registers. Weight rows sit on M of
// v_mfma_f32_32x32x16_bf16, up to 32 tokens on N. The tokens' activations are
// staged through LDS in chunks of 512 k, double buffered, one barrier per
// chunk. The four waves split a chunk 2 by k x 2 by row tile: wave w takes
// k in [256 (w & 1), + 256) of tile w >> 1, which is one whole 128-byte line
// of each of its 32 rows, fetched by four 16-byte loads per lane, and keeps
// one accumulator. Lane (m, hi) of load j holds the 32 codes
// k = 64 j + 32 hi .. + 32 of row m: exactly one MX block, so one scale byte
// serves the load. Its four dwords are the A operands of four MFMA steps;
// dword d covers k + 8 d .. + 8, and the B fragments are read from LDS at the
// same k offsets, so A and B share one k order and nothing is shuffled. A
// dword becomes eight bf16 by four v_cvt_scalef32_pk_bf16_fp4 (byte selectors
// 0-3: low nibble first), which multiply by the block's scale on the way.
// That scale is the fp32 2^(byte - 127), built by shifting the byte into the
// exponent field (the quantiser keeps the byte in [2, 252], so it is a
// normal number); it is only ever relied on as a power of two. A wave's 256 k
// of a row are 8 consecutive scale bytes: each lane reads them as two dwords
// (both half-waves the same address, one fetch) and picks byte 2 j + hi.
// The next chunk's codes, scale bytes and up to 8 activation loads per lane
// are issued before the current chunk's MFMAs, so a wave keeps 4 KiB of codes
// in flight. K % 256 == 128 leaves half a line in the last chunk: its loads,
// its second scale dword and its MFMA steps are skipped load-uniformly. Token
// slots past M are zeroed in LDS once per token tile and are neither loaded
// nor stored afterwards. The two k-waves of a tile meet in LDS (aliasing the
// staging buffers) and are added in wave order.
//
// M > 32 loops over token tiles and re-reads the weight tile from L2. A
// workgroup whose second tile lies past N neither loads nor stores it; its
// two waves only stage activations.
//
// Split-K is chosen on the host from (M, N, K) alone (graph-safe): split z
// takes the chunks [z cps, (z + 1) cps) and writes fp32 partials [S, M, N];
// linear_mxfp4w_reduce_kernel adds them in split order and casts. No float
// atomics anywhere: two calls give the same bits.

#include <torch/extension.h>

#include <algorithm>
#include <cstdint>

#include "hip_common.h"

namespace {

constexpr int NT = 32;         // tokens per MFMA N tile
constexpr int KW = 256;        // k per wave per chunk: one 128-byte line of a weight row
constexpr int KC = 2 * KW;     // k per LDS chunk
constexpr int PITCH = KC + 8;  // LDS row pitch (1040 B = 65 x 16 B: conflict-free b128 reads)
constexpr int XL = KC * NT / (256 * 8);  // 16-byte activation loads per thread per chunk

// SPLIT = false: outp = out bf16 [M, N]. gridDim.y == 1.
// SPLIT = true : outp = part fp32 [gridDim.y, M, N].
template <bool SPLIT>
__global__ __launch_bounds__(256, 2) void linear_mxfp4w_kernel(
    const short* __restrict__ x, const unsigned char* __restrict__ codes,
    const unsigned char* __restrict__ scales, void* __restrict__ outp, int M, int N, int K,
    int cps) {
  __shared__ __attribute__((aligned(16))) short xs[2 * NT * PITCH];
  float* red = reinterpret_cast<float*>(xs);  // [4 waves][16][64] after the k loop
  static_assert(4 * 16 * 64 * sizeof(float) <= sizeof(short) * 2 * NT * PITCH,
                "reduction image must fit the staging buffers");

  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int ln = lane & 31, hi = lane >> 5;
  const int kw = w & 1, rt = w >> 1;  // this wave's k half of a chunk and its row tile
  const int rows0 = blockIdx.x * 64;
  const bool two = rows0 + 32 < N;  // N % 32 == 0: the second tile is whole or absent
  const bool mine = rt == 0 || two;  // wave-uniform: this wave has a weight tile
  const long long row = rows0 + 32 * rt + ln;
  // a row is K / 2 bytes of codes and K / 32 scale bytes
  const unsigned char* ap = codes + row * (K / 2) + kw * (KW / 2) + 16 * hi;
  const unsigned char* sp = scales + row * (K / 32) + kw * (KW / 32);
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
    // this wave's 256 k of chunk c: one 128-byte line of each weight row and
    // its 8 scale bytes. K % 128 == 0, so loads 2 j and 2 j + 1 (128 k, 4 scale
    // bytes) are both inside the row or both past it.
    auto load_w = [&](int c, u32x4(&wr)[4], unsigned int(&sr)[2]) {
      if (!mine) return;
      const int k = c * KC + kw * KW;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (k + 128 * h < K) {
          wr[2 * h] = *reinterpret_cast<const u32x4*>(ap + (long long)c * (KC / 2) + 64 * h);
          wr[2 * h + 1] =
              *reinterpret_cast<const u32x4*>(ap + (long long)c * (KC / 2) + 64 * h + 32);
          sr[h] = *reinterpret_cast<const unsigned int*>(sp + (long long)c * (KC / 32) + 4 * h);
        }
      }
    };

    f32x16 acc = {};
    u32x4 wcur[4] = {}, wnxt[4] = {};
    unsigned int scur[2] = {}, snxt[2] = {};
    s16x8 xr[XL];
    load_x(c0, xr);
    load_w(c0, wcur, scur);
    store_x(0, xr);
    __syncthreads();
    for (int c = c0; c < c1; ++c) {
      const int buf = (c - c0) & 1;
      const bool more = c + 1 < c1;
      if (more) {
        load_x(c + 1, xr);
        load_w(c + 1, wnxt, snxt);
      }
      if (mine) {
        const int k = c * KC + kw * KW;
        const short* bp = xs + (buf * NT + ln) * PITCH + kw * KW + 32 * hi;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (k + 64 * j < K) {
            // scale byte 2 j + hi of the wave's 8: 2^(byte - 127) as fp32
            const float sc =
                __uint_as_float(((scur[j >> 1] >> (16 * (j & 1) + 8 * hi)) & 0xffu) << 23);
#pragma unroll
            for (int d = 0; d < 4; ++d) {
              const s16x8 b = *reinterpret_cast<const s16x8*>(bp + 64 * j + 8 * d);
              acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(e2m1x8_to_bf16x8(wcur[j][d], sc), b,
                                                            acc, 0, 0, 0);
            }
          }
        }
      }
      if (more) store_x(buf ^ 1, xr);
      __syncthreads();
      if (more) {
#pragma unroll
        for (int j = 0; j < 4; ++j) wcur[j] = wnxt[j];
        scur[0] = snxt[0];
        scur[1] = snxt[1];
      }
    }

    // the two k-waves of each tile meet in LDS and are added in wave order
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(w * 16 + r) * 64 + lane] = acc[r];
    __syncthreads();
    // thread (n, q): token n, tile rows 8 (q >> 1) + 4 (q & 1) .. + 4, which
    // are registers 4 (q >> 1) .. + 4 of MFMA lane 32 (q & 1) + n
    const int n = tid & 31, q = tid >> 5;
    f32x4 s0, s1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * (q >> 1) + i, src = 32 * (q & 1) + n;
      s0[i] = red[(0 * 16 + r) * 64 + src] + red[(1 * 16 + r) * 64 + src];
      s1[i] = red[(2 * 16 + r) * 64 + src] + red[(3 * 16 + r) * 64 + src];
    }
    if (n < live) {
      const int m = rows0 + 8 * (q >> 1) + 4 * (q & 1);
      if (!SPLIT) {
        short* o = static_cast<short*>(outp) + (long long)(t0 + n) * N + m;
        s16x4 o0;
#pragma unroll
        for (int i = 0; i < 4; ++i) o0[i] = f2bf(s0[i]);
        *reinterpret_cast<s16x4*>(o) = o0;
        if (two) {
          s16x4 o1;
#pragma unroll
          for (int i = 0; i < 4; ++i) o1[i] = f2bf(s1[i]);
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

// out[t, c .. c + 8] = bf16(sum_s part[s, t, c .. c + 8])
__global__ __launch_bounds__(256) void linear_mxfp4w_reduce_kernel(
    const float* __restrict__ part, short* __restrict__ out, long long n_vec, int N, int S,
    long long MN) {
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
  s16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = f2bf(acc[j]);
  *reinterpret_cast<s16x8*>(out + t * N + c) = o;
}

}  // namespace

// x bf16 [M, K], codes uint8 [N, K / 2], scales uint8 [N, K / 32] -> out bf16 [M, N]
torch::Tensor linear_mxfp4w(torch::Tensor x, torch::Tensor codes, torch::Tensor scales) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.dtype() == torch::kBFloat16 &&
                  x.is_contiguous(),
              "linear_mxfp4w: x must be contiguous bf16 [M, K] on the GPU");
  const long long M = x.size(0), K = x.size(1);
  TORCH_CHECK(codes.is_cuda() && codes.dim() == 2 && codes.dtype() == torch::kUInt8 &&
                  codes.is_contiguous() && codes.size(1) * 2 == K,
              "linear_mxfp4w: codes must be contiguous uint8 [N, K / 2] on the GPU");
  const long long N = codes.size(0);
  TORCH_CHECK(scales.is_cuda() && scales.dim() == 2 && scales.dtype() == torch::kUInt8 &&
                  scales.is_contiguous() && scales.size(0) == N && scales.size(1) * 32 == K,
              "linear_mxfp4w: scales must be contiguous uint8 [N, K / 32] on the GPU");
  TORCH_CHECK(K >= 128 && K % 128 == 0 && N >= 32 && N % 32 == 0 && K < (1 << 24) &&
                  N < (1 << 24) && M < (1 << 24),
              "linear_mxfp4w: K must be a multiple of 128 and N a multiple of 32");
  // K % 128 == 0 makes every row of codes a multiple of 64 bytes and every row
  // of scales a multiple of 4, so aligned bases keep all loads aligned
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(codes.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(scales.data_ptr()) % 4 == 0,
              "linear_mxfp4w: operands must be 16-byte aligned (scales 4-byte)");
  auto out = torch::empty({M, N}, x.options());
  if (M == 0) return out;

  // Split k over workgroups until the grid gives about two workgroups per CU,
  // while the fp32 partials (written and read once) stay under a quarter of
  // the weight bytes N K / 2: 16 S M / K <= 1/4. A function of the shapes only.
  const int nc = (int)((K + KC - 1) / KC);
  const long long wgs = (N + 63) / 64;
  long long want = std::min<long long>((512 + wgs - 1) / wgs, K / (64 * M));
  want = std::max<long long>(1, std::min<long long>(want, nc));
  const int cps = (int)((nc + want - 1) / want);
  const int S = (nc + cps - 1) / cps;

  hipStream_t stream = hypha_stream();
  const short* xp = (const short*)x.data_ptr();
  const unsigned char* cp = (const unsigned char*)codes.data_ptr();
  const unsigned char* sp = (const unsigned char*)scales.data_ptr();
  if (S == 1) {
    hipLaunchKernelGGL(linear_mxfp4w_kernel<false>, dim3((unsigned)wgs, 1), dim3(256), 0,
                       stream, xp, cp, sp, out.data_ptr(), (int)M, (int)N, (int)K, cps);
    return out;
  }
  auto part = torch::empty({(long long)S, M, N}, x.options().dtype(torch::kFloat32));
  hipLaunchKernelGGL(linear_mxfp4w_kernel<true>, dim3((unsigned)wgs, (unsigned)S), dim3(256), 0,
                     stream, xp, cp, sp, part.data_ptr(), (int)M, (int)N, (int)K, cps);
  const long long n_vec = M * (N / 8);
  hipLaunchKernelGGL(linear_mxfp4w_reduce_kernel, dim3((unsigned)((n_vec + 255) / 256)),
                     dim3(256), 0, stream, part.data_ptr<float>(), (short*)out.data_ptr(), n_vec,
                     (int)N, S, M * N);
  return out;
}
