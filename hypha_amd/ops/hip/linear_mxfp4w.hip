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
//
// MXFP8 activations (linear_mxfp4w_a8): the same weights against activations
// quantised to OCP MXFP8, e4m3 codes with one E8M0 byte per 32 k of a token,
//
//   out[M, N] = bf16(sum_k xq[m, k] * 2^(xe[m, k / 32] - 127)
//                          * e2m1(codes[n, k]) * 2^(scales[n, k / 32] - 127)).
//
// quantize_mxfp8_kernel makes xq and xe from bf16 rows. A block is 64 bytes of
// bf16: the four lanes of a quad load 16 bytes each, take the largest
// magnitude as an integer maximum of the bf16 bits (two cross-lane steps inside
// the quad), and read the scale off its exponent field: byte = max(2, field -
// 8), which is e = floor(log2(amax)) - 8 clamped below at -125 (a bf16 exponent
// cannot reach the upper clamp). x * 2^-e is exact in fp32, is clamped to
// +-448 and rounded to e4m3 by v_cvt_pk_fp8_f32 (nearest even). A lane stores
// its 8 codes as one 8-byte store, lane 0 of the quad the scale byte.
//
// linear_mxfp4w_a8_kernel<SPLIT, DEPTH> keeps linear_mxfp4w_kernel's geometry
// (two row tiles, waves 2 by k x 2 by row tile, one 128-byte line of a row per
// wave and chunk, the k-waves meeting in LDS, the same split-K and reduce) and
// replaces its inner loop by v_mfma_scale_f32_32x32x64_f8f6f4. That
// instruction takes, per lane (i, hi), 32 k of row i of each operand and one
// E8M0 byte per lane and operand, which scales the k block 32 hi .. + 32 of
// that row. The two formats sit differently in the lanes (measured on the
// device; the exact tests pin it). With cbsz:4 the A operand is 32 e2m1 codes
// in 4 VGPRs, k = 32 hi .. + 32 in order, element 2 i in the low nibble of
// byte i: load j of a lane, exactly as it arrives from global memory. The e4m3
// operand is 8 VGPRs in two halves of 16 bytes, k = 16 hi .. + 16 and
// k = 32 + 16 hi .. + 16, so a lane holds half of each of the two blocks and
// its scale byte serves its own half of block hi and the other half-wave's. Its scale is byte 2 j + hi of the
// wave's two scale dwords; the instruction picks the byte of the scale VGPR by
// an immediate, so each dword is shifted right by 8 hi and bytes 0 and 2 are
// selected. So a wave issues four MFMAs per chunk where the sibling issues
// sixteen MFMAs and sixteen conversions, and holds no conversion temporaries.
// The B operand is the token's e4m3 bytes at 64 j + 16 hi and 64 j + 32 + 16 hi,
// two 16-byte LDS reads; its scale byte is the token's block 2 j + hi of the
// wave's 8, read as one 8-byte LDS load per chunk and shifted the same way.
// LDS: a token's row of a chunk is its 512 code bytes followed by its 16 scale
// bytes, pitch 528 B = 33 x 16 B, two buffers of 32 rows: 33792 B. Lane
// (ln, hi) reads the 16 bytes at 528 ln + 256 kw + 64 j + 16 hi (+ 32): over
// 16 consecutive lanes, which a 128-bit read serves in one pass, the 16-byte
// slot index is 33 ln + const = ln + const (mod 16), so the sixteen reads fall
// in sixteen different 16-byte columns of the 256-byte bank row: no conflict.
// Staging writes 16 bytes per lane to consecutive addresses of one row.
// Token slots past M hold zero codes under the scale 0x7f (2^0): they are
// written once per token tile and neither loaded nor stored afterwards.
// Codes and scale dwords of the weights are loaded DEPTH chunks ahead into
// DEPTH + 1 register sets addressed by constants (moe_expert_mxfp4w_kernel's
// scheme, and its reason: the loads carry no branch, so the compiler can count
// them and wait for the oldest set only). A half line past the row
// (K % 256 == 128) or a chunk past the split re-reads the row's first 64
// bytes and first scale dword; its MFMAs are skipped. A wave whose row tile
// is absent (N % 64 == 32) has no rows of its own to read or store: its loads
// re-read tile 0's lines, which its sibling wave fetches at the same time,
// and it issues no MFMA. The activation loads are branch-free in the same way.
// The wave index goes through readfirstlane so that the tail conditions and
// chunk offsets are scalar.
// Registers decide depth against occupancy: DEPTH 1 is 144 / 146 VGPR and runs
// 3 waves/SIMD, DEPTH 2 is 180 / 182 and runs 2 (both 0 scratch; 128 VGPR for
// 4 waves spills). Measured on Llama-3-8B's shapes, DEPTH 1 is the faster or
// equal one at M <= 32 (by up to 17 % on gate/up at M = 1 and 8) and DEPTH 2
// by 1 - 3 % at M >= 64 on gate/up and head: DEPTH 1 is the default
// (profiles/linear_mxfp4w_a8.md, section 3).

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

// ---- MXFP8 activations --------------------------------------------------------

// x bf16 [n_vec * 8] -> q e4m3 [n_vec * 8], e E8M0 [n_vec / 4]; thread = 8
// elements, quad = one block of 32. n_vec % 4 == 0: a quad is whole or absent.
__global__ __launch_bounds__(256) void quantize_mxfp8_kernel(const short* __restrict__ x,
                                                             unsigned char* __restrict__ q,
                                                             unsigned char* __restrict__ e,
                                                             long long n_vec) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_vec) return;
  const s16x8 v = *reinterpret_cast<const s16x8*>(x + 8 * idx);
  int amax = 0;  // finite bf16 magnitudes order as their bits do
#pragma unroll
  for (int i = 0; i < 8; ++i) amax = max(amax, v[i] & 0x7fff);
  amax = max(amax, __shfl_xor(amax, 1, 64));
  amax = max(amax, __shfl_xor(amax, 2, 64));
  const int byte = max(2, (amax >> 7) - 8);
  // 2^(127 - byte): field 254 - byte in [8, 252], a normal fp32
  const float inv = __uint_as_float((unsigned int)(254 - byte) << 23);
  float f[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = fminf(fmaxf(bf2f(v[i]) * inv, -448.f), 448.f);
  u32x2 o;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    int d = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * h], f[4 * h + 1], 0, false);
    d = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * h + 2], f[4 * h + 3], d, true);
    o[h] = (unsigned int)d;
  }
  *reinterpret_cast<u32x2*>(q + 8 * idx) = o;
  if ((idx & 3) == 0) e[idx >> 2] = (unsigned char)byte;
}

constexpr int XP = KC + 16;  // LDS row of a token: 512 e4m3 codes, then 16 scale bytes
#ifndef HYPHA_MXFP4W_A8_DEPTH
#define HYPHA_MXFP4W_A8_DEPTH 1
#endif

// SPLIT as in linear_mxfp4w_kernel. xq e4m3 [M, K], xe E8M0 [M, K / 32].
template <bool SPLIT, int DEPTH>
__global__ __launch_bounds__(256, DEPTH == 1 ? 3 : 2) void linear_mxfp4w_a8_kernel(
    const unsigned char* __restrict__ xq, const unsigned char* __restrict__ xe,
    const unsigned char* __restrict__ codes, const unsigned char* __restrict__ scales,
    void* __restrict__ outp, int M, int N, int K, int cps) {
  static_assert(DEPTH >= 1 && DEPTH <= 3, "prefetch depth");
  constexpr int NS = DEPTH + 1;  // register sets: the chunk in use and DEPTH in flight
  __shared__ __attribute__((aligned(16))) unsigned char xs[2 * NT * XP];
  float* red = reinterpret_cast<float*>(xs);  // [4 waves][16][64] after the k loop
  static_assert(4 * 16 * 64 * sizeof(float) <= 2 * NT * XP,
                "reduction image must fit the staging buffers");

  const int tid = threadIdx.x;
  // the wave index through readfirstlane: what follows from it (k half, row
  // tile, every tail condition, the chunk offsets) then lives in SGPRs
  const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ln = lane & 31, hi = lane >> 5;
  const int kw = w & 1, rt = w >> 1;  // this wave's k half of a chunk and its row tile
  const int rows0 = blockIdx.x * 64;
  const bool two = rows0 + 32 < N;  // N % 32 == 0: the second tile is whole or absent
  const bool mine = rt == 0 || two;  // wave-uniform: this wave has a weight tile
  const int nb = K / 32;  // scale bytes of a row
  // every global address is a wave-uniform 64-bit base plus a 32-bit lane
  // offset that never changes, so a lane keeps one VGPR per stream of loads
  const unsigned char* ap = codes + (long long)rows0 * (K / 2);
  const unsigned char* sp = scales + (long long)rows0 * nb;
  const unsigned int arow = (unsigned int)((mine ? 32 * rt : 0) + ln);
  const unsigned int aoff = arow * (unsigned int)(K / 2) + 16 * hi, soff = arow * nb;
  const int nc = (K + KC - 1) / KC;
  const int c0 = blockIdx.y * cps;
  const int c1 = min(nc, c0 + cps);
  // staging: half-wave (w, hi) takes the token slots 2 w + hi + 8 i, lane ln
  // bytes 16 ln .. + 16 of the chunk; threads 0 .. 127 take dword tid & 3 of
  // the 16 scale bytes of slot tid >> 2
  const int xb = 16 * ln, xslot = 2 * w + hi;
  const int eslot = tid >> 2, eb = 4 * (tid & 3);

  for (int t0 = 0; t0 < M; t0 += NT) {
    const int live = min(NT, M - t0);  // token slots of this tile that exist
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (xslot + 8 * i >= live) {
        *reinterpret_cast<u32x4*>(xs + (xslot + 8 * i) * XP + xb) = u32x4{};
        *reinterpret_cast<u32x4*>(xs + (NT + xslot + 8 * i) * XP + xb) = u32x4{};
      }
    }
    if (w < 2 && eslot >= live) {
      *reinterpret_cast<unsigned int*>(xs + eslot * XP + KC + eb) = 0x7f7f7f7fu;
      *reinterpret_cast<unsigned int*>(xs + (NT + eslot) * XP + KC + eb) = 0x7f7f7f7fu;
    }
    const unsigned char* xrow = xq + (long long)t0 * K;
    const unsigned char* erow = xe + (long long)t0 * nb;
    const unsigned int xoff = (unsigned int)xslot * K + xb, eoff = (unsigned int)eslot * nb + eb;
    // The activation loads carry no branch either: a lane whose slot is dead,
    // whose bytes lie past K (the last chunk of a K that is no multiple of KC)
    // or whose chunk lies past the split re-reads the tile's first bytes. A
    // dead slot is never stored; what a live slot stores past K is never read,
    // because the MFMAs at that k are skipped.
    auto load_x = [&](int c, u32x4(&xr)[4], unsigned int& er) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool in = c < c1 && xslot + 8 * i < live && c * KC + xb < K;
        xr[i] = *reinterpret_cast<const u32x4*>(
            xrow + (in ? (unsigned int)(8 * i * K + c * KC) + xoff : 0u));
      }
      const bool in = c < c1 && w < 2 && eslot < live && c * (KC / 32) + eb < nb;
      er = *reinterpret_cast<const unsigned int*>(
          erow + (in ? (unsigned int)(c * (KC / 32)) + eoff : 0u));
    };
    auto store_x = [&](int buf, const u32x4(&xr)[4], unsigned int er) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (xslot + 8 * i < live)
          *reinterpret_cast<u32x4*>(xs + (buf * NT + xslot + 8 * i) * XP + xb) = xr[i];
      if (w < 2 && eslot < live)
        *reinterpret_cast<unsigned int*>(xs + (buf * NT + eslot) * XP + KC + eb) = er;
    };
    // this wave's 256 k of chunk c, without a branch (see the header)
    auto load_w = [&](int c, u32x4(&wr)[4], unsigned int(&sr)[2]) {
      const int k = c * KC + kw * KW;
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const bool in = c < c1 && k + 128 * g < K;  // wave-uniform
        const long long oc = in ? (long long)c * (KC / 2) + kw * (KW / 2) + 64 * g : 0;
        const long long os = in ? (long long)c * (KC / 32) + kw * (KW / 32) + 4 * g : 0;
        wr[2 * g] = *reinterpret_cast<const u32x4*>(ap + oc + aoff);
        wr[2 * g + 1] = *reinterpret_cast<const u32x4*>(ap + (oc + 32) + aoff);
        sr[g] = *reinterpret_cast<const unsigned int*>(sp + os + soff);
      }
    };

    f32x16 acc = {};
    // set s holds chunk c0 + s, c0 + s + NS, ...: the loop below is unrolled
    // over the sets, so every index is a constant and nothing is ever copied
    u32x4 wr[NS][4] = {};
    unsigned int sr[NS][2] = {};
    u32x4 xr[4];
    unsigned int er;
    load_x(c0, xr, er);
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) load_w(c0 + d, wr[d], sr[d]);
    store_x(0, xr, er);
    __syncthreads();
    for (int cb = c0; cb < c1; cb += NS) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int c = cb + s;
        if (c < c1) {  // uniform over the workgroup
          const int buf = (c - c0) & 1;
          const bool more = c + 1 < c1;
          load_x(c + 1, xr, er);
          load_w(c + DEPTH, wr[(s + DEPTH) % NS], sr[(s + DEPTH) % NS]);
          if (mine) {
            const int k = c * KC + kw * KW;
            const unsigned char* trow = xs + (buf * NT + ln) * XP;
            const unsigned char* bp = trow + kw * KW + 16 * hi;
            // the token's 8 scale bytes of this wave's k; byte 2 j + hi is wanted
            const u32x2 sb = *reinterpret_cast<const u32x2*>(trow + KC + kw * (KW / 32));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              if (k + 64 * j < K) {
                const u32x4 b0 = *reinterpret_cast<const u32x4*>(bp + 64 * j);
                const u32x4 b1 = *reinterpret_cast<const u32x4*>(bp + 64 * j + 32);
                const i32x8 b = {(int)b0[0], (int)b0[1], (int)b0[2], (int)b0[3],
                                 (int)b1[0], (int)b1[1], (int)b1[2], (int)b1[3]};
                const unsigned int wa = sr[s][j >> 1] >> (8 * hi), wb = sb[j >> 1] >> (8 * hi);
                acc = (j & 1) ? mfma_e2m1_e4m3<2>(wr[s][j], b, acc, wa, wb)
                              : mfma_e2m1_e4m3<0>(wr[s][j], b, acc, wa, wb);
              }
            }
          }
          if (more) store_x(buf ^ 1, xr, er);
          __syncthreads();
        }
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

// Split k over workgroups until the grid gives about two workgroups per CU,
// while the fp32 partials (written and read once) stay under a quarter of
// the weight bytes N K / 2: 16 S M / K <= 1/4. A function of the shapes only.
// Split z takes cps chunks; returns the number of splits.
int split_rule(long long M, long long N, long long K, int* cps) {
  const int nc = (int)((K + KC - 1) / KC);
  const long long wgs = (N + 63) / 64;
  long long want = std::min<long long>((512 + wgs - 1) / wgs, K / (64 * M));
  want = std::max<long long>(1, std::min<long long>(want, nc));
  *cps = (int)((nc + want - 1) / want);
  return (nc + *cps - 1) / *cps;
}

void launch_reduce(const torch::Tensor& part, torch::Tensor& out, hipStream_t stream) {
  const long long S = part.size(0), M = part.size(1), N = part.size(2);
  const long long n_vec = M * (N / 8);
  hipLaunchKernelGGL(linear_mxfp4w_reduce_kernel, dim3((unsigned)((n_vec + 255) / 256)),
                     dim3(256), 0, stream, part.data_ptr<float>(), (short*)out.data_ptr(), n_vec,
                     (int)N, (int)S, M * N);
}

void check_weights(const char* op, const torch::Tensor& codes, const torch::Tensor& scales,
                   long long M, long long K) {
  TORCH_CHECK(codes.is_cuda() && codes.dim() == 2 && codes.dtype() == torch::kUInt8 &&
                  codes.is_contiguous() && codes.size(1) * 2 == K,
              op, ": codes must be contiguous uint8 [N, K / 2] on the GPU");
  const long long N = codes.size(0);
  TORCH_CHECK(scales.is_cuda() && scales.dim() == 2 && scales.dtype() == torch::kUInt8 &&
                  scales.is_contiguous() && scales.size(0) == N && scales.size(1) * 32 == K,
              op, ": scales must be contiguous uint8 [N, K / 32] on the GPU");
  TORCH_CHECK(K >= 128 && K % 128 == 0 && N >= 32 && N % 32 == 0 && K < (1 << 24) &&
                  N < (1 << 24) && M < (1 << 24),
              op, ": K must be a multiple of 128 and N a multiple of 32");
  // K % 128 == 0 makes every row of codes a multiple of 64 bytes and every row
  // of scales a multiple of 4, so aligned bases keep all loads aligned
  TORCH_CHECK(reinterpret_cast<uintptr_t>(codes.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(scales.data_ptr()) % 4 == 0,
              op, ": operands must be 16-byte aligned (scales 4-byte)");
}

void launch_quantize_mxfp8(const torch::Tensor& x, torch::Tensor& q, torch::Tensor& e,
                           hipStream_t stream) {
  const long long n_vec = x.numel() / 8;
  if (n_vec == 0) return;
  hipLaunchKernelGGL(quantize_mxfp8_kernel, dim3((unsigned)((n_vec + 255) / 256)), dim3(256), 0,
                     stream, (const short*)x.data_ptr(), (unsigned char*)q.data_ptr(),
                     (unsigned char*)e.data_ptr(), n_vec);
}

template <int DEPTH>
void launch_a8(const torch::Tensor& q, const torch::Tensor& e, const torch::Tensor& codes,
               const torch::Tensor& scales, torch::Tensor& out, hipStream_t stream) {
  const long long M = q.size(0), K = q.size(1), N = codes.size(0);
  int cps;
  const int S = split_rule(M, N, K, &cps);
  const unsigned wgs = (unsigned)((N + 63) / 64);
  const unsigned char* qp = (const unsigned char*)q.data_ptr();
  const unsigned char* ep = (const unsigned char*)e.data_ptr();
  const unsigned char* cp = (const unsigned char*)codes.data_ptr();
  const unsigned char* sp = (const unsigned char*)scales.data_ptr();
  if (S == 1) {
    hipLaunchKernelGGL((linear_mxfp4w_a8_kernel<false, DEPTH>), dim3(wgs, 1), dim3(256), 0,
                       stream, qp, ep, cp, sp, out.data_ptr(), (int)M, (int)N, (int)K, cps);
    return;
  }
  auto part = torch::empty({(long long)S, M, N}, out.options().dtype(torch::kFloat32));
  hipLaunchKernelGGL((linear_mxfp4w_a8_kernel<true, DEPTH>), dim3(wgs, (unsigned)S), dim3(256),
                     0, stream, qp, ep, cp, sp, part.data_ptr(), (int)M, (int)N, (int)K, cps);
  launch_reduce(part, out, stream);
}

}  // namespace

// x bf16 [..., K] contiguous, K % 32 == 0 -> (codes e4m3 [..., K], scales uint8 [..., K / 32])
std::tuple<torch::Tensor, torch::Tensor> quantize_mxfp8(torch::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.dim() >= 1 && x.dtype() == torch::kBFloat16 &&
                  x.is_contiguous() && x.size(-1) % 32 == 0 &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "quantize_mxfp8: x must be contiguous, 16-byte aligned bf16 [..., K] on the GPU "
              "with K % 32 == 0");
  auto q = torch::empty(x.sizes(), x.options().dtype(torch::kFloat8_e4m3fn));
  auto esz = x.sizes().vec();
  esz.back() /= 32;
  auto e = torch::empty(esz, x.options().dtype(torch::kUInt8));
  launch_quantize_mxfp8(x, q, e, hypha_stream());
  return {q, e};
}

// linear_mxfp4w on x quantised to MXFP8 first: quantise, GEMM, reduce if split.
// depth: chunks of weights in flight per wave, 0 = the default (for measuring)
torch::Tensor linear_mxfp4w_a8(torch::Tensor x, torch::Tensor codes, torch::Tensor scales,
                               long depth) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.dtype() == torch::kBFloat16 &&
                  x.is_contiguous() && reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "linear_mxfp4w_a8: x must be contiguous, 16-byte aligned bf16 [M, K] on the GPU");
  const long long M = x.size(0), K = x.size(1);
  check_weights("linear_mxfp4w_a8", codes, scales, M, K);
  TORCH_CHECK(depth >= 0 && depth <= 2, "linear_mxfp4w_a8: depth must be 0, 1 or 2");
  auto out = torch::empty({M, codes.size(0)}, x.options());
  if (M == 0) return out;
  hipStream_t stream = hypha_stream();
  auto q = torch::empty({M, K}, x.options().dtype(torch::kUInt8));
  auto e = torch::empty({M, K / 32}, x.options().dtype(torch::kUInt8));
  launch_quantize_mxfp8(x, q, e, stream);
  if (depth == 0) depth = HYPHA_MXFP4W_A8_DEPTH;
  if (depth == 1)
    launch_a8<1>(q, e, codes, scales, out, stream);
  else
    launch_a8<2>(q, e, codes, scales, out, stream);
  return out;
}

// x bf16 [M, K], codes uint8 [N, K / 2], scales uint8 [N, K / 32] -> out bf16 [M, N]
torch::Tensor linear_mxfp4w(torch::Tensor x, torch::Tensor codes, torch::Tensor scales) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.dtype() == torch::kBFloat16 &&
                  x.is_contiguous() && reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "linear_mxfp4w: x must be contiguous, 16-byte aligned bf16 [M, K] on the GPU");
  const long long M = x.size(0), K = x.size(1);
  check_weights("linear_mxfp4w", codes, scales, M, K);
  const long long N = codes.size(0);
  auto out = torch::empty({M, N}, x.options());
  if (M == 0) return out;

  int cps;
  const int S = split_rule(M, N, K, &cps);
  const long long wgs = (N + 63) / 64;
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
  launch_reduce(part, out, stream);
  return out;
}
