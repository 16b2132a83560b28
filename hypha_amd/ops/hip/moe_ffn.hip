// Fused top-k MoE expert FFN for inference (Mixtral-style SwiGLU experts):
//
//   out[t] = sum_k w[t,k] * W_down[e] (silu(W_gate[e] x[t]) * (W_up[e] x[t])),
//   e = topi[t,k], w = renormalised fp32 softmax top-k of the router logits.
//
// Routing, grouping, both GEMM stages and the combine run on the device; the
// host never learns who chose what, so every grid depends on the shapes alone
// and a captured graph replays correctly under any routing. Five launches:
//
//   moe_route_kernel    one wave per token, one lane per expert (E <= 64):
//                       softmax by wave reductions, top_k rounds of (value,
//                       lowest index) arg-max on the logits, fp32 renormalise.
//   moe_group_kernel    stable counting sort of the pair ids p = t*K + k by
//                       expert, one workgroup: a wave owns an expert and walks
//                       the pairs in order with ballots, so counts and
//                       positions are fixed-order (no atomics at all).
//   moe_expert_kernel<false>  gate/up: grid (f/32, E). hbuf[p, f] = bf16(
//                       silu(g) * u) from fp32 accumulators.
//   moe_expert_kernel<true>   down: grid (h/64, E, splits). ybuf[s, p, h] =
//                       fp32 partial * w[p].
//   moe_combine_kernel  out[t] = bf16(sum_k sum_s ybuf[s, t*K+k]) in a fixed
//                       order. No float atomics anywhere: same bits every run.
//
// moe_expert_kernel is a weight-streaming kernel, not a throughput GEMM. A
// workgroup whose expert received no pair returns before its first weight
// load and its first barrier, so at T = 1 only top_k of the E experts are
// read. A live workgroup owns two 32-row weight tiles (gate and up rows of
// one f tile; or two adjacent h tiles of W_down) and streams them from global
// memory once, straight into registers as the A operand of
// v_mfma_f32_32x32x16_bf16 (weight rows on M). The expert's gathered
// activation rows are the B operand (tokens on N, 32 at a time), staged
// through LDS in chunks of 256 k, double buffered, one barrier per chunk.
// The four waves split every chunk by k: wave w takes k in [64 w, 64 w + 64),
// i.e. one whole 128-byte line of each of its 64 weight rows, fetched by four
// 16-byte loads per lane per tile (lane (m, hi) of MFMA step j reads k =
// 16 j + 8 hi .. + 8: the natural order, which A and B share). The next
// chunk's 8 weight loads and 4 activation loads per lane are issued before the
// current chunk's MFMAs, so a wave keeps 12 KiB in flight. The waves' partial
// accumulators meet in LDS (aliasing the staging buffers) in wave order.
// An expert with more than 32 pairs loops over token tiles and re-reads its
// weight tile from L2; columns past the count are zero in LDS and never
// stored.
//
// Weight-only fp8 experts (moe_ffn_fp8w): the same five launches with
// moe_expert_fp8w_kernel<DOWN> in place of moe_expert_kernel. The weights are
// e4m3 codes, one byte each, with one fp32 scale per expert and row. Every
// finite e4m3 value is a bf16 value, so a code becomes its bf16 in registers
// (v_cvt_pk_f32_fp8 gives two exact fp32, one v_perm_b32 keeps their high
// halves) and the GEMMs are the same bf16 MFMAs on exact operands; no
// dequantised copy exists in global memory or LDS. The scale is applied once
// per output element, in fp32, in the epilogue: g = acc_g * s_gate[e, row],
// u = acc_u * s_up[e, row], v = silu(g) * u; ybuf = acc * s_down[e, row] *
// w[pair], which is linear in acc, so split-K stays valid.
// hbuf [P, 2, f] holds v as two bf16 rows, hi = bf16(v) and lo = bf16(v - hi)
// (v - hi is exact in fp32). One bf16 rounding of v, 2^-9 relative, is an
// absolute error of the output that grows with the norm of the W_down row:
// with row scales 16x apart it passes 3e-2 on outputs near 0 at Mixtral's
// f. The down stage therefore takes a pair's hi and lo rows as two neighbouring
// N columns (16 pairs per 32-column tile), runs the same MFMAs per tile and
// adds the two accumulators in the epilogue by one lane swap: the
// intermediate has 16 bits of significand, LDS and registers are unchanged,
// and only an expert with more than 16 pairs pays, by a second pass over its
// weight tile (T = 64 and up, profiles/moe_ffn_fp8w.md).
// The kernel keeps its parent's structure (early exit, two 32-row tiles per
// workgroup, tokens on N, waves split by k, partials met in LDS in wave
// order) with the k geometry of 1-byte weights, which is linear_fp8w.hip's:
//   chunk   512 k, so that each of the four waves still owns one whole
//           128-byte line of each of its 64 code rows: wave w takes k in
//           [128 w, 128 w + 128), four 16-byte loads per lane per tile; lane
//           (m, hi) of load j holds k = 32 j + 16 hi .. + 16, bytes 0-7 the A
//           operand of MFMA step 2 j, bytes 8-15 that of step 2 j + 1, and B
//           is read from LDS at the same k. 8 KiB of codes in flight per wave.
//   gather  a wave stages whole rows: lane l holds k = 8 l .. + 8 of slots
//           w + 4 i, i < 8, so the slot's source row (pairs[off + s] / top_k
//           for gate/up; row 2 pairs[off + s / 2] + s % 2 of hbuf for down)
//           is wave-uniform. A slot
//           past the count is zeroed in both buffers once per token tile and
//           neither loaded nor stored afterwards.
//   tail    h and f are multiples of 128, not of 512: in the last chunk the
//           lanes whose k lies past the end stage zeros, and the waves whose
//           line starts past the end load no codes and issue no MFMA.
//   LDS     pitch 520 shorts (1040 B = 65 x 16 B: conflict-free b128 reads),
//           2 x 32 x 520 x 2 B = 66560 B a workgroup. Two workgroups fit the
//           CU's 160 KiB, three do not, so the target is 2 waves/SIMD
//           (__launch_bounds__(256, 2)): 206 / 204 VGPR (gate/up / down), 0
//           AGPR, 0 scratch. The parent's third wave would need chunks of 384
//           k at most, which four whole-line waves cannot make; the measured
//           rates (profiles/moe_ffn_fp8w.md: 3.9 and 4.5 TB/s of codes at
//           T = 1) are those of the bf16 kernel at 3 waves/SIMD.
// The down projection's split is the same rule on chunks of 512: at Mixtral
// widths and T = 1 (h 4096, f 14336, top-2) f has 28 chunks, the 2 x 64 live
// row tiles ask for 4 splits of 7 chunks, so 512 workgroups are live in the
// down stage (one full residency of 256 CUs x 2) and 2 x 448 = 896 in
// gate/up, out of 2048 and 3584 launched.
//
// Weight-only MXFP4 experts (moe_ffn_mxfp4w): the same five launches with
// moe_expert_mxfp4w_kernel<DOWN, DEPTH>. The weights are e2m1 codes, two per
// byte, with one E8M0 scale byte per 32 k of a row (ops.quantize_mxfp4 of the
// 3-D weight). Every e2m1 value times a power of two is a bf16 value, so the
// GEMMs are again bf16 MFMAs on exact operands. The scale belongs to a k block:
// it enters at the conversion (v_cvt_scalef32_pk_bf16_fp4, e2m1x8_to_bf16x8 in
// hip_common.h) inside the k loop, and the epilogues do no scaling. The
// intermediate is one bf16 row per pair, hbuf [P, f] = bf16(silu(g) * u),
// rounded once from fp32, 32 pairs on N in down, as in moe_expert_kernel: at
// 4-bit weights that rounding is not what limits accuracy, and fp8w's hi/lo
// pair of rows would halve the pairs per down tile.
// The kernel keeps moe_expert_kernel's structure with linear_mxfp4w.hip's k
// geometry:
//   chunk   512 k (pitch 520, double-buffered activation stage, one barrier
//           per chunk). The four waves split a chunk 2 by k x 2 by row tile:
//           wave w takes k in [256 (w & 1), + 256) of tile w >> 1 (gate/up:
//           tile 0 the gate rows and tile 1 the up rows of one f tile; down:
//           two 32-row h tiles), one whole 128-byte line of each of its 32 rows
//           and one accumulator. Lane (m, hi) of load j holds the 32 codes
//           k = 64 j + 32 hi .. + 32: one MX block, one scale byte, four MFMA
//           steps (dword d is k + 8 d .. + 8, B read from LDS at the same k).
//           The two k-waves of a tile meet in LDS in wave order.
//   depth   codes and scale dwords are loaded DEPTH chunks ahead into DEPTH + 1
//           register sets; the chunk loop is unrolled over the sets, so a set
//           is addressed by constants and never copied. Activations stay one
//           chunk ahead (they go through LDS). DEPTH = 2 is 8 KiB of codes in
//           flight per wave, 64 KiB per CU at two workgroups. It only holds if
//           the weight loads carry no branch: with `if (k < Kd) load` the
//           compiler cannot count the loads behind the one it needs and waits
//           for vmcnt(0) before the MFMAs, so one chunk is in flight whatever
//           DEPTH is (measured: DEPTH 2 was then 1 - 5 % slower than DEPTH 1).
//           The loads are therefore unconditional and a half line past the row
//           (K % 256 == 128) or a chunk past the split re-reads the row's
//           first, cached 64 bytes; its MFMA steps are skipped load-uniformly.
//           That version is 4 - 15 % faster than DEPTH 1
//           (profiles/moe_ffn_mxfp4w.md, section 3).
//   gather  as in the fp8w kernel: whole rows per wave, wave-uniform source
//           row, slots past the count zeroed once per token tile and neither
//           loaded nor stored afterwards.
//   LDS     66560 B, 2 waves/SIMD (__launch_bounds__(256, 2)); 218 / 216 VGPR
//           (gate/up / down), 0 AGPR, 0 scratch.
//
// MXFP8 activations on those experts (moe_ffn_mxfp4w_a8): another numerical
// mode. x and v = silu(g) * u are rounded to OCP MXFP8 (e4m3 codes, one E8M0
// byte per 32 k of a row) and both GEMMs are v_mfma_scale_f32_32x32x64_f8f6f4
// on the e2m1 and e4m3 codes and their scale bytes as loaded. Six launches:
// route, group, quantize_mxfp8_kernel on x (once, for gate and up),
// moe_expert_mxfp4w_a8_kernel<DOWN, DEPTH> twice, combine.
// The kernel keeps moe_expert_mxfp4w_kernel's structure (early exit, weight
// rows on M, 32 slots on N, 512-k chunks, waves 2 by k x 2 by row tile, one
// code line per row, wave and chunk, branch-free loads DEPTH ahead, k-waves
// met in LDS in wave order, the same split-K) with linear_mxfp4w_a8_kernel's
// inner loop: a lane's load j is the A operand of one MFMA (cbsz 4), four
// MFMAs a wave and chunk instead of sixteen and sixteen conversions.
//   stage   a slot's row of a chunk is its 512 code bytes and then the chunk's
//           16 scale bytes, pitch 528 B = 33 x 16 B: the sixteen lanes a
//           128-bit LDS read serves together fall in sixteen different 16-byte
//           columns (33 ln = ln mod 16), no conflict. 2 x 32 x 528 = 33792 B.
//           Wave w stages the slots w + 4 i, i < 8: lane l loads bytes
//           8 l .. + 8, so one load instruction is one whole row of one
//           source row (pairs[..] / top_k of xq, pairs[..] of hq), which is
//           wave-uniform and lives in SGPRs; lanes 0 - 31 also take one dword
//           of the 16 scale bytes of slot w + 4 (l >> 2). Double-buffered, one
//           barrier per chunk. A slot past the count holds zero codes under
//           byte 0x7f (2^0), written once per token tile.
//   v       after the meeting a workgroup of gate/up holds v in fp32 for 32 f
//           rows x 32 slots, and rows0 % 32 == 0: one MX block per slot. The
//           eight threads of a slot exchange the integer maximum of their
//           magnitudes through 1 KiB of LDS behind the meeting image (no
//           atomics), form the E8M0 byte from the fp32 exponent field and
//           the codes by v_cvt_pk_fp8_f32 after a clamp to +-448
//           (quantize_mxfp8's rule), and store 4 codes to hq [P, f] and, one
//           thread in eight, the byte to he [P, f / 32]. Nothing is rounded to
//           bf16 and the intermediate costs no launch.
//   regs    DEPTH 2: 179 / 177 VGPR, 2 waves/SIMD; DEPTH 1: 141 / 137, 3
//           waves/SIMD; 0 AGPR, 0 scratch. DEPTH 2 is the default: 7 % ahead
//           at T = 1, 1 % from T = 256 on, 1 - 3 % behind at T = 8 and 64
//           (profiles/moe_ffn_mxfp4w_a8.md, section 4).

#include <torch/extension.h>

#include <algorithm>
#include <cstdint>
#include <tuple>

#include "hip_common.h"

namespace {

constexpr int kMaxExperts = 64;
constexpr int kMaxTopK = 8;
constexpr int NT = 32;          // tokens per MFMA N tile
constexpr int KC = 256;         // k per LDS chunk: 4 waves x 64
constexpr int PITCH = KC + 8;   // LDS row pitch (528 B: conflict-free b128 reads)
constexpr int kGroupThreads = 1024;

// ---- routing ----------------------------------------------------------------

__global__ __launch_bounds__(64) void moe_route_kernel(
    const float* __restrict__ logits, int* __restrict__ topi, float* __restrict__ topw,
    int E, int K) {
  const int t = blockIdx.x, lane = threadIdx.x;
  float l = -INFINITY;
  if (lane < E) {
    l = logits[(long long)t * E + lane];
    if (!(l == l)) l = -INFINITY;  // NaN never wins
  }
  const float mx = wave_reduce_max(l);
  const float p = (lane < E && l > -INFINITY) ? expf(l - mx) : 0.f;
  const float prob = p / wave_reduce_sum(p);

  bool taken = lane >= E;
  int sel[kMaxTopK];
  float val[kMaxTopK];
  float denom = 0.f;
#pragma unroll
  for (int k = 0; k < kMaxTopK; ++k) {  // constant bound: sel/val stay in registers
    if (k >= K) break;
    // arg-max of (logit, lowest index) over the lanes not yet taken; taken
    // lanes rank below every free lane, whatever their value
    float v = taken ? -INFINITY : l;
    int i = taken ? 64 + lane : lane;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float vo = __shfl_xor(v, off, 64);
      const int io = __shfl_xor(i, off, 64);
      if (vo > v || (vo == v && io < i)) {
        v = vo;
        i = io;
      }
    }
    i &= 63;
    if (lane == i) taken = true;
    sel[k] = i;
    val[k] = __shfl(prob, i, 64);
    denom += val[k];
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kMaxTopK; ++k) {
      if (k >= K) break;
      topi[(long long)t * K + k] = sel[k];
      topw[(long long)t * K + k] = val[k] / denom;
    }
  }
}

// Stable counting sort of the pair ids by expert. Wave w owns experts w,
// w + 16, ...; for each it walks all pairs in ascending order, 64 at a time:
// the count is a sum of ballot popcounts and a pair's position is the count
// before it plus the matching lanes below it.
__global__ __launch_bounds__(kGroupThreads) void moe_group_kernel(
    const int* __restrict__ topi, int* __restrict__ offsets, int* __restrict__ pairs,
    int P, int E) {
  __shared__ int s_cnt[kMaxExperts];
  __shared__ int s_off[kMaxExperts + 1];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  constexpr int kWaves = kGroupThreads / 64;
  for (int e = wid; e < E; e += kWaves) {
    int c = 0;
    for (int i = 0; i < P; i += 64) {
      const int idx = i + lane;
      const bool m = idx < P && topi[idx] == e;
      c += __popcll(__ballot(m));
    }
    if (lane == 0) s_cnt[e] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int e = 0; e < E; ++e) {
      s_off[e] = run;
      offsets[e] = run;
      run += s_cnt[e];
    }
    s_off[E] = run;
    offsets[E] = run;
  }
  __syncthreads();
  for (int e = wid; e < E; e += kWaves) {
    int base = s_off[e];
    for (int i = 0; i < P; i += 64) {
      const int idx = i + lane;
      const bool m = idx < P && topi[idx] == e;
      const unsigned long long mask = __ballot(m);
      if (m) pairs[base + __popcll(mask & ((1ull << lane) - 1ull))] = idx;
      base += __popcll(mask);
    }
  }
}

// ---- expert GEMMs -------------------------------------------------------------

// DOWN = false: act = x [T, Kd], wa/wb = W_gate/W_up [E, R, Kd], 32-row tiles,
//               out = hbuf bf16 [P, R].
// DOWN = true : act = hbuf [P, Kd], wa = W_down [E, R, Kd], 64-row tiles,
//               out = ybuf fp32 [gridDim.z, P, R]; split z takes the chunks
//               [z * cps, (z + 1) * cps).
template <bool DOWN>
__global__ __launch_bounds__(256, 3) void moe_expert_kernel(
    const short* __restrict__ act, const short* __restrict__ wa,
    const short* __restrict__ wb, const int* __restrict__ offsets,
    const int* __restrict__ pairs, const float* __restrict__ topw,
    void* __restrict__ outp, int Kd, int R, int top_k, int P, int cps) {
  const int e = blockIdx.y;
  const int off = offsets[e];
  const int cnt = offsets[e + 1] - off;
  if (cnt == 0) return;  // nobody chose this expert: no weight is read

  __shared__ __attribute__((aligned(16))) short xs[2 * NT * PITCH];
  float* red = reinterpret_cast<float*>(xs);  // [4 waves][2 tiles][16][64] after the k loop
  static_assert(4 * 2 * 16 * 64 * sizeof(float) <= sizeof(short) * 2 * NT * PITCH,
                "reduction image must fit the staging buffers");

  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int ln = lane & 31, hi = lane >> 5;
  const int rows0 = blockIdx.x * (DOWN ? 64 : 32);
  const short* a0 = wa + ((long long)e * R + rows0 + ln) * Kd + 8 * hi;
  const short* a1 = DOWN ? a0 + 32ll * Kd
                         : wb + ((long long)e * R + rows0 + ln) * Kd + 8 * hi;
  const int nc = (Kd + KC - 1) / KC;
  const int c0 = blockIdx.z * cps;
  const int c1 = min(nc, c0 + cps);
  const int xslot = tid >> 5;        // staging: slots xslot + 8 i, i < 4
  const int xk = (tid & 31) * 8;     // k inside the chunk

  for (int t0 = 0; t0 < cnt; t0 += NT) {
    int rowi[4];  // activation row of each staged slot, -1 past the count
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int s = t0 + xslot + 8 * i;
      rowi[i] = -1;
      if (s < cnt) rowi[i] = DOWN ? pairs[off + s] : pairs[off + s] / top_k;
    }
    auto load_x = [&](int c, s16x8(&xr)[4]) {
      const int k = c * KC + xk;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        xr[i] = s16x8{};
        if (rowi[i] >= 0 && k < Kd)
          xr[i] = *reinterpret_cast<const s16x8*>(act + (long long)rowi[i] * Kd + k);
      }
    };
    auto store_x = [&](int buf, const s16x8(&xr)[4]) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        *reinterpret_cast<s16x8*>(xs + buf * NT * PITCH + (xslot + 8 * i) * PITCH + xk) =
            xr[i];
    };
    // this wave's 64 k of chunk c: one 128-byte line of each weight row
    auto load_w = [&](int c, s16x8(&wr)[2][4]) {
      const int kb = c * KC + w * 64;
      if (kb < Kd) {  // Kd % 128 == 0, so a started line is whole
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          wr[0][j] = *reinterpret_cast<const s16x8*>(a0 + kb + 16 * j);
          wr[1][j] = *reinterpret_cast<const s16x8*>(a1 + kb + 16 * j);
        }
      }
    };

    f32x16 acc0 = {}, acc1 = {};
    s16x8 wcur[2][4] = {}, wnxt[2][4] = {}, xr[4];
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
      if (c * KC + w * 64 < Kd) {
        const short* bp = xs + buf * NT * PITCH + ln * PITCH + w * 64 + 8 * hi;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const s16x8 b = *reinterpret_cast<const s16x8*>(bp + 16 * j);
          acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wcur[0][j], b, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wcur[1][j], b, acc1, 0, 0, 0);
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
    float s0[4], s1[4];
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
    if (t0 + n < cnt) {
      const int p = pairs[off + t0 + n];
      const int m = 8 * (q >> 1) + 4 * (q & 1);
      if (!DOWN) {
        s16x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          o[i] = f2bf(s0[i] / (1.f + __expf(-s0[i])) * s1[i]);
        *reinterpret_cast<s16x4*>(static_cast<short*>(outp) + (long long)p * R + rows0 + m) = o;
      } else {
        const float wt = topw[p];
        float* y = static_cast<float*>(outp) + ((long long)blockIdx.z * P + p) * R + rows0 + m;
        f32x4 y0, y1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          y0[i] = s0[i] * wt;
          y1[i] = s1[i] * wt;
        }
        *reinterpret_cast<f32x4*>(y) = y0;
        *reinterpret_cast<f32x4*>(y + 32) = y1;
      }
    }
    __syncthreads();  // red aliases the next token tile's staging buffers
  }
}

// ---- expert GEMMs on weight-only fp8 experts -----------------------------------

constexpr int KW8 = 128;         // k per wave per chunk: one 128-byte line of a code row
constexpr int KC8 = 4 * KW8;     // k per LDS chunk
constexpr int PITCH8 = KC8 + 8;  // LDS row pitch (1040 B = 65 x 16 B: conflict-free b128 reads)
constexpr int XL8 = KC8 * NT / (256 * 8);  // 16-byte activation loads per thread per chunk

// moe_expert_kernel on e4m3 codes with one fp32 scale per expert and row.
// DOWN = false: act = x [T, Kd], wa/wb = W8_gate/W8_up [E, R, Kd], sa/sb =
//               s_gate/s_up [E, R], 32-row tiles, out = hbuf bf16 [P, 2, R].
// DOWN = true : act = hbuf [P, 2, Kd], wa = W8_down [E, R, Kd], sa = s_down [E, R],
//               64-row tiles, out = ybuf fp32 [gridDim.z, P, R]; split z takes
//               the chunks [z * cps, (z + 1) * cps).
template <bool DOWN>
__global__ __launch_bounds__(256, 2) void moe_expert_fp8w_kernel(
    const short* __restrict__ act, const unsigned char* __restrict__ wa,
    const unsigned char* __restrict__ wb, const float* __restrict__ sa,
    const float* __restrict__ sb, const int* __restrict__ offsets,
    const int* __restrict__ pairs, const float* __restrict__ topw,
    void* __restrict__ outp, int Kd, int R, int top_k, int P, int cps) {
  const int e = blockIdx.y;
  const int off = offsets[e];
  const int cnt = offsets[e + 1] - off;
  if (cnt == 0) return;  // nobody chose this expert: no weight is read
  // N slots of this expert: a pair in gate/up; in down a pair's hi row of
  // hbuf (slot 2 i) and its lo row (slot 2 i + 1), 16 pairs per token tile
  const int ns = DOWN ? 2 * cnt : cnt;

  __shared__ __attribute__((aligned(16))) short xs[2 * NT * PITCH8];
  float* red = reinterpret_cast<float*>(xs);  // [4 waves][2 tiles][16][64] after the k loop
  static_assert(4 * 2 * 16 * 64 * sizeof(float) <= sizeof(short) * 2 * NT * PITCH8,
                "reduction image must fit the staging buffers");

  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int ln = lane & 31, hi = lane >> 5;
  const int rows0 = blockIdx.x * (DOWN ? 64 : 32);
  const long long row = (long long)e * R + rows0 + ln;
  const unsigned char* a0 = wa + row * Kd + w * KW8 + 16 * hi;
  const unsigned char* a1 = DOWN ? a0 + 32ll * Kd : wb + row * Kd + w * KW8 + 16 * hi;
  const int nc = (Kd + KC8 - 1) / KC8;
  const int c0 = blockIdx.z * cps;
  const int c1 = min(nc, c0 + cps);
  const int xk = lane * 8;  // staging: k inside the chunk; wave w stages slots w + 4 i

  for (int t0 = 0; t0 < ns; t0 += NT) {
    // activation row of each slot this wave stages (wave-uniform); a slot past
    // the count is zeroed in both buffers here and never loaded or stored again
    int rowi[XL8];
#pragma unroll
    for (int i = 0; i < XL8; ++i) {
      const int s = t0 + w + 4 * i;
      rowi[i] = -1;
      if (s < ns) {
        rowi[i] = DOWN ? 2 * pairs[off + (s >> 1)] + (s & 1) : pairs[off + s] / top_k;
      } else {
        *reinterpret_cast<s16x8*>(xs + (w + 4 * i) * PITCH8 + xk) = s16x8{};
        *reinterpret_cast<s16x8*>(xs + (NT + w + 4 * i) * PITCH8 + xk) = s16x8{};
      }
    }
    // a lane whose k lies past Kd (the last chunk of a Kd that is no multiple
    // of KC8) stages zeros; the waves that own that k skip their MFMAs anyway
    auto load_x = [&](int c, s16x8(&xr)[XL8]) {
      const int k = c * KC8 + xk;
#pragma unroll
      for (int i = 0; i < XL8; ++i) {
        xr[i] = s16x8{};
        if (rowi[i] >= 0 && k < Kd)
          xr[i] = *reinterpret_cast<const s16x8*>(act + (long long)rowi[i] * Kd + k);
      }
    };
    auto store_x = [&](int buf, const s16x8(&xr)[XL8]) {
#pragma unroll
      for (int i = 0; i < XL8; ++i)
        if (rowi[i] >= 0)
          *reinterpret_cast<s16x8*>(xs + (buf * NT + w + 4 * i) * PITCH8 + xk) = xr[i];
    };
    // this wave's 128 k of chunk c: one 128-byte line of each code row; lane
    // (m, hi) of load j holds the 16 codes k = 32 j + 16 hi .. + 16
    auto load_w = [&](int c, u32x4(&wr)[2][4]) {
      if (c * KC8 + w * KW8 < Kd) {  // Kd % 128 == 0, so a started line is whole
        const long long kb = (long long)c * KC8;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          wr[0][j] = *reinterpret_cast<const u32x4*>(a0 + kb + 32 * j);
          wr[1][j] = *reinterpret_cast<const u32x4*>(a1 + kb + 32 * j);
        }
      }
    };

    f32x16 acc0 = {}, acc1 = {};
    u32x4 wcur[2][4] = {}, wnxt[2][4] = {};
    s16x8 xr[XL8];
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
      if (c * KC8 + w * KW8 < Kd) {
        // bytes 0-7 of load j are the A operand of MFMA step 2 j, bytes 8-15
        // that of step 2 j + 1; B is read at the same k, so nothing is shuffled
        const short* bp = xs + (buf * NT + ln) * PITCH8 + w * KW8 + 16 * hi;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const s16x8 b0 = *reinterpret_cast<const s16x8*>(bp + 32 * j);
          const s16x8 b1 = *reinterpret_cast<const s16x8*>(bp + 32 * j + 8);
          acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              e4m3x8_to_bf16x8(wcur[0][j][0], wcur[0][j][1]), b0, acc0, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              e4m3x8_to_bf16x8(wcur[0][j][2], wcur[0][j][3]), b1, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              e4m3x8_to_bf16x8(wcur[1][j][0], wcur[1][j][1]), b0, acc1, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              e4m3x8_to_bf16x8(wcur[1][j][2], wcur[1][j][3]), b1, acc1, 0, 0, 0);
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
    if (DOWN) {  // hi + lo: a pair's two columns sit on neighbouring lanes
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s0[i] += __shfl_xor(s0[i], 1, 64);
        s1[i] += __shfl_xor(s1[i], 1, 64);
      }
    }
    if (t0 + n < ns && !(DOWN && (n & 1))) {
      const int p = pairs[off + (DOWN ? (t0 + n) >> 1 : t0 + n)];
      const int m = rows0 + 8 * (q >> 1) + 4 * (q & 1);
      // the only place a scale is used: once per output element, in fp32
      const long long srow = (long long)e * R + m;
      const f32x4 sc0 = *reinterpret_cast<const f32x4*>(sa + srow);
      const f32x4 sc1 = *reinterpret_cast<const f32x4*>(DOWN ? sa + srow + 32 : sb + srow);
      if (!DOWN) {
        s16x4 o, lo;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float g = s0[i] * sc0[i], u = s1[i] * sc1[i];
          const float v = g / (1.f + __expf(-g)) * u;
          o[i] = f2bf(v);
          lo[i] = f2bf(v - bf2f(o[i]));  // what the rounding dropped, exact in fp32
        }
        short* hp = static_cast<short*>(outp) + 2ll * p * R + m;
        *reinterpret_cast<s16x4*>(hp) = o;
        *reinterpret_cast<s16x4*>(hp + R) = lo;
      } else {
        const float wt = topw[p];
        float* y = static_cast<float*>(outp) + ((long long)blockIdx.z * P + p) * R + m;
        f32x4 y0, y1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          y0[i] = s0[i] * sc0[i] * wt;
          y1[i] = s1[i] * sc1[i] * wt;
        }
        *reinterpret_cast<f32x4*>(y) = y0;
        *reinterpret_cast<f32x4*>(y + 32) = y1;
      }
    }
    __syncthreads();  // red aliases the next token tile's staging buffers
  }
}

// ---- expert GEMMs on weight-only MXFP4 experts ---------------------------------

constexpr int KW4 = 256;         // k per wave per chunk: one 128-byte line of a code row
constexpr int KC4 = 2 * KW4;     // k per LDS chunk
constexpr int PITCH4 = KC4 + 8;  // LDS row pitch (1040 B = 65 x 16 B: conflict-free b128 reads)
constexpr int XL4 = KC4 * NT / (256 * 8);  // 16-byte activation loads per thread per chunk
// chunks of codes and scale bytes a wave keeps in flight ahead of its MFMAs
#ifndef HYPHA_MOE_MXFP4_DEPTH
#define HYPHA_MOE_MXFP4_DEPTH 2
#endif

// moe_expert_kernel on MXFP4 codes (two e2m1 per byte) with one E8M0 scale
// byte per 32 k of a row.
// DOWN = false: act = x [T, Kd], wa/wb = codes of W_gate/W_up [E, R, Kd / 2],
//               sa/sb = their scales [E, R, Kd / 32]; the workgroup's two
//               tiles are rows rows0 .. + 32 of gate and of up, out = hbuf
//               bf16 [P, R].
// DOWN = true : act = hbuf [P, Kd], wa/sa = codes/scales of W_down; the tiles
//               are rows rows0 .. + 32 and rows0 + 32 .. + 32, out = ybuf fp32
//               [gridDim.z, P, R]; split z takes the chunks [z * cps,
//               (z + 1) * cps).
template <bool DOWN, int DEPTH>
__global__ __launch_bounds__(256, 2) void moe_expert_mxfp4w_kernel(
    const short* __restrict__ act, const unsigned char* __restrict__ wa,
    const unsigned char* __restrict__ wb, const unsigned char* __restrict__ sa,
    const unsigned char* __restrict__ sb, const int* __restrict__ offsets,
    const int* __restrict__ pairs, const float* __restrict__ topw,
    void* __restrict__ outp, int Kd, int R, int top_k, int P, int cps) {
  static_assert(DEPTH >= 1 && DEPTH <= 3, "prefetch depth");
  constexpr int NS = DEPTH + 1;  // register sets: the chunk in use and DEPTH in flight
  const int e = blockIdx.y;
  const int off = offsets[e];
  const int cnt = offsets[e + 1] - off;
  if (cnt == 0) return;  // nobody chose this expert: no weight is read

  __shared__ __attribute__((aligned(16))) short xs[2 * NT * PITCH4];
  float* red = reinterpret_cast<float*>(xs);  // [4 waves][16][64] after the k loop
  static_assert(4 * 16 * 64 * sizeof(float) <= sizeof(short) * 2 * NT * PITCH4,
                "reduction image must fit the staging buffers");

  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int ln = lane & 31, hi = lane >> 5;
  const int kw = w & 1, rt = w >> 1;  // this wave's k half of a chunk and its row tile
  const int rows0 = blockIdx.x * (DOWN ? 64 : 32);
  // a row is Kd / 2 bytes of codes and Kd / 32 scale bytes
  const long long row = (long long)e * R + rows0 + (DOWN ? 32 * rt : 0) + ln;
  const unsigned char* ap = ((DOWN || rt == 0) ? wa : wb) + row * (Kd / 2) + 16 * hi;
  const unsigned char* sp = ((DOWN || rt == 0) ? sa : sb) + row * (Kd / 32);
  const int nc = (Kd + KC4 - 1) / KC4;
  const int c0 = blockIdx.z * cps;
  const int c1 = min(nc, c0 + cps);
  const int xk = lane * 8;  // staging: k inside the chunk; wave w stages slots w + 4 i

  for (int t0 = 0; t0 < cnt; t0 += NT) {
    // activation row of each slot this wave stages (wave-uniform); a slot past
    // the count is zeroed in both buffers here and never loaded or stored again
    int rowi[XL4];
#pragma unroll
    for (int i = 0; i < XL4; ++i) {
      const int s = t0 + w + 4 * i;
      rowi[i] = -1;
      if (s < cnt) {
        rowi[i] = DOWN ? pairs[off + s] : pairs[off + s] / top_k;
      } else {
        *reinterpret_cast<s16x8*>(xs + (w + 4 * i) * PITCH4 + xk) = s16x8{};
        *reinterpret_cast<s16x8*>(xs + (NT + w + 4 * i) * PITCH4 + xk) = s16x8{};
      }
    }
    // a lane whose k lies past Kd (the last chunk of a Kd that is no multiple
    // of KC4) stages zeros; the MFMA steps at that k are skipped anyway
    auto load_x = [&](int c, s16x8(&xr)[XL4]) {
      const int k = c * KC4 + xk;
#pragma unroll
      for (int i = 0; i < XL4; ++i) {
        xr[i] = s16x8{};
        if (rowi[i] >= 0 && k < Kd)
          xr[i] = *reinterpret_cast<const s16x8*>(act + (long long)rowi[i] * Kd + k);
      }
    };
    auto store_x = [&](int buf, const s16x8(&xr)[XL4]) {
#pragma unroll
      for (int i = 0; i < XL4; ++i)
        if (rowi[i] >= 0)
          *reinterpret_cast<s16x8*>(xs + (buf * NT + w + 4 * i) * PITCH4 + xk) = xr[i];
    };
    // this wave's 256 k of chunk c: one 128-byte line of each code row and its
    // 8 scale bytes; lane (m, hi) of load j holds the 32 codes k = 64 j + 32 hi
    // .. + 32, one MX block. Kd % 128 == 0, so loads 2 j and 2 j + 1 (128 k, 4
    // scale bytes) are both inside the row or both past it. The loads carry no
    // branch: a branch around a load makes the compiler wait for every load in
    // flight (vmcnt(0)) before the MFMAs, which leaves one chunk in flight
    // whatever DEPTH is. A half past the row, or a chunk at or past c1, reads
    // the first 64 bytes of its own row and its first scale dword again (every
    // row has them, they are in cache, and their MFMA steps are skipped): that
    // is one line per row and at most DEPTH + 1 times per workgroup.
    auto load_w = [&](int c, u32x4(&wr)[4], unsigned int(&sr)[2]) {
      const int k = c * KC4 + kw * KW4;
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const bool in = c < c1 && k + 128 * g < Kd;  // wave-uniform
        const long long oc = in ? (long long)c * (KC4 / 2) + kw * (KW4 / 2) + 64 * g : 0;
        const long long os = in ? (long long)c * (KC4 / 32) + kw * (KW4 / 32) + 4 * g : 0;
        wr[2 * g] = *reinterpret_cast<const u32x4*>(ap + oc);
        wr[2 * g + 1] = *reinterpret_cast<const u32x4*>(ap + oc + 32);
        sr[g] = *reinterpret_cast<const unsigned int*>(sp + os);
      }
    };

    f32x16 acc = {};
    // set s holds chunk c0 + s, c0 + s + NS, ...: the loop below is unrolled
    // over the sets, so every index is a constant and nothing is ever copied
    u32x4 wr[NS][4] = {};
    unsigned int sr[NS][2] = {};
    s16x8 xr[XL4];
    load_x(c0, xr);
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) load_w(c0 + d, wr[d], sr[d]);
    store_x(0, xr);
    __syncthreads();
    for (int cb = c0; cb < c1; cb += NS) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int c = cb + s;
        if (c < c1) {  // uniform over the workgroup
          const int buf = (c - c0) & 1;
          const bool more = c + 1 < c1;
          if (more) load_x(c + 1, xr);
          load_w(c + DEPTH, wr[(s + DEPTH) % NS], sr[(s + DEPTH) % NS]);
          const int k = c * KC4 + kw * KW4;
          const short* bp = xs + (buf * NT + ln) * PITCH4 + kw * KW4 + 32 * hi;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (k + 64 * j < Kd) {
              // scale byte 2 j + hi of the wave's 8: 2^(byte - 127) as fp32
              const float sc = __uint_as_float(
                  ((sr[s][j >> 1] >> (16 * (j & 1) + 8 * hi)) & 0xffu) << 23);
              // dword d of the load is k + 8 d .. + 8; B is read at the same k
#pragma unroll
              for (int d = 0; d < 4; ++d) {
                const s16x8 b = *reinterpret_cast<const s16x8*>(bp + 64 * j + 8 * d);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                    e2m1x8_to_bf16x8(wr[s][j][d], sc), b, acc, 0, 0, 0);
              }
            }
          }
          if (more) store_x(buf ^ 1, xr);
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
    if (t0 + n < cnt) {
      const int p = pairs[off + t0 + n];
      const int m = rows0 + 8 * (q >> 1) + 4 * (q & 1);
      if (!DOWN) {  // s0 = gate, s1 = up; rounded to bf16 once
        s16x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = f2bf(s0[i] / (1.f + __expf(-s0[i])) * s1[i]);
        *reinterpret_cast<s16x4*>(static_cast<short*>(outp) + (long long)p * R + m) = o;
      } else {
        const float wt = topw[p];
        float* y = static_cast<float*>(outp) + ((long long)blockIdx.z * P + p) * R + m;
        f32x4 y0, y1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          y0[i] = s0[i] * wt;
          y1[i] = s1[i] * wt;
        }
        *reinterpret_cast<f32x4*>(y) = y0;
        *reinterpret_cast<f32x4*>(y + 32) = y1;
      }
    }
    __syncthreads();  // red aliases the next token tile's staging buffers
  }
}

// ---- the same experts on MXFP8 activations: block-scaled MFMA -------------------

constexpr int XPA = KC4 + 16;  // LDS row of a slot: 512 e4m3 codes, then the chunk's 16 scale bytes
constexpr int XLA = NT / 4;  // slots a wave stages: one 8-byte load per lane is a slot's whole row
static_assert(64 * 8 == KC4, "a wave's 8-byte loads must cover one row of a chunk");
// chunks of codes and scale bytes a wave keeps in flight ahead of its MFMAs
#ifndef HYPHA_MOE_MXFP4_A8_DEPTH
#define HYPHA_MOE_MXFP4_A8_DEPTH 2
#endif

// moe_expert_mxfp4w_kernel on activations in OCP MXFP8 (e4m3 codes, one E8M0
// byte per 32 k of a row); weights as there.
// DOWN = false: actq/acte = codes [T, Kd] and scales [T, Kd / 32] of x, out =
//               hq e4m3 [P, R] and oute = he E8M0 [P, R / 32]: silu(g) * u of
//               the workgroup's 32 f rows, one MX block per slot, quantised
//               from the fp32 accumulators.
// DOWN = true : actq/acte = hq/he, out = ybuf fp32 [gridDim.z, P, R], oute unused.
template <bool DOWN, int DEPTH>
__global__ __launch_bounds__(256, 2) void moe_expert_mxfp4w_a8_kernel(
    const unsigned char* __restrict__ actq, const unsigned char* __restrict__ acte,
    const unsigned char* __restrict__ wa, const unsigned char* __restrict__ wb,
    const unsigned char* __restrict__ sa, const unsigned char* __restrict__ sb,
    const int* __restrict__ offsets, const int* __restrict__ pairs,
    const float* __restrict__ topw, void* __restrict__ outp, unsigned char* __restrict__ oute,
    int Kd, int R, int top_k, int P, int cps) {
  static_assert(DEPTH >= 1 && DEPTH <= 3, "prefetch depth");
  constexpr int NS = DEPTH + 1;  // register sets: the chunk in use and DEPTH in flight
  const int e = blockIdx.y;
  const int off = offsets[e];
  const int cnt = offsets[e + 1] - off;
  if (cnt == 0) return;  // nobody chose this expert: no weight is read

  __shared__ __attribute__((aligned(16))) unsigned char xs[2 * NT * XPA];
  float* red = reinterpret_cast<float*>(xs);  // [4 waves][16][64] after the k loop
  // behind it, the block's amax by thread: [8 row groups][32 slots]
  unsigned int* amx = reinterpret_cast<unsigned int*>(xs) + 4 * 16 * 64;
  static_assert((4 * 16 * 64 + 8 * 32) * sizeof(float) <= 2 * NT * XPA,
                "reduction image must fit the staging buffers");

  const int tid = threadIdx.x;
  // the wave index through readfirstlane: what follows from it (k half, row
  // tile, the staged slots' source rows, the chunk offsets) lives in SGPRs
  const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ln = lane & 31, hi = lane >> 5;
  const int kw = w & 1, rt = w >> 1;  // this wave's k half of a chunk and its row tile
  const int rows0 = blockIdx.x * (DOWN ? 64 : 32);
  const int nb = Kd / 32;  // scale bytes of a row
  // a wave-uniform 64-bit base plus a 32-bit lane offset that never changes
  const long long row0 = (long long)e * R + rows0 + (DOWN ? 32 * rt : 0);
  const unsigned char* ap = ((DOWN || rt == 0) ? wa : wb) + row0 * (Kd / 2);
  const unsigned char* sp = ((DOWN || rt == 0) ? sa : sb) + row0 * nb;
  const unsigned int aoff = (unsigned int)ln * (unsigned int)(Kd / 2) + 16 * hi;
  const unsigned int soff = (unsigned int)ln * nb;
  const int nc = (Kd + KC4 - 1) / KC4;
  const int c0 = blockIdx.z * cps;
  const int c1 = min(nc, c0 + cps);
  // staging: wave w takes the slots w + 4 i, i < 8, lane l the code bytes
  // 8 l .. + 8 of the chunk, so a load is one whole 512-byte row of one source
  // row; the lower half-wave also takes dword ln & 3 of the 16 scale bytes of
  // slot w + 4 (ln >> 2)
  const int xb = 8 * lane;
  const int eslot = w + 4 * (ln >> 2), eb = 4 * (ln & 3);

  for (int t0 = 0; t0 < cnt; t0 += NT) {
    // source row of each slot this wave stages (wave-uniform), -1 past the
    // count: such a slot gets zero codes under the scale 0x7f (2^0) in both
    // buffers here and is neither loaded into nor stored again
    int rowi[XLA];
#pragma unroll
    for (int i = 0; i < XLA; ++i) {
      const int s = t0 + w + 4 * i;
      rowi[i] = -1;
      if (s < cnt) {
        rowi[i] = DOWN ? pairs[off + s] : pairs[off + s] / top_k;
      } else {
        *reinterpret_cast<u32x2*>(xs + (w + 4 * i) * XPA + xb) = u32x2{};
        *reinterpret_cast<u32x2*>(xs + (NT + w + 4 * i) * XPA + xb) = u32x2{};
      }
    }
    int erowi = -1;  // source row of this lane's scale dword
    if (hi == 0) {
      if (t0 + eslot < cnt) {
        erowi = DOWN ? pairs[off + t0 + eslot] : pairs[off + t0 + eslot] / top_k;
      } else {
        *reinterpret_cast<unsigned int*>(xs + eslot * XPA + KC4 + eb) = 0x7f7f7f7fu;
        *reinterpret_cast<unsigned int*>(xs + (NT + eslot) * XPA + KC4 + eb) = 0x7f7f7f7fu;
      }
    }
    // The activation loads carry no branch either. A dead slot or a chunk at
    // or past c1 reads row 0 instead, a lane whose bytes lie past Kd (the last
    // chunk of a Kd that is no multiple of KC4) the first bytes of its chunk:
    // every such address is inside the tensor. A dead slot is never stored;
    // what a live slot stores past Kd is never read, because the MFMAs at that
    // k are skipped.
    auto load_x = [&](int c, u32x2(&xr)[XLA], unsigned int& er) {
      const unsigned int lo = c * KC4 + xb < Kd ? xb : 0;
#pragma unroll
      for (int i = 0; i < XLA; ++i) {
        const long long ro =
            (c < c1 && rowi[i] >= 0) ? (long long)rowi[i] * Kd + c * KC4 : 0;  // wave-uniform
        xr[i] = *reinterpret_cast<const u32x2*>(actq + ro + lo);
      }
      const bool in = c < c1 && erowi >= 0 && c * (KC4 / 32) + eb < nb;
      er = *reinterpret_cast<const unsigned int*>(
          acte + (in ? (long long)erowi * nb + c * (KC4 / 32) + eb : 0));
    };
    auto store_x = [&](int buf, const u32x2(&xr)[XLA], unsigned int er) {
#pragma unroll
      for (int i = 0; i < XLA; ++i)
        if (rowi[i] >= 0)
          *reinterpret_cast<u32x2*>(xs + (buf * NT + w + 4 * i) * XPA + xb) = xr[i];
      if (erowi >= 0)
        *reinterpret_cast<unsigned int*>(xs + (buf * NT + eslot) * XPA + KC4 + eb) = er;
    };
    // this wave's 256 k of chunk c without a branch, as in moe_expert_mxfp4w_kernel
    auto load_w = [&](int c, u32x4(&wr)[4], unsigned int(&sr)[2]) {
      const int k = c * KC4 + kw * KW4;
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const bool in = c < c1 && k + 128 * g < Kd;  // wave-uniform
        const long long oc = in ? (long long)c * (KC4 / 2) + kw * (KW4 / 2) + 64 * g : 0;
        const long long os = in ? (long long)c * (KC4 / 32) + kw * (KW4 / 32) + 4 * g : 0;
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
    u32x2 xr[XLA];
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
          const int k = c * KC4 + kw * KW4;
          // lane (ln, hi) of step j: A is load j as it came (32 e2m1 codes,
          // k = 64 j + 32 hi .. + 32, scale byte 2 j + hi of the wave's 8); B
          // is slot ln's e4m3 bytes at 64 j + 16 hi and 64 j + 32 + 16 hi, its
          // scale byte 2 j + hi of the slot's 8 (linear_mxfp4w_a8_kernel's map)
          const unsigned char* trow = xs + (buf * NT + ln) * XPA;
          const unsigned char* bp = trow + kw * KW4 + 16 * hi;
          const u32x2 sbv = *reinterpret_cast<const u32x2*>(trow + KC4 + kw * (KW4 / 32));
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (k + 64 * j < Kd) {
              const u32x4 b0 = *reinterpret_cast<const u32x4*>(bp + 64 * j);
              const u32x4 b1 = *reinterpret_cast<const u32x4*>(bp + 64 * j + 32);
              const i32x8 b = {(int)b0[0], (int)b0[1], (int)b0[2], (int)b0[3],
                               (int)b1[0], (int)b1[1], (int)b1[2], (int)b1[3]};
              const unsigned int sw = sr[s][j >> 1] >> (8 * hi), sx = sbv[j >> 1] >> (8 * hi);
              acc = (j & 1) ? mfma_e2m1_e4m3<2>(wr[s][j], b, acc, sw, sx)
                            : mfma_e2m1_e4m3<0>(wr[s][j], b, acc, sw, sx);
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
    // thread (n, q): slot n, tile rows 4 q .. + 4, which are registers
    // 4 (q >> 1) .. + 4 of MFMA lane 32 (q & 1) + n
    const int n = tid & 31, q = tid >> 5;
    f32x4 s0, s1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * (q >> 1) + i, src = 32 * (q & 1) + n;
      s0[i] = red[(0 * 16 + r) * 64 + src] + red[(1 * 16 + r) * 64 + src];
      s1[i] = red[(2 * 16 + r) * 64 + src] + red[(3 * 16 + r) * 64 + src];
    }
    const bool live = t0 + n < cnt;
    const int p = live ? pairs[off + t0 + n] : 0;
    if (!DOWN) {
      // s0 = gate, s1 = up. The tile's 32 f rows are one MX block of the down
      // projection's k: quantize_mxfp8's rule on the fp32 values. The eight
      // threads of a slot exchange their largest magnitude (finite fp32
      // magnitudes order as their bits do) through LDS.
      float v[4];
      unsigned int am = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i] = s0[i] / (1.f + __expf(-s0[i])) * s1[i];
        am = max(am, __float_as_uint(v[i]) & 0x7fffffffu);
      }
      amx[q * 32 + n] = am;
      __syncthreads();
#pragma unroll
      for (int qq = 0; qq < 8; ++qq) am = max(am, amx[qq * 32 + n]);
      // e = floor(log2(amax)) - 8 clamped below at -125 (zeros and fp32
      // denormals included); an fp32 exponent cannot reach the upper clamp
      const int byte = max(2, (int)(am >> 23) - 8);
      // 2^(127 - byte): field 254 - byte in [8, 252], a normal fp32
      const float inv = __uint_as_float((unsigned int)(254 - byte) << 23);
      if (live) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = fminf(fmaxf(v[i] * inv, -448.f), 448.f);
        int d = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
        d = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], d, true);
        *reinterpret_cast<int*>(static_cast<unsigned char*>(outp) + (long long)p * R + rows0 +
                                4 * q) = d;
        if (q == 0) oute[(long long)p * (R / 32) + rows0 / 32] = (unsigned char)byte;
      }
    } else if (live) {
      const float wt = topw[p];
      float* y = static_cast<float*>(outp) + ((long long)blockIdx.z * P + p) * R + rows0 + 4 * q;
      f32x4 y0, y1;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        y0[i] = s0[i] * wt;
        y1[i] = s1[i] * wt;
      }
      *reinterpret_cast<f32x4*>(y) = y0;
      *reinterpret_cast<f32x4*>(y + 32) = y1;
    }
    __syncthreads();  // red aliases the next token tile's staging buffers
  }
}

// out[t, c .. c + 8] = bf16(sum_k (sum_s ybuf[s, t K + k, c .. c + 8]))
__global__ __launch_bounds__(256) void moe_combine_kernel(
    const float* __restrict__ ybuf, short* __restrict__ out, long long n_vec, int h,
    int K, int S, long long P) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_vec) return;
  const int hv = h / 8;
  const long long t = idx / hv;
  const int c = (int)(idx % hv) * 8;
  float acc[8] = {};
  for (int k = 0; k < K; ++k) {
    float part[8] = {};
    for (int s = 0; s < S; ++s) {
      const float* y = ybuf + ((long long)s * P + t * K + k) * h + c;
      const f32x4 lo = *reinterpret_cast<const f32x4*>(y);
      const f32x4 hi = *reinterpret_cast<const f32x4*>(y + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        part[j] += lo[j];
        part[4 + j] += hi[j];
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += part[j];
  }
  s16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = f2bf(acc[j]);
  *reinterpret_cast<s16x8*>(out + t * h + c) = o;
}

// ---- host ---------------------------------------------------------------------

struct Routing {
  torch::Tensor topi, topw, offsets, pairs;
};

void check_router(const torch::Tensor& logits, long top_k) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.dtype() == torch::kFloat32 &&
                  logits.is_contiguous(),
              "moe: router_logits must be contiguous fp32 [T, E] on the GPU");
  const long long E = logits.size(1);
  TORCH_CHECK(E >= 1 && E <= kMaxExperts, "moe: E must lie in [1, 64]");
  TORCH_CHECK(top_k >= 1 && top_k <= E && top_k <= kMaxTopK,
              "moe: top_k must lie in [1, min(E, 8)]");
  TORCH_CHECK(logits.size(0) * top_k < (1ll << 30), "moe: T * top_k out of range");
}

// T > 0. Routing buffers come from the caching allocator on the current
// stream (graph-safe); the grids depend on (T, E, K) alone.
Routing route(const torch::Tensor& logits, int K, hipStream_t stream) {
  const int T = (int)logits.size(0), E = (int)logits.size(1);
  const auto i32 = logits.options().dtype(torch::kInt32);
  Routing r;
  r.topi = torch::empty({T, K}, i32);
  r.topw = torch::empty({T, K}, logits.options());
  r.offsets = torch::empty({E + 1}, i32);
  r.pairs = torch::empty({(long long)T * K}, i32);
  hipLaunchKernelGGL(moe_route_kernel, dim3((unsigned)T), dim3(64), 0, stream,
                     logits.data_ptr<float>(), r.topi.data_ptr<int>(),
                     r.topw.data_ptr<float>(), E, K);
  hipLaunchKernelGGL(moe_group_kernel, dim3(1), dim3(kGroupThreads), 0, stream,
                     r.topi.data_ptr<int>(), r.offsets.data_ptr<int>(),
                     r.pairs.data_ptr<int>(), T * K, E);
  return r;
}

// Chunks per split of the down projection: k is split over workgroups until
// top_k live experts alone give about two workgroups per CU (512 on 256 CUs),
// at most 8 ways; a function of the shapes only. nc = number of k chunks.
int down_chunks_per_split(int nc, long long h, int K, long long P) {
  if (P > 256) return nc;
  const long long live = (h / 64) * K;
  int want = (int)std::min<long long>((512 + live - 1) / live, 8);
  want = std::max(1, std::min(want, nc));
  return (nc + want - 1) / want;
}

// The operand checks of moe_ffn_mxfp4w and moe_ffn_mxfp4w_a8. -> f
long long check_mxfp4_experts(const char* op, const torch::Tensor& x,
                              const torch::Tensor& router_logits, const torch::Tensor& c_gate,
                              const torch::Tensor& e_gate, const torch::Tensor& c_up,
                              const torch::Tensor& e_up, const torch::Tensor& c_down,
                              const torch::Tensor& e_down, long top_k) {
  check_router(router_logits, top_k);
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.dtype() == torch::kBFloat16 &&
                  x.is_contiguous(),
              op, ": x must be contiguous bf16 [T, h] on the GPU");
  const long long T = x.size(0), h = x.size(1), E = router_logits.size(1);
  TORCH_CHECK(router_logits.size(0) == T, op, ": router_logits must be [T, E]");
  // codes [E, rows, cols / 2] or scales [E, rows, cols / 32]
  auto bytes = [&](const torch::Tensor& w, long long rows, long long cols, int per) {
    return w.is_cuda() && w.dim() == 3 && w.dtype() == torch::kUInt8 && w.is_contiguous() &&
           w.size(0) == E && w.size(1) == rows && w.size(2) * per == cols;
  };
  TORCH_CHECK(c_gate.dim() == 3, op, ": c_gate must be [E, f, h / 2]");
  const long long f = c_gate.size(1);
  TORCH_CHECK(bytes(c_gate, f, h, 2) && bytes(c_up, f, h, 2) && bytes(c_down, h, f, 2), op,
              ": the codes must be contiguous uint8 [E, f, h / 2], [E, f, h / 2] and "
              "[E, h, f / 2] on the GPU");
  TORCH_CHECK(bytes(e_gate, f, h, 32) && bytes(e_up, f, h, 32) && bytes(e_down, h, f, 32), op,
              ": the scales must be contiguous uint8 [E, f, h / 32], [E, f, h / 32] and "
              "[E, h, f / 32] on the GPU");
  TORCH_CHECK(h >= 128 && h % 128 == 0 && f >= 128 && f % 128 == 0 && h < (1 << 24) &&
                  f < (1 << 24),
              op, ": h and f must be multiples of 128");
  // h, f % 128 == 0 make every row of codes a multiple of 64 bytes and every
  // row of scales a multiple of 4, so aligned bases keep all loads aligned
  for (const torch::Tensor* t : {&x, &c_gate, &c_up, &c_down, &e_gate, &e_up, &e_down})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, op,
                ": operands must be 16-byte aligned");
  return f;
}

// gate/up, down and combine of moe_ffn_mxfp4w_a8 at one prefetch depth
template <int D>
void launch_experts_a8(const torch::Tensor& xq, const torch::Tensor& xe, const Routing& r,
                       const torch::Tensor& c_gate, const torch::Tensor& e_gate,
                       const torch::Tensor& c_up, const torch::Tensor& e_up,
                       const torch::Tensor& c_down, const torch::Tensor& e_down,
                       torch::Tensor& out, int K, hipStream_t stream) {
  const long long T = out.size(0), h = out.size(1), E = c_gate.size(0), f = c_gate.size(1);
  const long long P = T * K;
  const int nc_down = (int)((f + KC4 - 1) / KC4);
  const int cps = down_chunks_per_split(nc_down, h, K, P);
  const int S = (nc_down + cps - 1) / cps;

  const auto u8opt = out.options().dtype(torch::kUInt8);
  auto hq = torch::empty({P, f}, u8opt);       // e4m3 codes of silu(g) * u
  auto he = torch::empty({P, f / 32}, u8opt);  // their E8M0 scales
  auto ybuf = torch::empty({(long long)S, P, h}, out.options().dtype(torch::kFloat32));
  const int* offs = r.offsets.data_ptr<int>();
  const int* pairs = r.pairs.data_ptr<int>();
  const float* topw = r.topw.data_ptr<float>();
  using u8 = unsigned char;
  hipLaunchKernelGGL((moe_expert_mxfp4w_a8_kernel<false, D>),
                     dim3((unsigned)(f / 32), (unsigned)E, 1), dim3(256), 0, stream,
                     (const u8*)xq.data_ptr(), (const u8*)xe.data_ptr(),
                     (const u8*)c_gate.data_ptr(), (const u8*)c_up.data_ptr(),
                     (const u8*)e_gate.data_ptr(), (const u8*)e_up.data_ptr(), offs, pairs, topw,
                     hq.data_ptr(), (u8*)he.data_ptr(), (int)h, (int)f, K, (int)P,
                     (int)((h + KC4 - 1) / KC4));
  hipLaunchKernelGGL((moe_expert_mxfp4w_a8_kernel<true, D>),
                     dim3((unsigned)(h / 64), (unsigned)E, (unsigned)S), dim3(256), 0, stream,
                     (const u8*)hq.data_ptr(), (const u8*)he.data_ptr(),
                     (const u8*)c_down.data_ptr(), (const u8*)nullptr,
                     (const u8*)e_down.data_ptr(), (const u8*)nullptr, offs, pairs, topw,
                     ybuf.data_ptr(), (u8*)nullptr, (int)f, (int)h, K, (int)P, cps);
  const long long n_vec = T * (h / 8);
  hipLaunchKernelGGL(moe_combine_kernel, dim3((unsigned)((n_vec + 255) / 256)), dim3(256), 0,
                     stream, ybuf.data_ptr<float>(), (short*)out.data_ptr(), n_vec, (int)h, K,
                     S, P);
}

}  // namespace

// linear_mxfp4w.hip: bf16 [..., K] -> (e4m3 codes [..., K], E8M0 scales [..., K / 32])
std::tuple<torch::Tensor, torch::Tensor> quantize_mxfp8(torch::Tensor x);

// router_logits fp32 [T, E] -> (topi int32 [T, K], topw fp32 [T, K],
// offsets int32 [E + 1], pairs int32 [T * K])
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor> moe_route(
    torch::Tensor router_logits, long top_k) {
  check_router(router_logits, top_k);
  const long long T = router_logits.size(0), E = router_logits.size(1);
  if (T == 0) {
    const auto i32 = router_logits.options().dtype(torch::kInt32);
    return {torch::empty({0, top_k}, i32), torch::empty({0, top_k}, router_logits.options()),
            torch::zeros({E + 1}, i32), torch::empty({0}, i32)};
  }
  Routing r = route(router_logits, (int)top_k, hypha_stream());
  return {r.topi, r.topw, r.offsets, r.pairs};
}

// x bf16 [T, h], router_logits fp32 [T, E], w_gate/w_up bf16 [E, f, h],
// w_down bf16 [E, h, f] -> out bf16 [T, h]
torch::Tensor moe_ffn(torch::Tensor x, torch::Tensor router_logits, torch::Tensor w_gate,
                      torch::Tensor w_up, torch::Tensor w_down, long top_k) {
  check_router(router_logits, top_k);
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.dtype() == torch::kBFloat16 &&
                  x.is_contiguous(),
              "moe_ffn: x must be contiguous bf16 [T, h] on the GPU");
  const long long T = x.size(0), h = x.size(1), E = router_logits.size(1);
  TORCH_CHECK(router_logits.size(0) == T, "moe_ffn: router_logits must be [T, E]");
  TORCH_CHECK(w_gate.is_cuda() && w_gate.dim() == 3 && w_gate.dtype() == torch::kBFloat16 &&
                  w_gate.is_contiguous() && w_gate.size(0) == E && w_gate.size(2) == h,
              "moe_ffn: w_gate must be contiguous bf16 [E, f, h] on the GPU");
  const long long f = w_gate.size(1);
  TORCH_CHECK(w_up.is_cuda() && w_up.dtype() == torch::kBFloat16 && w_up.is_contiguous() &&
                  w_up.sizes() == w_gate.sizes(),
              "moe_ffn: w_up must match w_gate");
  TORCH_CHECK(w_down.is_cuda() && w_down.dim() == 3 && w_down.dtype() == torch::kBFloat16 &&
                  w_down.is_contiguous() && w_down.size(0) == E && w_down.size(1) == h &&
                  w_down.size(2) == f,
              "moe_ffn: w_down must be contiguous bf16 [E, h, f] on the GPU");
  TORCH_CHECK(h >= 128 && h % 128 == 0 && f >= 128 && f % 128 == 0 && h < (1 << 24) &&
                  f < (1 << 24),
              "moe_ffn: h and f must be multiples of 128");
  auto out = torch::empty({T, h}, x.options());
  if (T == 0) return out;

  const int K = (int)top_k;
  const long long P = T * K;
  hipStream_t stream = hypha_stream();
  Routing r = route(router_logits, K, stream);

  const int nc_down = (int)((f + KC - 1) / KC);
  const int cps = down_chunks_per_split(nc_down, h, K, P);
  const int S = (nc_down + cps - 1) / cps;

  auto hbuf = torch::empty({P, f}, x.options());
  auto ybuf = torch::empty({(long long)S, P, h}, x.options().dtype(torch::kFloat32));
  const int* offs = r.offsets.data_ptr<int>();
  const int* pairs = r.pairs.data_ptr<int>();
  const float* topw = r.topw.data_ptr<float>();
  hipLaunchKernelGGL(moe_expert_kernel<false>, dim3((unsigned)(f / 32), (unsigned)E, 1),
                     dim3(256), 0, stream, (const short*)x.data_ptr(),
                     (const short*)w_gate.data_ptr(), (const short*)w_up.data_ptr(), offs,
                     pairs, topw, hbuf.data_ptr(), (int)h, (int)f, K, (int)P,
                     (int)((h + KC - 1) / KC));
  hipLaunchKernelGGL(moe_expert_kernel<true>, dim3((unsigned)(h / 64), (unsigned)E, (unsigned)S),
                     dim3(256), 0, stream, (const short*)hbuf.data_ptr(),
                     (const short*)w_down.data_ptr(), (const short*)nullptr, offs, pairs, topw,
                     ybuf.data_ptr(), (int)f, (int)h, K, (int)P, cps);
  const long long n_vec = T * (h / 8);
  hipLaunchKernelGGL(moe_combine_kernel, dim3((unsigned)((n_vec + 255) / 256)), dim3(256), 0,
                     stream, ybuf.data_ptr<float>(), (short*)out.data_ptr(), n_vec, (int)h, K,
                     S, P);
  return out;
}

// x bf16 [T, h], router_logits fp32 [T, E], w_gate8/w_up8 e4m3 [E, f, h] with
// s_gate/s_up fp32 [E, f], w_down8 e4m3 [E, h, f] with s_down fp32 [E, h]
// -> out bf16 [T, h]
torch::Tensor moe_ffn_fp8w(torch::Tensor x, torch::Tensor router_logits, torch::Tensor w_gate8,
                           torch::Tensor s_gate, torch::Tensor w_up8, torch::Tensor s_up,
                           torch::Tensor w_down8, torch::Tensor s_down, long top_k) {
  check_router(router_logits, top_k);
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.dtype() == torch::kBFloat16 &&
                  x.is_contiguous(),
              "moe_ffn_fp8w: x must be contiguous bf16 [T, h] on the GPU");
  const long long T = x.size(0), h = x.size(1), E = router_logits.size(1);
  TORCH_CHECK(router_logits.size(0) == T, "moe_ffn_fp8w: router_logits must be [T, E]");
  auto codes = [&](const torch::Tensor& w, long long rows, long long cols) {
    return w.is_cuda() && w.dim() == 3 && w.dtype() == torch::kFloat8_e4m3fn &&
           w.is_contiguous() && w.size(0) == E && w.size(1) == rows && w.size(2) == cols;
  };
  auto scales = [&](const torch::Tensor& s, long long rows) {
    return s.is_cuda() && s.dim() == 2 && s.dtype() == torch::kFloat32 && s.is_contiguous() &&
           s.size(0) == E && s.size(1) == rows;
  };
  TORCH_CHECK(w_gate8.dim() == 3, "moe_ffn_fp8w: w_gate8 must be [E, f, h]");
  const long long f = w_gate8.size(1);
  TORCH_CHECK(codes(w_gate8, f, h) && codes(w_up8, f, h) && codes(w_down8, h, f),
              "moe_ffn_fp8w: the codes must be contiguous e4m3 [E, f, h], [E, f, h] and "
              "[E, h, f] on the GPU");
  TORCH_CHECK(scales(s_gate, f) && scales(s_up, f) && scales(s_down, h),
              "moe_ffn_fp8w: the scales must be contiguous fp32 [E, f], [E, f] and [E, h] on "
              "the GPU");
  TORCH_CHECK(h >= 128 && h % 128 == 0 && f >= 128 && f % 128 == 0 && h < (1 << 24) &&
                  f < (1 << 24),
              "moe_ffn_fp8w: h and f must be multiples of 128");
  for (const torch::Tensor* t : {&x, &w_gate8, &w_up8, &w_down8, &s_gate, &s_up, &s_down})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                "moe_ffn_fp8w: operands must be 16-byte aligned");
  auto out = torch::empty({T, h}, x.options());
  if (T == 0) return out;

  const int K = (int)top_k;
  const long long P = T * K;
  hipStream_t stream = hypha_stream();
  Routing r = route(router_logits, K, stream);

  const int nc_down = (int)((f + KC8 - 1) / KC8);
  const int cps = down_chunks_per_split(nc_down, h, K, P);
  const int S = (nc_down + cps - 1) / cps;

  auto hbuf = torch::empty({P, 2, f}, x.options());  // hi and lo row of each pair
  auto ybuf = torch::empty({(long long)S, P, h}, x.options().dtype(torch::kFloat32));
  const int* offs = r.offsets.data_ptr<int>();
  const int* pairs = r.pairs.data_ptr<int>();
  const float* topw = r.topw.data_ptr<float>();
  using u8 = unsigned char;
  hipLaunchKernelGGL(moe_expert_fp8w_kernel<false>, dim3((unsigned)(f / 32), (unsigned)E, 1),
                     dim3(256), 0, stream, (const short*)x.data_ptr(),
                     (const u8*)w_gate8.data_ptr(), (const u8*)w_up8.data_ptr(),
                     s_gate.data_ptr<float>(), s_up.data_ptr<float>(), offs, pairs, topw,
                     hbuf.data_ptr(), (int)h, (int)f, K, (int)P, (int)((h + KC8 - 1) / KC8));
  hipLaunchKernelGGL(moe_expert_fp8w_kernel<true>,
                     dim3((unsigned)(h / 64), (unsigned)E, (unsigned)S), dim3(256), 0, stream,
                     (const short*)hbuf.data_ptr(), (const u8*)w_down8.data_ptr(),
                     (const u8*)nullptr, s_down.data_ptr<float>(), (const float*)nullptr, offs,
                     pairs, topw, ybuf.data_ptr(), (int)f, (int)h, K, (int)P, cps);
  const long long n_vec = T * (h / 8);
  hipLaunchKernelGGL(moe_combine_kernel, dim3((unsigned)((n_vec + 255) / 256)), dim3(256), 0,
                     stream, ybuf.data_ptr<float>(), (short*)out.data_ptr(), n_vec, (int)h, K,
                     S, P);
  return out;
}

// x bf16 [T, h], router_logits fp32 [T, E], c_gate/c_up uint8 [E, f, h / 2] with
// e_gate/e_up uint8 [E, f, h / 32], c_down uint8 [E, h, f / 2] with e_down uint8
// [E, h, f / 32] (MXFP4 codes and E8M0 scales) -> out bf16 [T, h]
torch::Tensor moe_ffn_mxfp4w(torch::Tensor x, torch::Tensor router_logits, torch::Tensor c_gate,
                             torch::Tensor e_gate, torch::Tensor c_up, torch::Tensor e_up,
                             torch::Tensor c_down, torch::Tensor e_down, long top_k) {
  const long long f = check_mxfp4_experts("moe_ffn_mxfp4w", x, router_logits, c_gate, e_gate,
                                          c_up, e_up, c_down, e_down, top_k);
  const long long T = x.size(0), h = x.size(1), E = router_logits.size(1);
  auto out = torch::empty({T, h}, x.options());
  if (T == 0) return out;

  const int K = (int)top_k;
  const long long P = T * K;
  hipStream_t stream = hypha_stream();
  Routing r = route(router_logits, K, stream);

  const int nc_down = (int)((f + KC4 - 1) / KC4);
  const int cps = down_chunks_per_split(nc_down, h, K, P);
  const int S = (nc_down + cps - 1) / cps;

  auto hbuf = torch::empty({P, f}, x.options());
  auto ybuf = torch::empty({(long long)S, P, h}, x.options().dtype(torch::kFloat32));
  const int* offs = r.offsets.data_ptr<int>();
  const int* pairs = r.pairs.data_ptr<int>();
  const float* topw = r.topw.data_ptr<float>();
  using u8 = unsigned char;
  constexpr int D = HYPHA_MOE_MXFP4_DEPTH;
  hipLaunchKernelGGL((moe_expert_mxfp4w_kernel<false, D>),
                     dim3((unsigned)(f / 32), (unsigned)E, 1), dim3(256), 0, stream,
                     (const short*)x.data_ptr(), (const u8*)c_gate.data_ptr(),
                     (const u8*)c_up.data_ptr(), (const u8*)e_gate.data_ptr(),
                     (const u8*)e_up.data_ptr(), offs, pairs, topw, hbuf.data_ptr(), (int)h,
                     (int)f, K, (int)P, (int)((h + KC4 - 1) / KC4));
  hipLaunchKernelGGL((moe_expert_mxfp4w_kernel<true, D>),
                     dim3((unsigned)(h / 64), (unsigned)E, (unsigned)S), dim3(256), 0, stream,
                     (const short*)hbuf.data_ptr(), (const u8*)c_down.data_ptr(),
                     (const u8*)nullptr, (const u8*)e_down.data_ptr(), (const u8*)nullptr, offs,
                     pairs, topw, ybuf.data_ptr(), (int)f, (int)h, K, (int)P, cps);
  const long long n_vec = T * (h / 8);
  hipLaunchKernelGGL(moe_combine_kernel, dim3((unsigned)((n_vec + 255) / 256)), dim3(256), 0,
                     stream, ybuf.data_ptr<float>(), (short*)out.data_ptr(), n_vec, (int)h, K,
                     S, P);
  return out;
}

// moe_ffn_mxfp4w on activations rounded to OCP MXFP8: x is quantised once for
// gate and up, silu(g) * u in the gate/up epilogue, and both GEMMs are
// block-scaled MFMAs on the codes as loaded. Route, group, quantise, gate/up,
// down, combine: every launch sized by (T, E, h, f, top_k) alone.
// depth: chunks of weights in flight per wave, 0 = the default (for measuring)
torch::Tensor moe_ffn_mxfp4w_a8(torch::Tensor x, torch::Tensor router_logits,
                                torch::Tensor c_gate, torch::Tensor e_gate, torch::Tensor c_up,
                                torch::Tensor e_up, torch::Tensor c_down, torch::Tensor e_down,
                                long top_k, long depth) {
  check_mxfp4_experts("moe_ffn_mxfp4w_a8", x, router_logits, c_gate, e_gate, c_up, e_up, c_down,
                      e_down, top_k);
  TORCH_CHECK(depth >= 0 && depth <= 2, "moe_ffn_mxfp4w_a8: depth must be 0, 1 or 2");
  auto out = torch::empty(x.sizes(), x.options());
  if (x.size(0) == 0) return out;

  hipStream_t stream = hypha_stream();
  Routing r = route(router_logits, (int)top_k, stream);
  auto [xq, xe] = quantize_mxfp8(x);
  if (depth == 0) depth = HYPHA_MOE_MXFP4_A8_DEPTH;
  if (depth == 1)
    launch_experts_a8<1>(xq, xe, r, c_gate, e_gate, c_up, e_up, c_down, e_down, out, (int)top_k,
                         stream);
  else
    launch_experts_a8<2>(xq, xe, r, c_gate, e_gate, c_up, e_up, c_down, e_down, out, (int)top_k,
                         stream);
  return out;
}
