// The forward tile pipeline shared by the MFMA flash-attention forward
// kernels (attention.hip attn_fwd_kernel, prefill.hip attn_prefill_kernel).
//
// One workgroup = 4 waves = 128 q rows, one wave = 32 q rows, KV tile = 64.
// Per kv tile a kernel stages K and V into LDS (attn_write_tile), runs
// attn_tile_step on every wave that can see the tile, and after the last
// tile calls attn_store_o once. The global loads, the loop, its barriers and
// the wave-skip test stay in the kernels: those really differ.
//  * swapped QK^T: S^T = mfma(A=K, B=Q) so each lane owns ONE q column and
//    the online-softmax state (m, l) is lane-local — no cross-lane reduce
//    beyond the in-reg accumulator sweep + one __shfl_xor(32) half combine.
//  * O is accumulated TRANSPOSED: O^T = mfma(A=V^T, B=P^T), keeping the
//    per-q rescale factor lane-local as well; the epilogue transposes O
//    back through LDS once per q block for coalesced stores.
//  * P^T (f32 accum regs) is packed to bf16 in-register (pack pairs +
//    __builtin_amdgcn_permlane32_swap half exchange) and feeds the PV MFMA
//    B operand directly — no LDS round trip for P.
//  * K tile lives in LDS row-major with an XOR-16 swizzle (bank-conflict
//    free ds_read_b128); V is transposed into LDS at staging time (pitch
//    padded to 72 elems, conflict-free b128 rows).
// 32x32x16 accumulator map used throughout: register r of lane (hi, ln)
// holds row (r & 3) + 8 * (r >> 2) + 4 * hi, column ln.
#pragma once

#include "hip_common.h"

constexpr int KVB = 64;   // kv tile (fwd)
constexpr int QB = 32;    // q rows per wave
constexpr int NWAVE = 4;  // waves per workgroup
constexpr int WGQ = QB * NWAVE;
constexpr int PADV = 8;   // V^T pitch pad (72 elems -> conflict-free b128)
constexpr int VT_PITCH = KVB + PADV;

// per-thread 8-element chunks of one staged tile (256 threads)
template <int HD> constexpr int ATTN_KCH = KVB * HD / 8 / 256;
template <int HD> constexpr int ATTN_VCH = HD / 32;

__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
  return (unsigned)(unsigned short)f2bf(lo) | ((unsigned)(unsigned short)f2bf(hi) << 16);
}

// Swizzled byte offset inside the K tile: row-major [KVB][HD] bf16 with
// byte ^= (row & 15) << 4 (guide G4 XOR swizzle: conflict-free on
// ds_read_b128 when the 16-lane group's rows are distinct mod 16 — ours are).
template <int HD>
__device__ __forceinline__ int k_lds_off(int row, int elem) {
  return (row * HD + elem) * 2 ^ ((row & 15) << 4);
}

// Which part of the tile a thread stages. K: chunk c covers kv row
// attn_k_row(c, tid), elements attn_k_e0(c, tid) .. +8. V: every chunk i of a
// thread belongs to kv row attn_v_row(tid), elements attn_v_e0(i, tid) .. +8.
// The kernels' global loads and attn_write_tile both index through these.
template <int HD>
__device__ __forceinline__ int attn_k_row(int c, int tid) {
  return (c * 256 + tid) / (HD / 8);
}
template <int HD>
__device__ __forceinline__ int attn_k_e0(int c, int tid) {
  return ((c * 256 + tid) % (HD / 8)) * 8;
}
__device__ __forceinline__ int attn_v_row(int tid) { return tid & 63; }
__device__ __forceinline__ int attn_v_e0(int i, int tid) { return (i * 4 + (tid >> 6)) * 8; }

// Tile write: this thread's bf16 K and V chunks (already dequantized in the
// fp8 case) -> swizzled K image and transposed V image. The caller brackets
// this with the loop's two barriers.
template <int HD>
__device__ __forceinline__ void attn_write_tile(short* k_lds, short* vt_lds, int tid,
                                                const s16x8 (&k8)[ATTN_KCH<HD>],
                                                const s16x8 (&v8)[ATTN_VCH<HD>]) {
#pragma unroll
  for (int c = 0; c < ATTN_KCH<HD>; ++c)
    *reinterpret_cast<s16x8*>(
        (char*)k_lds + k_lds_off<HD>(attn_k_row<HD>(c, tid), attn_k_e0<HD>(c, tid))) = k8[c];
  // V^T transpose: lane-per-kv stores walk the contiguous image row
  // (conflict-free; the d-major pattern was a 16-way bank conflict)
#pragma unroll
  for (int i = 0; i < ATTN_VCH<HD>; ++i) {
    const int kvr = attn_v_row(tid);
    const int e0 = attn_v_e0(i, tid);
#pragma unroll
    for (int j = 0; j < 8; ++j) vt_lds[(e0 + j) * VT_PITCH + kvr] = v8[i][j];
  }
}

// Tile step for one wave: S^T = K Q^T, mask, online softmax, O rescale,
// P pack, O^T += V^T P^T. vis is the last kv index this lane's q row may see
// (INT_MAX = no mask). m_run must be finite after the first tile a wave
// processes, i.e. that tile must hold a visible kv for every row: then
// exp(m_run - m_new) is exp(-inf) = 0 there and never exp(-inf + inf), and a
// later tile that is fully masked for a row leaves m_new = m_run. Both
// kernels start at tile 0, where kv 0 is visible to every row.
template <int HD>
__device__ __forceinline__ void attn_tile_step(const short* k_lds, const short* vt_lds,
                                               const s16x8 (&qfrag)[HD / 16],
                                               f32x16 (&ot)[HD / 32], float& m_run,
                                               float& l_run, int kv0, float scale, int vis) {
  constexpr int KC = HD / 16;    // 16-wide k chunks over head dim
  constexpr int DBLK = HD / 32;  // 32-row d blocks
  const int lane = threadIdx.x & 63;
  const int hi = lane >> 5;  // half-wave
  const int ln = lane & 31;

  // ---- S^T = K Q^T : two 32-kv accumulators ----
  f32x16 st[2];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
    f32x16 acc = {};
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
      s16x8 kf = *reinterpret_cast<const s16x8*>(
          (const char*)k_lds + k_lds_off<HD>(32 * mb + ln, 16 * kc + 8 * hi));
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qfrag[kc], acc, 0, 0, 0);
    }
    st[mb] = acc;
  }

  // ---- online softmax over the 32 regs (all kv of this tile, own q) ----
  float tmax = -INFINITY;
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int kv = kv0 + 32 * mb + (r & 3) + 8 * (r >> 2) + 4 * hi;
      float s = st[mb][r] * scale;
      if (kv > vis) s = -INFINITY;
      st[mb][r] = s;
      tmax = fmaxf(tmax, s);
    }
  tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
  const float m_new = fmaxf(m_run, tmax);
  const float alpha = __expf(m_run - m_new);
  float psum = 0.f;
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float p = __expf(st[mb][r] - m_new);
      st[mb][r] = p;
      psum += p;
    }
  psum += __shfl_xor(psum, 32, 64);
  l_run = l_run * alpha + psum;
  m_run = m_new;
#pragma unroll
  for (int db = 0; db < DBLK; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) ot[db][r] *= alpha;

  // ---- pack P^T to bf16 B-fragments (pair-pack + half swap) ----
  s16x8 pfrag[4];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      unsigned c0 = pack_bf16x2(st[mb][8 * half + 0], st[mb][8 * half + 1]);
      unsigned c1 = pack_bf16x2(st[mb][8 * half + 2], st[mb][8 * half + 3]);
      unsigned c2 = pack_bf16x2(st[mb][8 * half + 4], st[mb][8 * half + 5]);
      unsigned c3 = pack_bf16x2(st[mb][8 * half + 6], st[mb][8 * half + 7]);
      auto r02 = __builtin_amdgcn_permlane32_swap(c0, c2, false, false);
      auto r13 = __builtin_amdgcn_permlane32_swap(c1, c3, false, false);
      unsigned frag[4] = {(unsigned)r02[0], (unsigned)r13[0], (unsigned)r02[1],
                          (unsigned)r13[1]};
      pfrag[2 * mb + half] = *reinterpret_cast<s16x8*>(frag);
    }
  }

  // ---- O^T += V^T P^T ----
#pragma unroll
  for (int db = 0; db < DBLK; ++db) {
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      s16x8 vf = *reinterpret_cast<const s16x8*>(
          vt_lds + (32 * db + ln) * VT_PITCH + 16 * kc + 8 * hi);
      ot[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pfrag[kc], ot[db], 0, 0, 0);
    }
  }
}

// Epilogue for one wave: normalize, transpose through the wave's own LDS
// slice ot_lds [QB][HD + 8], coalesced 16-byte stores of the rows
// q0 + row < nrows to og + (q0 + row) * row_stride. No barrier inside: the
// slice is private to the wave.
template <int HD>
__device__ __forceinline__ void attn_store_o(const f32x16 (&ot)[HD / 32], float l_run,
                                             short* ot_lds, short* og, long long row_stride,
                                             int q0, int nrows) {
  constexpr int DBLK = HD / 32;
  constexpr int OPITCH = HD + 8;
  const int lane = threadIdx.x & 63;
  const int hi = lane >> 5;
  const int ln = lane & 31;
  const float inv_l = l_run > 0.f ? 1.f / l_run : 0.f;
#pragma unroll
  for (int db = 0; db < DBLK; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int d = 32 * db + (r & 3) + 8 * (r >> 2) + 4 * hi;
      ot_lds[ln * OPITCH + d] = f2bf(ot[db][r] * inv_l);
    }
  __builtin_amdgcn_s_waitcnt(0);  // lgkmcnt(0): own-wave LDS writes visible
#pragma unroll
  for (int it = 0; it < QB * HD / 8 / 64; ++it) {
    int c = it * 64 + lane;
    int row = c / (HD / 8), e0 = (c % (HD / 8)) * 8;
    if (q0 + row < nrows) {
      s16x8 o8 = *reinterpret_cast<const s16x8*>(ot_lds + row * OPITCH + e0);
      *reinterpret_cast<s16x8*>(og + (long long)(q0 + row) * row_stride + e0) = o8;
    }
  }
}
