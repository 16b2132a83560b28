// The forward tile pipeline shared by the MFMA flash-attention forward
// kernels (attn_fwd.hip attn_fwd_kernel, prefill.hip attn_prefill_kernel),
// and the LDS image layout it shares with the backward (attention.hip).
//
// One workgroup = 4 waves = 128 q rows, one wave = 32 q rows of G query heads
// of one kv head, KV tile = 64. Per kv tile a kernel stages K and V into LDS
// (attn_write_tile), runs attn_tile_step on every wave that can see the tile,
// and after the last tile calls attn_store_o once per head. The global loads,
// the loop, its barriers and buffers and the wave-skip test stay in the
// kernels: those really differ.
//  * swapped QK^T: S^T = mfma(A=K, B=Q) so each lane owns ONE q column and
//    the online-softmax state (m, l) is lane-local — no cross-lane reduce
//    beyond the in-reg accumulator sweep + one __shfl_xor(32) half combine.
//  * O is accumulated TRANSPOSED: O^T = mfma(A=V^T, B=P^T), keeping the
//    per-q rescale factor lane-local as well; the epilogue transposes O
//    back through LDS once per q block for coalesced stores.
//  * P^T (f32 accum regs) is packed to bf16 in-register (acc_frag) and feeds
//    the PV MFMA B operand directly — no LDS round trip for P. The k order
//    of such a fragment is permuted; V^T is read in that order.
//  * K and V tiles each have ONE row-major image (img_off), written with
//    16-byte stores. K is read by rows (ds_read_b128) as the A operand of
//    S^T; V is read by columns (ds_read_b64_tr_b16, lds_tr_pair) as V^T.
//    probe.hip's mfma_probe_tr_v_operand checks that pairing exactly.
//  * G heads of the GQA group sit at the same q rows under the same causal
//    bound, so every K and V fragment read feeds G MFMAs.
//  * the exponent is exp2 of scores times c2 = log2(e)/sqrt(D): m is kept in
//    those units and the lse store converts back.
// 32x32x16 accumulator map used throughout: register r of lane (hi, ln)
// holds row (r & 3) + 8 * (r >> 2) + 4 * hi, column ln.
#pragma once

#include "hip_common.h"

constexpr int KVB = 64;   // kv tile (fwd)
constexpr int QB = 32;    // q rows per wave
constexpr int NWAVE = 4;  // waves per workgroup
constexpr int WGQ = QB * NWAVE;

// 16-byte chunks per thread of one staged K or V tile (256 threads)
template <int HD> constexpr int ATTN_CH = KVB * HD / 8 / 256;

__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
  return (unsigned)(unsigned short)f2bf(lo) | ((unsigned)(unsigned short)f2bf(hi) << 16);
}

// ---- LDS images ------------------------------------------------------------
// Byte offset of element `elem` of row `row` in a [rows][HD] bf16 image laid
// out as 8-row x 32-column subtiles of 512 B whose 16-byte chunks are XORed
// with (row >> 2) & 3: one image serves 16-byte row reads and
// ds_read_b64_tr_b16 column reads, and the 32x32x16 operand reads of a
// 32-row tile need two address registers of each kind, the rest being
// constants (AttnLaneOffs here and the backward's rd_base / tr_base /
// trk_base spell those out; this function is the definition they follow).
// The XOR moves 16-byte chunks, so a lane's 8-byte piece of a transposed read
// is not at base + 8 * p.
template <int HD>
__device__ __forceinline__ int img_off(int row, int elem) {
  const int ch = elem >> 3;
  return (HD / 32) * 512 * (row >> 3) + 512 * (ch >> 2) + 64 * (row & 7) +
         16 * ((ch & 3) ^ ((row >> 2) & 3)) + 2 * (elem & 7);
}

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// Two ds_read_b64_tr_b16 (4 rows x 16 columns each, delivered column-major)
// joined into one 8-element MFMA fragment.
__device__ __forceinline__ s16x8 lds_tr_pair(const short* img, int off0, int off1) {
  s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)((char*)img + off0));
  s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)((char*)img + off1));
  return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

// Registers 8s .. 8s+7 of a 32x32 accumulator as the bf16 fragment of k-step
// s of a following MFMA that sums over the accumulator's rows. Element j of
// lane half h is row 16s + 8(j>>2) + 4h + (j&3): the other operand must be
// read in that k order (AttnLaneOffs::tr and the backward's tr_a do).
// FINITE: the values are known to be finite (the forward's P is in [0, 1]),
// so gfx950's pair conversion, which rounds to nearest even as f2bf does and
// differs from it only in the NaN it returns, replaces f2bf's integer code.
template <bool FINITE = false>
__device__ __forceinline__ s16x8 acc_frag(const f32x16& x, int s) {
  unsigned w[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    if (FINITE) {
      typedef __attribute__((ext_vector_type(2))) __bf16 hw_bf16x2;
      const f32x2 v = {x[8 * s + 2 * m], x[8 * s + 2 * m + 1]};
      const hw_bf16x2 b = __builtin_convertvector(v, hw_bf16x2);
      w[m] = *reinterpret_cast<const unsigned*>(&b);
    } else {
      w[m] = pack_bf16x2(x[8 * s + 2 * m], x[8 * s + 2 * m + 1]);
    }
  }
  return *reinterpret_cast<s16x8*>(w);
}

// Which part of a tile a thread stages: chunk c covers kv row
// attn_ch_row(c, tid), elements attn_ch_e0(tid) .. +8, of K and of V alike.
// The kernels' global loads and attn_write_tile both index through these.
template <int HD>
__device__ __forceinline__ int attn_ch_row(int c, int tid) {
  return (c * 256 + tid) / (HD / 8);
}
template <int HD>
__device__ __forceinline__ int attn_ch_e0(int tid) {
  return (tid % (HD / 8)) * 8;
}

// Tile write: this thread's bf16 K and V chunks (already dequantized in the
// fp8 case) -> the K and V images, 16-byte stores. The caller's barriers
// separate this from the reads of the same buffer.
template <int HD>
__device__ __forceinline__ void attn_write_tile(short* k_img, short* v_img, int tid,
                                                const s16x8 (&k8)[ATTN_CH<HD>],
                                                const s16x8 (&v8)[ATTN_CH<HD>]) {
#pragma unroll
  for (int c = 0; c < ATTN_CH<HD>; ++c) {
    const int off = img_off<HD>(attn_ch_row<HD>(c, tid), attn_ch_e0<HD>(tid));
    *reinterpret_cast<s16x8*>((char*)k_img + off) = k8[c];
    *reinterpret_cast<s16x8*>((char*)v_img + off) = v8[c];
  }
}

// A lane's byte offsets into a tile image; the rest of every operand address
// is a compile-time constant.
//  rd[par]: row read, A fragment of S^T. img_off(32n + ln, 16kc + 8hi) =
//    4 * GRP * n + rd[kc & 1] + 512 * (kc >> 1), GRP = (HD / 32) * 512 the
//    bytes of an 8-row group.
//  tr[x]: column read, A fragment of k-step s of V^T for d-block db, in
//    acc_frag's k order: elements 0..3 are kv rows 16s + 4hi + 0..3 (x = 0),
//    elements 4..7 the same + 8 (x = 1); this lane's column is 32db + ln.
//    With lane 4*tq + tp of 16-lane group (hi, tg):
//    img_off(16s + 8x + 4hi + tq, 32db + 16tg + 4tp) =
//    tr[x] + GRP * (2s + x) + 512 * db.
struct AttnLaneOffs {
  int rd[2], tr[2];
};
__device__ __forceinline__ AttnLaneOffs attn_lane_offs(int grp_bytes) {
  const int lane = threadIdx.x & 63;
  const int hi = lane >> 5, ln = lane & 31;
  const int tg = (lane >> 4) & 1, tq = (lane >> 2) & 3, tp = lane & 3;
  AttnLaneOffs lo;
#pragma unroll
  for (int x = 0; x < 2; ++x) {
    lo.rd[x] = grp_bytes * (ln >> 3) + 64 * (ln & 7) + 16 * ((2 * x + hi) ^ ((ln >> 2) & 3));
    lo.tr[x] = 64 * (4 * hi + tq) + 16 * ((2 * tg + (tp >> 1)) ^ (hi + 2 * x)) + 8 * (tp & 1);
  }
  return lo;
}

// O^T += V^T P^T for one 64-kv tile and G heads: every V^T fragment read
// feeds G MFMAs. pf[g][2 * mb + s] = acc_frag(P^T of kv 32mb .. 32mb+31, s).
template <int HD, int G>
__device__ __forceinline__ void attn_pv(const short* v_img, const AttnLaneOffs& lo,
                                        const s16x8 (&pf)[G][4], f32x16 (&ot)[G][HD / 32]) {
  constexpr int GRP = (HD / 32) * 512;
#pragma unroll
  for (int db = 0; db < HD / 32; ++db) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const s16x8 vf = lds_tr_pair(v_img, lo.tr[0] + GRP * (2 * ks) + 512 * db,
                                   lo.tr[1] + GRP * (2 * ks + 1) + 512 * db);
#pragma unroll
      for (int g = 0; g < G; ++g)
        ot[g][db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[g][ks], ot[g][db], 0, 0, 0);
    }
  }
}

// Tile step for one wave and its G heads: S^T = K Q^T, mask (MASKED only:
// the caller picks it for tiles that cross the diagonal of some row of the
// wave), online softmax, O rescale, P pack, O^T += V^T P^T. vis is the last
// kv index this lane's q row may see. c2 = log2(e)/sqrt(D); m_run is in
// units of c2 * score. m_run must be finite after the first tile a wave
// processes, i.e. that tile must hold a visible kv for every row: then
// exp2(m_run - m_new) is exp2(-inf) = 0 there and never exp2(-inf + inf), and
// a later tile that is fully masked for a row leaves m_new = m_run. Both
// kernels start at tile 0, where kv 0 is visible to every row.
template <int HD, int G, bool MASKED>
__device__ __forceinline__ void attn_tile_step(const short* k_img, const short* v_img,
                                               const AttnLaneOffs& lo,
                                               const s16x8 (&qfrag)[G][HD / 16],
                                               f32x16 (&ot)[G][HD / 32], float (&m_run)[G],
                                               float (&l_run)[G], int kv0, float c2, int vis) {
  constexpr int KC = HD / 16;    // 16-wide k chunks over head dim
  constexpr int DBLK = HD / 32;  // 32-row d blocks
  constexpr int GRP = DBLK * 512;
  const int hi = (threadIdx.x & 63) >> 5;  // half-wave

  // ---- S^T = K Q^T : two 32-kv accumulators per head, K read once ----
  f32x16 st[G][2];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
    for (int g = 0; g < G; ++g) st[g][mb] = f32x16{};
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
      const s16x8 kf = *reinterpret_cast<const s16x8*>(
          (const char*)k_img + 4 * GRP * mb + lo.rd[kc & 1] + 512 * (kc >> 1));
#pragma unroll
      for (int g = 0; g < G; ++g)
        st[g][mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qfrag[g][kc], st[g][mb], 0, 0, 0);
    }
  }

  // ---- online softmax over the 32 regs (all kv of this tile, own q) ----
  s16x8 pf[G][4];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float tmax = -INFINITY;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (MASKED) {
          const int kv = kv0 + 32 * mb + (r & 3) + 8 * (r >> 2) + 4 * hi;
          if (kv > vis) st[g][mb][r] = -INFINITY;
        }
        tmax = fmaxf(tmax, st[g][mb][r]);
      }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = fmaxf(m_run[g], tmax * c2);  // c2 > 0: max commutes
    const float alpha = __builtin_amdgcn_exp2f(m_run[g] - m_new);
    float psum = 0.f;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(st[g][mb][r], c2, -m_new));
        st[g][mb][r] = p;
        psum += p;
      }
    psum += __shfl_xor(psum, 32, 64);
    l_run[g] = l_run[g] * alpha + psum;
    m_run[g] = m_new;
#pragma unroll
    for (int db = 0; db < DBLK; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) ot[g][db][r] *= alpha;
    // ---- pack P^T to bf16 B-fragments, in registers ----
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int s = 0; s < 2; ++s) pf[g][2 * mb + s] = acc_frag<true>(st[g][mb], s);
  }

  // keep the V^T reads (16 fragments) below the softmax: hoisted above it
  // they spill at G = 2, D = 128 and G = 4, D = 64. 0 scratch there also
  // needs the packed-fp32 option setup.py compiles attn_fwd.hip with.
  __builtin_amdgcn_sched_barrier(0);
  attn_pv<HD, G>(v_img, lo, pf, ot);
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
