// Fused causal GQA flash attention, forward + backward, for CDNA4 (gfx950).
// Covers K1's attention piece natively — the reference
// delegates this to HF/PyTorch SDPA inside its Python executor.
//
// Forward (one workgroup = 4 waves = 128 q rows; KV tile = 64): the tile
// pipeline — LDS images, swapped QK^T, lane-local online softmax, in-register
// P pack, transposed O and its epilogue — is attn_tile.h's, shared with
// prefill.hip and documented there. This file owns the strided, unguarded
// global loads with register prefetch of the next tile, the causal tile
// bound and wave skip, and the lse store.
//
// Backward (attn_bwd_keylane_kernel; one workgroup = 4 waves = 256 keys of
// one (batch, kv head), each wave owning 64 keys, all waves walking all
// q-tiles together): recomputes P from q/k/lse (FA2-style) with the key on
// the MFMA lane, so the packed P and dS accumulators are the B operands of
// the dV^T and dK^T products and only dS crosses LDS, once, for dQ. Q, dO and
// K have one LDS image each, read by rows and (ds_read_b64_tr_b16) by
// columns; V stays in registers. dK/dV are complete per wave and stored
// directly as bf16; dQ is one pass of global f32 atomics per 256 keys,
// deferred by one q-tile so that it overlaps the next tile's MFMA work.

#include <climits>

#include <torch/extension.h>

#include "attn_tile.h"
#include "hip_common.h"

namespace {

template <int HD>
__global__ __launch_bounds__(256, 1) void attn_fwd_kernel(
    const short* __restrict__ qg, const short* __restrict__ kg,
    const short* __restrict__ vg, short* __restrict__ og, float* __restrict__ lseg,
    int B, int Hq, int Hkv, int S, float scale, bool causal,
    long long q_sb, long long q_sh, long long q_ss,  // q/o strides (elements)
    long long kv_sb, long long kv_sh, long long kv_ss) {
  constexpr int KC = HD / 16;        // 16-wide k chunks over head dim
  constexpr int DBLK = HD / 32;      // 32-row d blocks
  __shared__ __attribute__((aligned(16))) short k_lds[KVB * HD];
  __shared__ __attribute__((aligned(16))) short vt_lds[HD * VT_PITCH];
  __shared__ __attribute__((aligned(16))) short ot_lds[NWAVE][QB * (HD + 8)];  // epilogue transpose

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int hi = lane >> 5;  // half-wave
  const int ln = lane & 31;

  const int bh = blockIdx.y;
  const int b = bh / Hq;
  const int hq = bh % Hq;
  const int hkv = hq / (Hq / Hkv);
  const long long qbase = (long long)b * q_sb + (long long)hq * q_sh;
  const long long kvbase = (long long)b * kv_sb + (long long)hkv * kv_sh;

  const int q0wg = blockIdx.x * WGQ;
  const int q0 = q0wg + wid * QB;   // this wave's q rows
  const int qrow = q0 + ln;         // this lane's q row (its S^T column)
  const int vis = causal ? qrow : INT_MAX;  // last kv index this row may see

  // ---- Q fragments: B operand of S^T = mfma(K, Q); lane ln = q column ----
  s16x8 qfrag[KC];
#pragma unroll
  for (int kc = 0; kc < KC; ++kc)
    qfrag[kc] = *reinterpret_cast<const s16x8*>(qg + qbase + (long long)qrow * q_ss +
                                                16 * kc + 8 * hi);

  f32x16 ot[DBLK] = {};
  float m_run = -INFINITY, l_run = 0.f;

  // ---- register-staged K/V prefetch (guide T14: issue the next tile's
  // global loads before computing the current one; HBM latency hides under
  // the MFMA phase instead of stalling every wave at the staging barrier) --
  s16x8 kreg[ATTN_KCH<HD>];
  s16x8 vreg[ATTN_VCH<HD>];
  auto load_tile = [&](int kv0) {
#pragma unroll
    for (int c = 0; c < ATTN_KCH<HD>; ++c)
      kreg[c] = *reinterpret_cast<const s16x8*>(
          kg + kvbase + (long long)(kv0 + attn_k_row<HD>(c, tid)) * kv_ss +
          attn_k_e0<HD>(c, tid));
#pragma unroll
    for (int i = 0; i < ATTN_VCH<HD>; ++i)
      vreg[i] = *reinterpret_cast<const s16x8*>(
          vg + kvbase + (long long)(kv0 + attn_v_row(tid)) * kv_ss + attn_v_e0(i, tid));
  };

  const int kv_end = causal ? (q0wg + WGQ) : S;  // exclusive upper bound
  load_tile(0);
  for (int kv0 = 0; kv0 < kv_end; kv0 += KVB) {
    __syncthreads();  // previous tile's LDS consumers done
    attn_write_tile<HD>(k_lds, vt_lds, tid, kreg, vreg);
    if (kv0 + KVB < kv_end) load_tile(kv0 + KVB);  // prefetch next tile
    __syncthreads();  // this tile's LDS image ready

    if (causal && kv0 > q0 + QB - 1) continue;  // wave fully above the diagonal
    attn_tile_step<HD>(k_lds, vt_lds, qfrag, ot, m_run, l_run, kv0, scale, vis);
  }

  if (lane < 32) lseg[(long long)bh * S + qrow] = m_run + __logf(fmaxf(l_run, 1e-30f));
  attn_store_o<HD>(ot, l_run, ot_lds[wid], og + qbase, q_ss, q0, S);
}

}  // namespace

// layout: "bhsd" = [B,H,S,D] contiguous; "bshd" = [B,S,H,D] contiguous
// (the model's natural projection layout — no transpose copies needed).
std::vector<torch::Tensor> attn_fwd_ex(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                                       bool causal, const std::string& layout) {
  TORCH_CHECK(q.dim() == 4 && q.dtype() == torch::kBFloat16 && q.is_contiguous());
  const bool bshd = layout == "bshd";
  const int B = q.size(0);
  const int Hq = bshd ? q.size(2) : q.size(1);
  const int S = bshd ? q.size(1) : q.size(2);
  const int HD = q.size(3);
  const int Hkv = bshd ? k.size(2) : k.size(1);
  TORCH_CHECK(Hq % Hkv == 0 && (HD == 64 || HD == 128));
  TORCH_CHECK(S % WGQ == 0, "seq len must be a multiple of 128");
  auto o = torch::empty_like(q);
  auto lse = torch::empty({B, Hq, S}, q.options().dtype(torch::kFloat32));
  const float scale = 1.0f / sqrtf((float)HD);
  dim3 grid(S / WGQ, B * Hq);
  hipStream_t stream = hypha_stream();
  long long q_sb, q_sh, q_ss, kv_sb, kv_sh, kv_ss;
  if (bshd) {
    q_sh = HD; q_ss = (long long)Hq * HD; q_sb = (long long)S * Hq * HD;
    kv_sh = HD; kv_ss = (long long)Hkv * HD; kv_sb = (long long)S * Hkv * HD;
  } else {
    q_ss = HD; q_sh = (long long)S * HD; q_sb = (long long)Hq * S * HD;
    kv_ss = HD; kv_sh = (long long)S * HD; kv_sb = (long long)Hkv * S * HD;
  }
#define LAUNCH_FWD(HDV)                                                                 \
  hipLaunchKernelGGL(attn_fwd_kernel<HDV>, grid, dim3(256), 0, stream,                  \
                     (const short*)q.data_ptr(), (const short*)k.data_ptr(),            \
                     (const short*)v.data_ptr(), (short*)o.data_ptr(),                  \
                     lse.data_ptr<float>(), B, Hq, Hkv, S, scale, causal, q_sb, q_sh,   \
                     q_ss, kv_sb, kv_sh, kv_ss)
  if (HD == 128)
    LAUNCH_FWD(128);
  else
    LAUNCH_FWD(64);
#undef LAUNCH_FWD
  return {o, lse};
}

std::vector<torch::Tensor> attn_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                                    bool causal) {
  return attn_fwd_ex(q, k, v, causal, "bhsd");
}

// ===========================================================================
// Backward
// ===========================================================================

namespace {

// Di = rowsum(dO * O) per (b,h,q) row — FA2 preprocess. HD/8 lanes per row,
// 16 bytes of dO and O per lane: a wave covers 512/HD rows.
template <int HD>
__global__ void attn_bwd_di_kernel(const short* __restrict__ dog,
                                   const short* __restrict__ og,
                                   float* __restrict__ dig, long long nrows, int Hq,
                                   int S, long long sb, long long sh, long long ss) {
  constexpr int LPR = HD / 8;     // lanes per row
  constexpr int RPB = 256 / LPR;  // rows per block
  const long long row = (long long)blockIdx.x * RPB + threadIdx.x / LPR;
  float acc = 0.f;
  if (row < nrows) {
    const long long b = row / ((long long)Hq * S);
    const long long h = (row / S) % Hq;
    const long long sq = row % S;
    const long long addr = b * sb + h * sh + sq * ss + (threadIdx.x % LPR) * 8;
    const s16x8 d8 = *reinterpret_cast<const s16x8*>(dog + addr);
    const s16x8 o8 = *reinterpret_cast<const s16x8*>(og + addr);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += bf2f(d8[j]) * bf2f(o8[j]);
  }
#pragma unroll
  for (int off = LPR / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (row < nrows && threadIdx.x % LPR == 0) dig[row] = acc;
}

__global__ void cast_f32_to_bf16_kernel(const float* __restrict__ in,
                                        short* __restrict__ out, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x * 4;
  for (long long base = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; base < n;
       base += stride) {
    if (base + 4 <= n) {
      f32x4 v = *reinterpret_cast<const f32x4*>(in + base);
      s16x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = f2bf(v[j]);
      *reinterpret_cast<s16x4*>(out + base) = o;
    } else {
      for (long long i = base; i < n; ++i) out[i] = f2bf(in[i]);
    }
  }
}

// ---- LDS images of the backward kernel ------------------------------------
// Byte offset of element `elem` of row `row` in a [rows][HD] bf16 image laid
// out as 8-row x 32-column subtiles of 512 B whose 16-byte chunks are XORed
// with (row >> 2) & 3: one image serves 16-byte row reads and
// ds_read_b64_tr_b16 column reads, and the 32x32x16 operand reads of a
// 32-row tile need two address registers of each kind, the rest being
// constants (the kernel's rd_base / tr_base / trk_base spell those out; this
// function is the definition they follow). The XOR moves 16-byte chunks, so a
// lane's 8-byte piece of a transposed read is not at base + 8 * p.
template <int HD>
__device__ __forceinline__ int img_off(int row, int elem) {
  const int ch = elem >> 3;
  return (HD / 32) * 512 * (row >> 3) + 512 * (ch >> 2) + 64 * (row & 7) +
         16 * ((ch & 3) ^ ((row >> 2) & 3)) + 2 * (elem & 7);
}

// dS image [key][32 q] bf16, 64-byte rows, addressed in 8-byte units of 4 q
// rows; the unit index is XORed with (key >> 2) & 7 so that the 32 lanes of
// a half (32 keys, one unit each) store to 32 distinct bank pairs.
__device__ __forceinline__ int ds_off(int key, int unit) {
  return key * 64 + ((unit ^ ((key >> 2) & 7)) << 3);
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
// read in that k order (tr_a_off below does).
__device__ __forceinline__ s16x8 acc_frag(const f32x16& x, int s) {
  unsigned w[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) w[m] = pack_bf16x2(x[8 * s + 2 * m], x[8 * s + 2 * m + 1]);
  return *reinterpret_cast<s16x8*>(w);
}

// Backward, key on the lane. (v2, v3 and v4 are the removed earlier
// variants; docs/kernels.md and profiles/attn_bwd_keylane.md keep their
// numbers.) One workgroup = 4 waves = 4*KPW keys of one (batch, kv head);
// each wave owns KPW keys (KPW/32 tiles of 32) and keeps their dK^T and dV^T
// in accumulators while the workgroup sweeps its query heads x 32-row q-tiles.
//   * S = mfma(Q, K) and dP = mfma(dO, V): query rows in the 16 registers,
//     key on the lane. Their accumulators start from -lse*sqrt(D) and -Di, so
//     P = exp2(c*S) and dS = P*dP with no subtraction; packed to bf16 they ARE
//     the B operands of dV^T += dO^T P and dK^T += Q^T dS (acc_frag).
//   * Q and dO tiles are staged once, row-major, 16-byte stores, double
//     buffered and register-prefetched one tile ahead; S/dP read them by rows,
//     dV^T/dK^T by columns (ds_read_b64_tr_b16). K has one image, read by rows
//     for S and by columns for dQ. V lives in registers as B fragments.
//   * dS crosses LDS once, as a [key][q] image of packed 8-byte stores, read
//     back transposed as dQ's A operand. dQ = dS K is deferred one q-tile (one
//     barrier per tile) and added with fp32 atomics, one d-block per wave.
//   * 1/sqrt(D) is applied to dK at the store and to dQ before the atomics.
// Keys at or past S (a half block) are whole 32-key tiles: they are staged as
// zeros, never computed, stored or added.
// `ablate` is a perf-diagnosis bitmask (HYPHA_ATTN_ABLATE, default 0=full):
// 1 = skip the dQ atomics, 2 = skip the whole dQ phase, 4 = skip the exp,
// 8 = launch the key blocks of a (batch, kv head) pair together instead of
// the heaviest key blocks of all pairs first; 16 (host side) = 128-key blocks.
template <int HD, int KPW>
__global__ __launch_bounds__(256, 1) void attn_bwd_keylane_kernel(
    const short* __restrict__ qg, const short* __restrict__ kg,
    const short* __restrict__ vg, const short* __restrict__ dog,
    const float* __restrict__ lseg, const float* __restrict__ dig,
    float* __restrict__ dqg, short* __restrict__ dkg, short* __restrict__ dvg,
    int B, int Hq, int Hkv, int S, float scale, bool causal,
    long long q_sb, long long q_sh, long long q_ss,
    long long kv_sb, long long kv_sh, long long kv_ss, int ablate) {
  constexpr int NH = KPW / 32;     // 32-key tiles per wave
  constexpr int NT = NWAVE * NH;   // 32-key tiles per workgroup
  constexpr int KVW = NWAVE * KPW; // keys per workgroup
  constexpr int QT = 32;           // q rows per tile
  constexpr int KC = HD / 16;
  constexpr int DBLK = HD / 32;
  constexpr int NSTG = HD / 64;    // 16-byte chunks per thread of a staged q-tile
  __shared__ __attribute__((aligned(16))) short k_img[KVW * HD];       // [key][d]
  __shared__ __attribute__((aligned(16))) short q_img[2][QT * HD];     // [q][d]
  __shared__ __attribute__((aligned(16))) short do_img[2][QT * HD];    // [q][d]
  __shared__ __attribute__((aligned(16))) short ds_img[2][KVW * QT];   // [key][q]
  __shared__ __attribute__((aligned(16))) float rc_img[2][2][QT];  // -lse*sqrt(D), -Di

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5;
  const int ln = lane & 31;
  // transposed-read lane roles: lane 4*tq + tp of 16-lane group (hi, tg)
  const int tg = (lane >> 4) & 1;
  const int tq = (lane >> 2) & 3;
  const int tp = lane & 3;

  const int nkb = (S + KVW - 1) / KVW;
  const int npair = B * Hkv;
  int kb, bhkv;
  if (ablate & 8) {
    bhkv = blockIdx.x / nkb;
    kb = blockIdx.x % nkb;
  } else {  // causal: key block 0 sees every q-tile; all pairs' block 0 first
    kb = blockIdx.x / npair;
    bhkv = blockIdx.x % npair;
  }
  const int b = bhkv / Hkv;
  const int hkv = bhkv % Hkv;
  const int G = Hq / Hkv;
  const int kv_base = kb * KVW;
  const long long kvbase = (long long)b * kv_sb + (long long)hkv * kv_sh;
  const int nt_valid = min(NT, (S - kv_base) / 32);  // tiles with keys < S

  // ---- stage K (rows at or past S as zeros); V B-fragments into registers ----
  for (int c = tid; c < KVW * HD / 8; c += 256) {
    const int row = c / (HD / 8), e0 = (c % (HD / 8)) * 8;
    s16x8 k8 = {};
    if (kv_base + row < S)
      k8 = *reinterpret_cast<const s16x8*>(kg + kvbase + (long long)(kv_base + row) * kv_ss + e0);
    *reinterpret_cast<s16x8*>((char*)k_img + img_off<HD>(row, e0)) = k8;
  }
  s16x8 vfrag[NH][KC];
#pragma unroll
  for (int hh = 0; hh < NH; ++hh) {
    const int key = kv_base + wid * KPW + 32 * hh + ln;
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
      s16x8 v8 = {};
      if (key < S)
        v8 = *reinterpret_cast<const s16x8*>(vg + kvbase + (long long)key * kv_ss + 16 * kc +
                                             8 * hi);
      vfrag[hh][kc] = v8;
    }
  }

  f32x16 dk_acc[NH][DBLK] = {};  // D[m=d][n=key], this wave's keys
  f32x16 dv_acc[NH][DBLK] = {};  // D[m=d][n=key]

  const float c2 = 1.4426950408889634f * scale;  // exp(scale*x) = exp2(c2*x)
  const float neg_sqrt_d = -1.0f / scale;
  const int t0 = causal ? kv_base / QT : 0;
  const int Tq = S / QT;

  constexpr int GRP = (HD / 32) * 512;  // bytes of an 8-row group of an image
  // Row read of a 32-row tile: img_off(32n + ln, 16kc + 8hi) =
  // 32n * 2HD + rd_base[kc & 1] + 512 * (kc >> 1).
  int rd_base[2];
#pragma unroll
  for (int par = 0; par < 2; ++par)
    rd_base[par] = GRP * (ln >> 3) + 64 * (ln & 7) + 16 * ((2 * par + hi) ^ ((ln >> 2) & 3));
  auto rd = [&](const short* img, int kc) {
    return *reinterpret_cast<const s16x8*>((const char*)img + rd_base[kc & 1] + 512 * (kc >> 1));
  };
  // A fragment of k-step s of dO^T / Q^T for d-block db, read by columns from
  // the [q][d] image in acc_frag's k order: elements 0..3 are q rows
  // 16s + 4hi + 0..3 (x = 0), elements 4..7 the same + 8 (x = 1); this lane's
  // column is 32db + ln. img_off(16s + 8x + 4hi + tq, 32db + 16tg + 4tp) =
  // tr_base[x] + GRP * (2s + x) + 512 * db.
  int tr_base[2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
    tr_base[x] = 64 * (4 * hi + tq) + 16 * ((2 * tg + (tp >> 1)) ^ (hi + 2 * x)) + 8 * (tp & 1);
  auto tr_a = [&](const short* img, int db, int s) {
    return lds_tr_pair(img, tr_base[0] + GRP * (2 * s) + 512 * db,
                       tr_base[1] + GRP * (2 * s + 1) + 512 * db);
  };
  // dQ operands, natural k order: element j of half hi is key 16kck + 8hi + j.
  // K by columns: img_off(16kck + 8hi + 4x + tq, 32db + 16tg + 4tp) =
  // trk_base[x] + 2 * GRP * kck + 512 * db. dS by columns:
  // ds_off(16kck + 8hi + 4x + tq, 4tg + tp) = trs_base[kck & 1][x] + 2048 * (kck >> 1).
  int trk_base[2], trs_base[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x) {
    trk_base[x] = GRP * hi + 64 * (tq + 4 * x) + 16 * ((2 * tg + (tp >> 1)) ^ (2 * hi + x)) +
                  8 * (tp & 1) + 512 * wid;
#pragma unroll
    for (int par = 0; par < 2; ++par)
      trs_base[par][x] = 1024 * par + 64 * (8 * hi + tq + 4 * x) +
                         8 * ((4 * tg + tp) ^ (4 * par + 2 * hi + x));
  }

  // q-tile staging: thread tid takes 16-byte chunk tid (+ 256i) of the tile
  constexpr int RSTEP = 256 / (HD / 8);  // rows between a thread's chunks
  const unsigned pf_off = (unsigned)(tid / (HD / 8)) * (unsigned)q_ss + (tid % (HD / 8)) * 8;

  // deferred-dQ pipeline state: the previous q-tile whose dS image is
  // complete but whose dQ pass has not run yet (crosses hq boundaries: k_img
  // is per-hkv, shared by every head in the GQA group)
  int prev_q0 = -1, prev_na = 0, buf = 0;
  long long prev_qbase = 0;

  auto run_dq = [&](int dbuf) {
    if (wid >= DBLK || prev_q0 < 0) return;
    const int db = wid;  // trk_base carries 512 * db
    f32x16 dq = {};
    for (int kt = 0; kt < prev_na; ++kt) {  // one 32-key tile = two k-steps
#pragma unroll
      for (int par = 0; par < 2; ++par) {
        s16x8 af = lds_tr_pair(ds_img[dbuf], trs_base[par][0] + 2048 * kt,
                               trs_base[par][1] + 2048 * kt);
        s16x8 bf = lds_tr_pair(k_img, trk_base[0] + 2 * GRP * (2 * kt + par),
                               trk_base[1] + 2 * GRP * (2 * kt + par));
        dq = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, dq, 0, 0, 0);
      }
    }
    if (!(ablate & 1)) {
      // uniform 64-bit base + 32-bit lane offset: addresses stay out of VGPR pairs
      float* tile = dqg + prev_qbase + (long long)prev_q0 * q_ss + 32 * db;
      const unsigned voff = (unsigned)(4 * hi) * (unsigned)q_ss + ln;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        atomicAdd(tile + (long long)((r & 3) + 8 * (r >> 2)) * q_ss + voff, dq[r] * scale);
    } else {
      asm volatile("" ::"v"(dq[0]));  // keep the MFMA chain live (perf probe)
    }
  };

  for (int hq = hkv * G; hq < (hkv + 1) * G; ++hq) {
    const long long qbase = (long long)b * q_sb + (long long)hq * q_sh;
    const long long lsebase = (long long)(b * Hq + hq) * S;

    // prefetch the first q-tile of this head into registers
    s16x8 qreg[NSTG], doreg[NSTG];
    float rcreg = 0.f;
    auto issue_prefetch = [&](int t) {
#pragma unroll
      for (int i = 0; i < NSTG; ++i) {  // chunk tid + 256i: row pf_row + RSTEP * i
        const long long tile = qbase + (long long)(t * QT + RSTEP * i) * q_ss;  // uniform
        qreg[i] = *reinterpret_cast<const s16x8*>(qg + tile + pf_off);
        doreg[i] = *reinterpret_cast<const s16x8*>(dog + tile + pf_off);
      }
      if (wid == 0)
        rcreg = hi ? -dig[lsebase + t * QT + ln] : lseg[lsebase + t * QT + ln] * neg_sqrt_d;
    };
    issue_prefetch(t0);

    for (int t = t0; t < Tq; ++t) {
      const int q0 = t * QT;

      // ---- (a) write the prefetched q-tile into this tile's images ----
#pragma unroll
      for (int i = 0; i < NSTG; ++i) {
        const int c = tid + 256 * i;
        const int off = img_off<HD>(c / (HD / 8), (c % (HD / 8)) * 8);
        *reinterpret_cast<s16x8*>((char*)q_img[buf] + off) = qreg[i];
        *reinterpret_cast<s16x8*>((char*)do_img[buf] + off) = doreg[i];
      }
      if (wid == 0) rc_img[buf][hi][ln] = rcreg;
      // the only barrier of the tile: images [buf] ready, and everything the
      // previous tile wrote (dS [buf^1]) or read (images [buf^1]) is settled
      __syncthreads();

      // ---- (b) issue next tile's loads; they land under the MFMA work ----
      if (t + 1 < Tq) issue_prefetch(t + 1);

      // active 32-key tiles for this q-tile (tiles above the diagonal idle)
      const int na = causal ? min(nt_valid, (q0 + QT - 1 - kv_base) / 32 + 1) : nt_valid;

      // deferred dQ of the PREVIOUS tile: its dS buffer is complete and
      // nobody writes it this phase
      if (!(ablate & 2)) run_dq(buf ^ 1);

#pragma unroll
      for (int hh = 0; hh < NH; ++hh) {
        if (wid * NH + hh >= na) continue;
        const int krow = wid * KPW + 32 * hh + ln;  // this lane's key, in the block
        const short* k_tile = k_img + (wid * KPW + 32 * hh) * HD;
        const int key = kv_base + krow;
        const bool diag = causal && kv_base + wid * KPW + 32 * hh + 31 > q0;

        // ---- S' = Q K^T - lse*sqrt(D): rows = q in registers, key on lane ----
        f32x16 s;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 c4 = *reinterpret_cast<const f32x4*>(&rc_img[buf][0][8 * g + 4 * hi]);
#pragma unroll
          for (int j = 0; j < 4; ++j) s[4 * g + j] = c4[j];
        }
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(rd(q_img[buf], kc), rd(k_tile, kc), s, 0, 0, 0);
        }
        // ---- P = exp2(c2 * S'), causal mask on diagonal tiles ----
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float pv = (ablate & 4) ? s[r] * c2 : __builtin_amdgcn_exp2f(s[r] * c2);
          if (diag && key > q0 + (r & 3) + 8 * (r >> 2) + 4 * hi) pv = 0.f;
          s[r] = pv;
        }
        const s16x8 pf[2] = {acc_frag(s, 0), acc_frag(s, 1)};
        // ---- dV^T += dO^T P (A by columns from the dO image, B = P) ----
#pragma unroll
        for (int db = 0; db < DBLK; ++db)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
            dv_acc[hh][db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                tr_a(do_img[buf], db, ks), pf[ks], dv_acc[hh][db], 0, 0, 0);
        // ---- dP' = dO V^T - Di ----
        f32x16 dp;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 c4 = *reinterpret_cast<const f32x4*>(&rc_img[buf][1][8 * g + 4 * hi]);
#pragma unroll
          for (int j = 0; j < 4; ++j) dp[4 * g + j] = c4[j];
        }
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {
          dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(rd(do_img[buf], kc), vfrag[hh][kc], dp, 0, 0, 0);
        }
        // ---- dS = P dP' (1/sqrt(D) applied to dK and dQ at their stores) ----
#pragma unroll
        for (int r = 0; r < 16; ++r) dp[r] *= s[r];
        const s16x8 dsf[2] = {acc_frag(dp, 0), acc_frag(dp, 1)};
        // the one LDS crossing: registers 4g..4g+3 (q rows 8g + 4hi + 0..3)
        // packed into 8 bytes of this lane's key row
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          s16x4 d4 = (g & 1) ? __builtin_shufflevector(dsf[g >> 1], dsf[g >> 1], 4, 5, 6, 7)
                             : __builtin_shufflevector(dsf[g >> 1], dsf[g >> 1], 0, 1, 2, 3);
          *reinterpret_cast<s16x4*>((char*)ds_img[buf] + ds_off(krow, 2 * g + hi)) = d4;
        }
        // ---- dK^T += Q^T dS (A by columns from the Q image, B = dS) ----
#pragma unroll
        for (int db = 0; db < DBLK; ++db)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
            dk_acc[hh][db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                tr_a(q_img[buf], db, ks), dsf[ks], dk_acc[hh][db], 0, 0, 0);
      }

      prev_q0 = q0;
      prev_na = na;
      prev_qbase = qbase;
      buf ^= 1;
    }
  }

  // drain: the final q-tile's dQ pass, once every wave has written its dS
  __syncthreads();
  if (!(ablate & 2)) run_dq(buf ^ 1);

  // ---- bf16 stores: this wave owns its keys fully; registers 4g..4g+3 are
  // d = 32db + 8g + 4hi + 0..3 of key ln: one 8-byte store ----
#pragma unroll
  for (int hh = 0; hh < NH; ++hh) {
    if (wid * NH + hh >= nt_valid) continue;
    const long long tile = kvbase + (long long)(kv_base + wid * KPW + 32 * hh) * kv_ss;
    const unsigned voff = (unsigned)ln * (unsigned)kv_ss + 4 * hi;
#pragma unroll
    for (int db = 0; db < DBLK; ++db) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        s16x4 k4, v4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          k4[j] = f2bf(dk_acc[hh][db][4 * g + j] * scale);
          v4[j] = f2bf(dv_acc[hh][db][4 * g + j]);
        }
        *reinterpret_cast<s16x4*>(dkg + tile + (32 * db + 8 * g) + voff) = k4;
        *reinterpret_cast<s16x4*>(dvg + tile + (32 * db + 8 * g) + voff) = v4;
      }
    }
  }
}

}  // namespace

// The backward into caller-allocated dq, dk, dv (contiguous bf16 of q's, k's
// and v's shapes): what attn_bwd_ex runs, and what lets a test put guard
// elements around the outputs.
void attn_bwd_into(torch::Tensor q, torch::Tensor k, torch::Tensor v, torch::Tensor o,
                   torch::Tensor dout, torch::Tensor lse, bool causal,
                   const std::string& layout, torch::Tensor dq, torch::Tensor dk,
                   torch::Tensor dv) {
  // every check runs before any launch: a mis-shaped tensor reaching a
  // kernel is an out-of-bounds access
  auto bf16_dense = [](const torch::Tensor& t) {
    return t.is_cuda() && t.dim() == 4 && t.dtype() == torch::kBFloat16 &&
           t.is_contiguous();
  };
  TORCH_CHECK(bf16_dense(q), "attn_bwd: q must be a contiguous 4-D bf16 tensor");
  TORCH_CHECK(layout == "bhsd" || layout == "bshd",
              "attn_bwd: layout must be bhsd or bshd");
  const bool bshd = layout == "bshd";
  const int B = q.size(0);
  const int Hq = bshd ? q.size(2) : q.size(1);
  const int S = bshd ? q.size(1) : q.size(2);
  const int HD = q.size(3);
  TORCH_CHECK(bf16_dense(k) && k.size(0) == B && k.size(3) == HD &&
                  (bshd ? k.size(1) : k.size(2)) == S,
              "attn_bwd: k must be a contiguous bf16 tensor with q's batch, seq len "
              "and head dim");
  const int Hkv = bshd ? k.size(2) : k.size(1);
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0, "attn_bwd: Hq must be a multiple of Hkv");
  TORCH_CHECK(bf16_dense(v) && v.sizes() == k.sizes(),
              "attn_bwd: v must be a contiguous bf16 tensor of k's shape");
  TORCH_CHECK(bf16_dense(o) && o.sizes() == q.sizes(),
              "attn_bwd: o must be a contiguous bf16 tensor of q's shape");
  TORCH_CHECK(bf16_dense(dout) && dout.sizes() == q.sizes(),
              "attn_bwd: dout must be a contiguous bf16 tensor of q's shape");
  TORCH_CHECK(lse.is_cuda() && lse.dtype() == torch::kFloat32 && lse.is_contiguous() &&
                  lse.numel() == (long long)B * Hq * S,
              "attn_bwd: lse must be a contiguous fp32 tensor of B*Hq*S elements");
  TORCH_CHECK(HD == 64 || HD == 128);
  TORCH_CHECK(S % 128 == 0, "seq len must be a multiple of 128");
  TORCH_CHECK(bf16_dense(dq) && dq.sizes() == q.sizes() && bf16_dense(dk) &&
                  dk.sizes() == k.sizes() && bf16_dense(dv) && dv.sizes() == k.sizes(),
              "attn_bwd: dq, dk, dv must be contiguous bf16 tensors of q's, k's and v's shapes");
  auto di = torch::empty({B, Hq, S}, q.options().dtype(torch::kFloat32));
  const float scale = 1.0f / sqrtf((float)HD);
  hipStream_t stream = hypha_stream();
  long long nrows = (long long)B * Hq * S;
  long long q_sb, q_sh, q_ss, kv_sb, kv_sh, kv_ss;
  if (bshd) {
    q_sh = HD; q_ss = (long long)Hq * HD; q_sb = (long long)S * Hq * HD;
    kv_sh = HD; kv_ss = (long long)Hkv * HD; kv_sb = (long long)S * Hkv * HD;
  } else {
    q_ss = HD; q_sh = (long long)S * HD; q_sb = (long long)Hq * S * HD;
    kv_ss = HD; kv_sh = (long long)S * HD; kv_sb = (long long)Hkv * S * HD;
  }

  static const int bwd_ablate = [] {
    const char* e = getenv("HYPHA_ATTN_ABLATE");
    return e ? atoi(e) : 0;
  }();
  auto dq32 = torch::zeros(q.sizes(), q.options().dtype(torch::kFloat32));

#define LAUNCH_BWD(HDV, KPWV)                                                           \
  hipLaunchKernelGGL((attn_bwd_keylane_kernel<HDV, KPWV>),                              \
                     dim3((unsigned)((S + 4 * KPWV - 1) / (4 * KPWV) * B * Hkv)),       \
                     dim3(256), 0, stream, (const short*)q.data_ptr(),                  \
                     (const short*)k.data_ptr(), (const short*)v.data_ptr(),            \
                     (const short*)dout.data_ptr(), lse.data_ptr<float>(),              \
                     di.data_ptr<float>(), dq32.data_ptr<float>(),                      \
                     (short*)dk.data_ptr(), (short*)dv.data_ptr(), B, Hq, Hkv, S,       \
                     scale, causal, q_sb, q_sh, q_ss, kv_sb, kv_sh, kv_ss, bwd_ablate)
#define DISPATCH(HDV)                                                                   \
  do {                                                                                  \
    constexpr int rows_per_block = 2048 / HDV;                                          \
    hipLaunchKernelGGL(attn_bwd_di_kernel<HDV>,                                         \
                       dim3((unsigned)((nrows + rows_per_block - 1) / rows_per_block)), \
                       dim3(256), 0, stream, (const short*)dout.data_ptr(),             \
                       (const short*)o.data_ptr(), di.data_ptr<float>(), nrows, Hq, S,  \
                       q_sb, q_sh, q_ss);                                               \
    if (bwd_ablate & 16)                                                                \
      LAUNCH_BWD(HDV, 32);                                                              \
    else                                                                                \
      LAUNCH_BWD(HDV, 64);                                                              \
  } while (0)

  if (HD == 128)
    DISPATCH(128);
  else
    DISPATCH(64);
#undef DISPATCH
#undef LAUNCH_BWD

  long long n = dq32.numel();
  hipLaunchKernelGGL(cast_f32_to_bf16_kernel, dim3(elementwise_grid((n + 3) / 4)),
                     dim3(256), 0, stream, dq32.data_ptr<float>(), (short*)dq.data_ptr(),
                     n);
}

std::vector<torch::Tensor> attn_bwd_ex(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                                       torch::Tensor o, torch::Tensor dout,
                                       torch::Tensor lse, bool causal,
                                       const std::string& layout) {
  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  auto dv = torch::empty_like(v);
  attn_bwd_into(q, k, v, o, dout, lse, causal, layout, dq, dk, dv);
  return {dq, dk, dv};
}

std::vector<torch::Tensor> attn_bwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                                    torch::Tensor o, torch::Tensor dout,
                                    torch::Tensor lse, bool causal) {
  return attn_bwd_ex(q, k, v, o, dout, lse, causal, "bhsd");
}
