// Fused causal GQA flash attention, forward, for CDNA4 (gfx950). The
// backward is attention.hip's.
//
// One workgroup = 4 waves x 32 q rows x G query heads of one (batch, kv
// head): the heads of a GQA group see the same keys under the same causal
// bound at the same q rows, so a wave that holds those rows of G heads uses
// every K and V fragment it reads from LDS for G MFMAs, and a tile is loaded,
// staged and waited for once per G heads. G is the largest of {4, 2, 1} that
// divides Hq/Hkv (at D 128 of {2, 1}: four heads' Q fragments and O
// accumulators do not fit 512 registers), chosen on the host.
//
// The tile pipeline — LDS images, swapped QK^T, lane-local online softmax,
// in-register P pack, transposed O and its epilogue — is attn_tile.h's,
// shared with prefill.hip and documented there. This file owns the strided,
// unguarded global loads with register prefetch of the next tile, the two
// LDS buffers and the one barrier per tile, the causal tile bound, wave skip
// and choice of the masked tile body, the launch order and the lse store.

#include <climits>
#include <cstdlib>

#include <torch/extension.h>

#include "attn_tile.h"
#include "hip_common.h"

namespace {

// `pair_order` is a perf-diagnosis switch (HYPHA_ATTN_FWD_ABLATE bit 1,
// default 0): launch the q blocks of a (batch, head group) pair together
// instead of the heaviest q blocks of all pairs first.
template <int HD, int G>
__global__ __launch_bounds__(256, 1) void attn_fwd_kernel(
    const short* __restrict__ qg, const short* __restrict__ kg,
    const short* __restrict__ vg, short* __restrict__ og, float* __restrict__ lseg,
    int B, int Hq, int Hkv, int S, float scale, bool causal,
    long long q_sb, long long q_sh, long long q_ss,  // q/o strides (elements)
    long long kv_sb, long long kv_sh, long long kv_ss, int pair_order) {
  constexpr int KC = HD / 16;        // 16-wide k chunks over head dim
  constexpr int DBLK = HD / 32;      // 32-row d blocks
  constexpr int CH = ATTN_CH<HD>;    // 16-byte chunks per thread and image
  constexpr int RSTEP = 256 / (HD / 8);  // rows between a thread's chunks
  __shared__ __attribute__((aligned(16))) short k_img[2][KVB * HD];
  __shared__ __attribute__((aligned(16))) short v_img[2][KVB * HD];
  __shared__ __attribute__((aligned(16))) short ot_lds[NWAVE][QB * (HD + 8)];  // epilogue transpose

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5;  // half-wave
  const int ln = lane & 31;

  // 1-D grid. Causal: q block nqb-1 walks the most tiles; all pairs' heaviest
  // blocks go first, so the light ones fill in behind them.
  const int nqb = S / WGQ;
  const int hgs = Hq / G;  // head groups per batch
  const int npair = B * hgs;
  int qb, pair;
  if (pair_order) {
    pair = blockIdx.x / nqb;
    qb = blockIdx.x % nqb;
  } else {
    qb = nqb - 1 - blockIdx.x / npair;
    pair = blockIdx.x % npair;
  }
  const int b = pair / hgs;
  const int hq0 = (pair % hgs) * G;  // G | Hq/Hkv: the G heads share hkv
  const int hkv = hq0 / (Hq / Hkv);
  const long long qbase = (long long)b * q_sb + (long long)hq0 * q_sh;
  const long long kvbase = (long long)b * kv_sb + (long long)hkv * kv_sh;

  const int q0wg = qb * WGQ;
  const int q0 = q0wg + wid * QB;   // this wave's q rows
  const int qrow = q0 + ln;         // this lane's q row (its S^T column)
  const int vis = causal ? qrow : INT_MAX;  // last kv index this row may see

  // ---- Q fragments: B operand of S^T = mfma(K, Q); lane ln = q column ----
  s16x8 qfrag[G][KC];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int kc = 0; kc < KC; ++kc)
      qfrag[g][kc] = *reinterpret_cast<const s16x8*>(
          qg + qbase + (long long)g * q_sh + (long long)qrow * q_ss + 16 * kc + 8 * hi);

  f32x16 ot[G][DBLK] = {};
  float m_run[G], l_run[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m_run[g] = -INFINITY;
    l_run[g] = 0.f;
  }

  // ---- register-staged K/V prefetch (guide T14: the next tile's global
  // loads are in flight during a tile's MFMA phase). Chunk c of a thread is
  // row attn_ch_row(c, tid) = tid / (HD/8) + RSTEP * c: a wave-uniform 64-bit
  // base plus one 32-bit lane offset ----
  const AttnLaneOffs lo = attn_lane_offs(DBLK * 512);
  const unsigned pf_off =
      (unsigned)attn_ch_row<HD>(0, tid) * (unsigned)kv_ss + attn_ch_e0<HD>(tid);
  s16x8 kreg[CH], vreg[CH];
  auto load_tile = [&](int kv0) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const long long tile = kvbase + (long long)(kv0 + RSTEP * c) * kv_ss;  // uniform
      kreg[c] = *reinterpret_cast<const s16x8*>(kg + tile + pf_off);
      vreg[c] = *reinterpret_cast<const s16x8*>(vg + tile + pf_off);
    }
  };

  const float c2 = 1.4426950408889634f * scale;  // exp(scale*x) = exp2(c2*x)
  const int kv_end = causal ? (q0wg + WGQ) : S;  // exclusive upper bound
  load_tile(0);
  int buf = 0;
  for (int kv0 = 0; kv0 < kv_end; kv0 += KVB) {
    // ---- write the prefetched tile into this tile's images. The barrier
    // before last settled the reads of images [buf] (two tiles ago) ----
    attn_write_tile<HD>(k_img[buf], v_img[buf], tid, kreg, vreg);
    // the only barrier of the tile: images [buf] ready, and nobody reads
    // images [buf ^ 1] (the previous tile's) any more
    __syncthreads();
    if (kv0 + KVB < kv_end) load_tile(kv0 + KVB);  // prefetch next tile

    if (!(causal && kv0 > q0 + QB - 1)) {  // else: wave fully above the diagonal
      // the masked body only where the tile crosses the diagonal of the
      // wave's first row; the G heads sit at the same rows
      if (causal && kv0 + KVB - 1 > q0)
        attn_tile_step<HD, G, true>(k_img[buf], v_img[buf], lo, qfrag, ot, m_run, l_run, kv0,
                                    c2, vis);
      else
        attn_tile_step<HD, G, false>(k_img[buf], v_img[buf], lo, qfrag, ot, m_run, l_run, kv0,
                                     c2, vis);
    }
    buf ^= 1;
  }

  // lse in natural-log units: m_run is in units of log2(e) * scale * score
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (lane < 32)
      lseg[((long long)b * Hq + hq0 + g) * S + qrow] =
          __builtin_fmaf(m_run[g], 0.6931471805599453f, __logf(fmaxf(l_run[g], 1e-30f)));
    // the wave's own slice, reused head after head: a wave's LDS accesses
    // complete in order
    attn_store_o<HD>(ot[g], l_run[g], ot_lds[wid], og + qbase + (long long)g * q_sh, q_ss, q0,
                     S);
  }
}

}  // namespace

// layout: "bhsd" = [B,H,S,D] contiguous; "bshd" = [B,S,H,D] contiguous
// (the model's natural projection layout — no transpose copies needed).
std::vector<torch::Tensor> attn_fwd_ex(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                                       bool causal, const std::string& layout) {
  // every check runs before the launch: a mis-shaped tensor reaching the
  // kernel is an out-of-bounds access
  auto bf16_dense = [](const torch::Tensor& t) {
    return t.is_cuda() && t.dim() == 4 && t.dtype() == torch::kBFloat16 && t.is_contiguous();
  };
  TORCH_CHECK(bf16_dense(q), "attn_fwd: q must be a contiguous 4-D bf16 tensor");
  TORCH_CHECK(layout == "bhsd" || layout == "bshd", "attn_fwd: layout must be bhsd or bshd");
  const bool bshd = layout == "bshd";
  const int B = q.size(0);
  const int Hq = bshd ? q.size(2) : q.size(1);
  const int S = bshd ? q.size(1) : q.size(2);
  const int HD = q.size(3);
  TORCH_CHECK(bf16_dense(k) && k.size(0) == B && k.size(3) == HD &&
                  (bshd ? k.size(1) : k.size(2)) == S,
              "attn_fwd: k must be a contiguous bf16 tensor with q's batch, seq len and "
              "head dim");
  const int Hkv = bshd ? k.size(2) : k.size(1);
  TORCH_CHECK(bf16_dense(v) && v.sizes() == k.sizes(),
              "attn_fwd: v must be a contiguous bf16 tensor of k's shape");
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0 && (HD == 64 || HD == 128));
  TORCH_CHECK(S % WGQ == 0, "seq len must be a multiple of 128");
  auto o = torch::empty_like(q);
  auto lse = torch::empty({B, Hq, S}, q.options().dtype(torch::kFloat32));
  if (q.numel() == 0) return {o, lse};
  const float scale = 1.0f / sqrtf((float)HD);
  hipStream_t stream = hypha_stream();
  long long q_sb, q_sh, q_ss, kv_sb, kv_sh, kv_ss;
  if (bshd) {
    q_sh = HD; q_ss = (long long)Hq * HD; q_sb = (long long)S * Hq * HD;
    kv_sh = HD; kv_ss = (long long)Hkv * HD; kv_sb = (long long)S * Hkv * HD;
  } else {
    q_ss = HD; q_sh = (long long)S * HD; q_sb = (long long)Hq * S * HD;
    kv_ss = HD; kv_sh = (long long)S * HD; kv_sb = (long long)Hkv * S * HD;
  }

  // perf diagnosis (default 0 = full): 1 = pair launch order, 2 = one head
  // per wave (G = 1) whatever the group size, 4 = two heads at most
  static const int fwd_ablate = [] {
    const char* e = getenv("HYPHA_ATTN_FWD_ABLATE");
    return e ? atoi(e) : 0;
  }();
  const int grp = Hq / Hkv;
  int G = grp % 4 == 0 ? 4 : grp % 2 == 0 ? 2 : 1;
  if (HD == 128 && G > 2) G = 2;
  if ((fwd_ablate & 4) && G > 2) G = 2;
  if (fwd_ablate & 2) G = 1;
  const long long nwg = (long long)(S / WGQ) * B * (Hq / G);
  TORCH_CHECK(nwg < (1LL << 31), "attn_fwd: grid too large");

#define LAUNCH_FWD(HDV, GV)                                                              \
  hipLaunchKernelGGL((attn_fwd_kernel<HDV, GV>), dim3((unsigned)nwg), dim3(256), 0,      \
                     stream, (const short*)q.data_ptr(), (const short*)k.data_ptr(),     \
                     (const short*)v.data_ptr(), (short*)o.data_ptr(),                   \
                     lse.data_ptr<float>(), B, Hq, Hkv, S, scale, causal, q_sb, q_sh,    \
                     q_ss, kv_sb, kv_sh, kv_ss, fwd_ablate & 1)
  if (HD == 128) {
    if (G == 2) LAUNCH_FWD(128, 2);
    else LAUNCH_FWD(128, 1);
  } else {
    if (G == 4) LAUNCH_FWD(64, 4);
    else if (G == 2) LAUNCH_FWD(64, 2);
    else LAUNCH_FWD(64, 1);
  }
#undef LAUNCH_FWD
  return {o, lse};
}

std::vector<torch::Tensor> attn_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                                    bool causal) {
  return attn_fwd_ex(q, k, v, causal, "bhsd");
}
