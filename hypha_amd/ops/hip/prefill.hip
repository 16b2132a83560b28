// Prefill attention over the KV cache for CDNA4 (gfx950): ragged prompts
// (any s >= 1) and chunked continuation (pos > 0), bf16 or fp8-e4m3 cache.
//
// Problem shape: q [B, s, Hq, D] bf16 (bshd) holds the chunk's queries, q
// row i sitting at absolute position pos + i. The chunk's own K/V rows are
// already appended, so the cache [B, T_alloc, Hkv, D] (bshd, read in place —
// the layout KVCache and decode.hip use) is valid for t = pos + s rows.
// kv index j is visible to q row i iff j <= pos + i.
//
// The tile pipeline is attn_tile.h's, shared with attn_fwd_kernel
// (attention.hip) and documented there; the fragment maps are verified by
// probe.hip. What differs from attn_fwd_kernel:
//  * the causal diagonal is shifted by pos; the per-workgroup kv bound is
//    min(t, pos + q0wg + 128);
//  * q rows >= s load zeros and are never stored (in bshd the row after the
//    last one belongs to the next batch);
//  * kv rows >= the workgroup bound are STAGED AS ZEROS, never loaded: no
//    read past T_alloc, and no stale or non-finite cache tail (a masked
//    p = 0 times a NaN V would still poison O);
//  * QUANT=true dequantizes e4m3 rows (per-row fp32 scale) while writing the
//    LDS images, as decode.hip does, so the MFMA phases are shared.
//  * seq_lens (optional, int32 [B], right-padded batches): sequence b is
//    valid for len_b = clamp(seq_lens[b], 0, pos + s) rows, so this chunk
//    holds s_b = max(0, len_b - pos) live q rows. s_b and len_b replace s and
//    t in every bound below; a workgroup with no live row returns at once,
//    and the (pre-zeroed) output rows >= s_b are never written.
//  * PAGED=true: the cache is a pool [n_pages, KVB, Hkv, D] and logical row j
//    of sequence b is row j % KVB of page block_table[b, j / KVB]. kv tiles
//    start at multiples of KVB, so one staged tile is one page: load_tile
//    looks the tile's page up (one workgroup-uniform load, clamped to the
//    pool) and nothing else changes. It is only called for kv0 < kv_end, so
//    a table slot past the sequence's pages is never read. T_alloc is then
//    max_pages * KVB.
// No lse, no backward. Grid (ceil(s/128), B*Hq): a short chunk against a
// long prefix runs few workgroups (no split-KV).

#include <torch/extension.h>

#include "attn_tile.h"
#include "hip_common.h"

namespace {

// 8 e4m3 bytes * row scale -> 8 bf16 (fp32 multiply, RNE: the same values
// KVCache.dequant produces)
__device__ __forceinline__ s16x8 dequant8(uint2 raw, float sc) {
  s16x8 o;
  o[0] = f2bf(__builtin_amdgcn_cvt_f32_fp8(raw.x, 0) * sc);
  o[1] = f2bf(__builtin_amdgcn_cvt_f32_fp8(raw.x, 1) * sc);
  o[2] = f2bf(__builtin_amdgcn_cvt_f32_fp8(raw.x, 2) * sc);
  o[3] = f2bf(__builtin_amdgcn_cvt_f32_fp8(raw.x, 3) * sc);
  o[4] = f2bf(__builtin_amdgcn_cvt_f32_fp8(raw.y, 0) * sc);
  o[5] = f2bf(__builtin_amdgcn_cvt_f32_fp8(raw.y, 1) * sc);
  o[6] = f2bf(__builtin_amdgcn_cvt_f32_fp8(raw.y, 2) * sc);
  o[7] = f2bf(__builtin_amdgcn_cvt_f32_fp8(raw.y, 3) * sc);
  return o;
}

template <int HD, bool QUANT, bool PAGED = false>
__global__ __launch_bounds__(256, 1) void attn_prefill_kernel(
    const short* __restrict__ qg, const void* __restrict__ kgv,
    const void* __restrict__ vgv, const float* __restrict__ kscale,
    const float* __restrict__ vscale, short* __restrict__ og, int Hq, int Hkv,
    int s, int pos, int T_alloc, float scale, const int* __restrict__ seq_lens,
    const int* __restrict__ block_table, int max_pages, int n_pages) {
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
  const int q0wg = blockIdx.x * WGQ;
  // valid cache rows / live q rows of this chunk: the batch's (pos + s, s),
  // or this sequence's own when lengths are given
  const int len_b = seq_lens ? min(max(seq_lens[b], 0), pos + s) : pos + s;
  const int s_b = max(0, len_b - pos);
  if (q0wg >= s_b) return;  // uniform over the workgroup; before any barrier
  const long long q_ss = (long long)Hq * HD;
  const long long qbase = (long long)b * s * q_ss + (long long)hq * HD;
  const long long kvrow0 = (long long)b * T_alloc;  // cache row index of kv 0

  const int q0 = q0wg + wid * QB;   // this wave's q rows
  const int qrow = q0 + ln;         // this lane's q row (its S^T column)
  const bool wave_live = q0 < s_b;  // a wave past the ragged tail only stages
  // last kv index this lane's row may see; rows >= s_b (never stored) are
  // clamped to the valid prefix so their state stays finite too
  const int vis = min(pos + qrow, len_b - 1);
  // exclusive kv bound of this workgroup: >= 1, <= len_b <= T_alloc
  const int kv_end = min(len_b, pos + q0wg + WGQ);

  // ---- Q fragments: B operand of S^T = mfma(K, Q); lane ln = q column ----
  s16x8 qfrag[KC];
#pragma unroll
  for (int kc = 0; kc < KC; ++kc) {
    s16x8 qv = {};
    if (qrow < s_b)
      qv = *reinterpret_cast<const s16x8*>(qg + qbase + (long long)qrow * q_ss +
                                           16 * kc + 8 * hi);
    qfrag[kc] = qv;
  }

  f32x16 ot[DBLK] = {};
  float m_run = -INFINITY, l_run = 0.f;

  // ---- register-staged K/V prefetch: the next tile's global loads are
  // issued before the current tile's MFMA phase. fp8 mode keeps the raw
  // bytes + row scale in registers and converts at the LDS write, so the
  // conversion does not wait on the loads it was meant to hide ----
  constexpr int KCH = ATTN_KCH<HD>, VCH = ATTN_VCH<HD>;  // 8-elem chunks per thread
  s16x8 kreg[KCH], vreg[VCH];  // bf16 chunks (fp8 mode: filled at the LDS write)
  uint2 kraw[KCH], vraw[VCH];  // fp8 mode: raw bytes
  float ksc[KCH], vsc = 0.f;   // fp8 mode: row scales
  auto load_tile = [&](int kv0) {
    // paged: pool row index of this tile's row 0 (kv0 < kv_end <= max_pages * KVB)
    long long prow0 = 0;
    if (PAGED) {
      const int page = block_table[(long long)b * max_pages + kv0 / KVB];
      prow0 = (long long)min(max(page, 0), n_pages - 1) * KVB;
    }
#pragma unroll
    for (int c = 0; c < KCH; ++c) {
      const int row = attn_k_row<HD>(c, tid), e0 = attn_k_e0<HD>(c, tid);
      const bool ok = kv0 + row < kv_end;
      const long long srow =
          PAGED ? (prow0 + row) * Hkv + hkv : (kvrow0 + kv0 + row) * Hkv + hkv;
      if (QUANT) {
        kraw[c] = make_uint2(0u, 0u);
        ksc[c] = 0.f;
        if (ok) {
          kraw[c] = *reinterpret_cast<const uint2*>(
              reinterpret_cast<const unsigned char*>(kgv) + srow * HD + e0);
          ksc[c] = kscale[srow];
        }
      } else {
        s16x8 kv8 = {};
        if (ok)
          kv8 = *reinterpret_cast<const s16x8*>(
              reinterpret_cast<const short*>(kgv) + srow * HD + e0);
        kreg[c] = kv8;
      }
    }
    {
      const int kvr = attn_v_row(tid);
      const bool ok = kv0 + kvr < kv_end;
      const long long srow =
          PAGED ? (prow0 + kvr) * Hkv + hkv : (kvrow0 + kv0 + kvr) * Hkv + hkv;
      if (QUANT) vsc = ok ? vscale[srow] : 0.f;
#pragma unroll
      for (int i = 0; i < VCH; ++i) {
        const int e0 = attn_v_e0(i, tid);
        if (QUANT) {
          vraw[i] = make_uint2(0u, 0u);
          if (ok)
            vraw[i] = *reinterpret_cast<const uint2*>(
                reinterpret_cast<const unsigned char*>(vgv) + srow * HD + e0);
        } else {
          s16x8 v8 = {};
          if (ok)
            v8 = *reinterpret_cast<const s16x8*>(
                reinterpret_cast<const short*>(vgv) + srow * HD + e0);
          vreg[i] = v8;
        }
      }
    }
  };
  auto write_tile = [&]() {
    if (QUANT) {
#pragma unroll
      for (int c = 0; c < KCH; ++c) kreg[c] = dequant8(kraw[c], ksc[c]);
#pragma unroll
      for (int i = 0; i < VCH; ++i) vreg[i] = dequant8(vraw[i], vsc);
    }
    attn_write_tile<HD>(k_lds, vt_lds, tid, kreg, vreg);
  };

  load_tile(0);
  for (int kv0 = 0; kv0 < kv_end; kv0 += KVB) {
    __syncthreads();  // previous tile's LDS consumers done
    write_tile();
    if (kv0 + KVB < kv_end) load_tile(kv0 + KVB);  // prefetch next tile
    __syncthreads();  // this tile's LDS image ready

    // wave fully above the shifted diagonal, or fully past the q tail.
    // Tile 0 is never skipped for a live wave (0 <= pos + q0 + 31), and kv 0
    // is visible to every row (vis >= 0): attn_tile_step's m_run is finite
    // from the first processed tile on.
    if (!wave_live || kv0 > pos + q0 + QB - 1) continue;
    attn_tile_step<HD>(k_lds, vt_lds, qfrag, ot, m_run, l_run, kv0, scale, vis);
  }

  if (!wave_live) return;  // no barrier below this point

  // only the rows < s_b are stored
  attn_store_o<HD>(ot, l_run, ot_lds[wid], og + qbase, q_ss, q0, s_b);
}

torch::Tensor attn_prefill_impl(torch::Tensor q, torch::Tensor kcache,
                                torch::Tensor vcache, const torch::Tensor* kscale,
                                const torch::Tensor* vscale, long pos,
                                const torch::Tensor* seq_lens = nullptr,
                                const torch::Tensor* block_table = nullptr) {
  TORCH_CHECK(q.is_cuda() && kcache.is_cuda() && vcache.is_cuda(),
              "prefill: tensors must be on the GPU");
  TORCH_CHECK(q.dim() == 4 && q.dtype() == torch::kBFloat16 && q.is_contiguous(),
              "prefill: q must be contiguous bf16 [B, s, Hq, D]");
  TORCH_CHECK(kcache.dim() == 4 && kcache.is_contiguous() && vcache.is_contiguous() &&
                  vcache.sizes() == kcache.sizes() && vcache.dtype() == kcache.dtype(),
              "prefill: k/v caches must be contiguous [B, T_alloc, Hkv, D] of one dtype");
  // paged: kcache/vcache are the pools [n_pages, KVB, Hkv, D]; a sequence's
  // logical cache is max_pages * KVB rows
  long max_pages = 0, n_pages = 0;
  const int* bt_ptr = nullptr;
  if (block_table) {
    TORCH_CHECK(block_table->is_cuda() && block_table->dtype() == torch::kInt32 &&
                    block_table->is_contiguous() && block_table->dim() == 2 &&
                    block_table->size(0) == q.size(0) && block_table->size(1) >= 1 &&
                    block_table->size(1) <= (1L << 24),
                "prefill: block_table must be contiguous int32 [B, max_pages]");
    TORCH_CHECK(kcache.size(1) == KVB && kcache.size(0) >= 1 && kcache.size(0) <= (1L << 24),
                "prefill: pools must be [n_pages, 64, Hkv, D]");
    max_pages = block_table->size(1);
    n_pages = kcache.size(0);
    bt_ptr = block_table->data_ptr<int>();
  }
  const bool quant = kcache.dtype() == torch::kFloat8_e4m3fn;
  TORCH_CHECK(quant || kcache.dtype() == torch::kBFloat16,
              "prefill: cache must be bf16 or float8_e4m3fn");
  const long B = q.size(0), s = q.size(1), Hq = q.size(2), HD = q.size(3);
  const long T_alloc = block_table ? max_pages * KVB : kcache.size(1);
  const long Hkv = kcache.size(2);
  TORCH_CHECK((block_table || kcache.size(0) == B) && kcache.size(3) == HD,
              "prefill: q/cache shape mismatch");
  TORCH_CHECK(HD == 64 || HD == 128, "prefill: head dim must be 64 or 128");
  TORCH_CHECK(Hkv >= 1 && Hq % Hkv == 0, "prefill: Hq must be a multiple of Hkv");
  TORCH_CHECK(s >= 1 && pos >= 0 && pos + s <= T_alloc,
              "prefill: pos + s exceeds the cache (pos=", pos, ", s=", s,
              ", T_alloc=", T_alloc, ")");
  TORCH_CHECK(B * Hq <= 65535 && T_alloc + WGQ < (1L << 31), "prefill: shape too large");
  const float* ksp = nullptr;
  const float* vsp = nullptr;
  if (quant) {
    TORCH_CHECK(kscale && vscale, "prefill: fp8 cache needs row scales");
    for (const torch::Tensor* sc : {kscale, vscale})
      TORCH_CHECK(sc->is_cuda() && sc->dtype() == torch::kFloat32 && sc->is_contiguous() &&
                      sc->dim() == 3 && sc->size(0) == kcache.size(0) &&
                      sc->size(1) == kcache.size(1) && sc->size(2) == Hkv,
                  "prefill: scales must be contiguous fp32 [B, T_alloc, Hkv]");
    ksp = kscale->data_ptr<float>();
    vsp = vscale->data_ptr<float>();
  }

  const int* lens_p = nullptr;
  if (seq_lens) {
    TORCH_CHECK(seq_lens->is_cuda() && seq_lens->dtype() == torch::kInt32 &&
                    seq_lens->is_contiguous() && seq_lens->dim() == 1 &&
                    seq_lens->size(0) == B,
                "prefill: seq_lens must be contiguous int32 [B] on the GPU");
    lens_p = seq_lens->data_ptr<int>();
  }

  // with lengths, the rows past a sequence's end are never written: exact zeros
  auto o = seq_lens ? torch::zeros_like(q) : torch::empty_like(q);
  const float scale = 1.0f / sqrtf((float)HD);
  dim3 grid((unsigned)((s + WGQ - 1) / WGQ), (unsigned)(B * Hq));
  hipStream_t stream = hypha_stream();

#define PREFILL_LAUNCH(HDV, QV)                                                       \
  do {                                                                                \
    if (block_table)                                                                  \
      PREFILL_LAUNCH_P(HDV, QV, true);                                                \
    else                                                                              \
      PREFILL_LAUNCH_P(HDV, QV, false);                                               \
  } while (0)
#define PREFILL_LAUNCH_P(HDV, QV, PV)                                                 \
  hipLaunchKernelGGL((attn_prefill_kernel<HDV, QV, PV>), grid, dim3(256), 0, stream,  \
                     (const short*)q.data_ptr(), (const void*)kcache.data_ptr(),      \
                     (const void*)vcache.data_ptr(), ksp, vsp, (short*)o.data_ptr(),  \
                     (int)Hq, (int)Hkv, (int)s, (int)pos, (int)T_alloc, scale,        \
                     lens_p, bt_ptr, (int)max_pages, (int)n_pages)
  if (HD == 128 && !quant)
    PREFILL_LAUNCH(128, false);
  else if (HD == 128)
    PREFILL_LAUNCH(128, true);
  else if (!quant)
    PREFILL_LAUNCH(64, false);
  else
    PREFILL_LAUNCH(64, true);
#undef PREFILL_LAUNCH
#undef PREFILL_LAUNCH_P
  return o;
}

}  // namespace

// q [B, s, Hq, D] bf16; caches [B, T_alloc, Hkv, D] bf16 (bshd, the chunk's
// own rows already appended); pos = absolute position of q row 0.
// Returns o [B, s, Hq, D] bf16.
torch::Tensor attn_prefill(torch::Tensor q, torch::Tensor kcache, torch::Tensor vcache,
                           long pos) {
  return attn_prefill_impl(q, kcache, vcache, nullptr, nullptr, pos);
}

// fp8 (OCP e4m3) cache with per-row fp32 scales [B, T_alloc, Hkv].
torch::Tensor attn_prefill_fp8(torch::Tensor q, torch::Tensor kcache,
                               torch::Tensor vcache, torch::Tensor kscale,
                               torch::Tensor vscale, long pos) {
  return attn_prefill_impl(q, kcache, vcache, &kscale, &vscale, pos);
}

// Right-padded batches: seq_lens int32 [B] on the device gives each
// sequence's valid length (clamped to [0, pos + s]). Rows and tiles past it
// are skipped, kv rows past it are never read, and output rows past it are
// exact zeros.
torch::Tensor attn_prefill_varlen(torch::Tensor q, torch::Tensor kcache,
                                  torch::Tensor vcache, long pos, torch::Tensor seq_lens) {
  return attn_prefill_impl(q, kcache, vcache, nullptr, nullptr, pos, &seq_lens);
}

torch::Tensor attn_prefill_varlen_fp8(torch::Tensor q, torch::Tensor kcache,
                                      torch::Tensor vcache, torch::Tensor kscale,
                                      torch::Tensor vscale, long pos,
                                      torch::Tensor seq_lens) {
  return attn_prefill_impl(q, kcache, vcache, &kscale, &vscale, pos, &seq_lens);
}

// Paged cache: kpool/vpool [n_pages, 64, Hkv, D] (bf16, or fp8 with scales
// [n_pages, 64, Hkv]) and block_table int32 [B, max_pages] on the device;
// needs pos + s <= max_pages * 64. Semantics and, for the same logical cache,
// output bits of attn_prefill / attn_prefill_varlen.
torch::Tensor attn_prefill_paged(torch::Tensor q, torch::Tensor kpool, torch::Tensor vpool,
                                 std::optional<torch::Tensor> kscale,
                                 std::optional<torch::Tensor> vscale,
                                 torch::Tensor block_table, long pos,
                                 std::optional<torch::Tensor> seq_lens) {
  TORCH_CHECK(kscale.has_value() == vscale.has_value(),
              "prefill: give both scales or none");
  return attn_prefill_impl(q, kpool, vpool, kscale ? &*kscale : nullptr,
                           vscale ? &*vscale : nullptr, pos,
                           seq_lens ? &*seq_lens : nullptr, &block_table);
}
