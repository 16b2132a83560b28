// KV-cache decode attention (flash-decoding) for single-token generation —
// the MI355X-native serving path (replaces the round-1 Python fp32 matmul
// decode noted in VERDICT.md; reference serves inference through the same
// executor surface, /root/reference/executors' inference flow).
//
// Problem shape: q [B, Hq, D] (one new token per sequence), KV cache
// [B, T_alloc, Hkv, D] (bshd — the projections' natural layout, appended
// in place), valid length t. Decode is BANDWIDTH-bound: the whole K and V
// prefix is read once; all arithmetic is VALU fp32 (MFMA needs matrix
// shapes a 1-token query cannot fill).
//
// Parallelization: grid (nsplits, B*Hkv) — flash-decoding split-KV so small
// batches still fill 256 CUs. One workgroup = 4 waves covers ONE (b, hkv)
// pair and ALL G = Hq/Hkv grouped q-heads over its kv chunk: K/V tiles are
// staged cooperatively into LDS once and shared by every q head (GQA cuts
// cache-read bytes by G vs a per-q-head layout). Each wave owns
// ceil(G/4) heads; per 64-row tile it computes that head's scores (one kv
// row per lane, online softmax) and then accumulates p*V with lanes over
// the head dim. Split partials (o, m, l) merge in a second kernel with the
// standard log-sum-exp rescale.

#include <torch/extension.h>

#include "hip_common.h"

namespace {

constexpr int TILE = 64;  // kv rows per staged tile

__device__ __forceinline__ float e4m3_to_f32(unsigned char b) {
  return __builtin_amdgcn_cvt_f32_fp8((unsigned)b, 0);
}

// ---- main split kernel -------------------------------------------------
// partial_o: [nsplits, B, Hq, D] fp32; partial_ml: [nsplits, B, Hq, 2]
// QUANT=false: bf16 cache rows; QUANT=true: OCP e4m3 rows + one fp32
// scale per (b, t, hkv) row (kscale/vscale) — dequantized during the LDS
// staging pass, so phases A/B are identical and cache reads halve.
// PAGED=true: the cache is a pool [n_pages, TILE, Hkv, D] and logical row j of
// sequence b is row j % TILE of page block_table[b, j / TILE]. A split's
// tiles start at multiples of TILE, so one staged tile is one page: the only
// code that differs is the tile's first row, found through one workgroup-
// uniform table load per tile (clamped: a page id from device memory must
// never address outside the pool). T_alloc is then max_pages * TILE.
template <int HD, bool QUANT, bool PAGED = false>
__global__ __launch_bounds__(256) void attn_decode_kernel(
    const short* __restrict__ qg, const short* __restrict__ kg,
    const short* __restrict__ vg, const float* __restrict__ kscale,
    const float* __restrict__ vscale, float* __restrict__ partial_o,
    float* __restrict__ partial_ml, int B, int Hq, int Hkv, int T_alloc, int t_in,
    const int* __restrict__ t_dev, int t_stride, int nsplits, float scale,
    const int* __restrict__ block_table, int max_pages, int n_pages) {
  constexpr int PITCH = HD + 8;  // shorts; 16B-aligned, conflict-free b128
  __shared__ __attribute__((aligned(16))) short k_t[TILE * PITCH];
  __shared__ __attribute__((aligned(16))) short v_t[TILE * PITCH];
  __shared__ float p_t[4][TILE];

  const int tid = threadIdx.x;
  const int w = tid >> 6;
  const int l = tid & 63;
  const int split = blockIdx.x;
  const int bh = blockIdx.y;
  const int b = bh / Hkv;
  const int hkv = bh % Hkv;
  const int G = Hq / Hkv;
  constexpr int GWMAX = 2;  // compile-time bound: supports G <= 8

  // hipGraph mode: the valid length lives in device memory so one captured
  // graph serves every decode step (t grows between replays). t_stride 0:
  // one length for the batch; t_stride 1: one per sequence (varlen), so the
  // split range below is this workgroup's own sequence's. Clamped: a length
  // from device memory must never index past the cache.
  const int t = t_dev ? min(max(t_dev[b * t_stride], 0), T_alloc) : t_in;

  // this split's kv range (tile-aligned chunks); a sequence shorter than
  // the batch's longest leaves its later splits empty (s0 >= s1)
  const int chunk = ((t + nsplits - 1) / nsplits + TILE - 1) / TILE * TILE;
  const int s0 = split * chunk;
  const int s1 = min(t, s0 + chunk);

  // q rows for this wave's heads, kept in registers (HD/8 x 8 elems).
  // GWMAX is a compile-time constant: a runtime-sized local array is a
  // device VLA (dynamic alloca) and memory-faults on gfx950.
  float qreg[GWMAX][HD];
  int heads[GWMAX];
#pragma unroll
  for (int gw = 0; gw < GWMAX; ++gw) {
    int g = w + 4 * gw;
    heads[gw] = g < G ? hkv * G + g : -1;
    if (heads[gw] >= 0) {
      const short* qp = qg + ((long long)b * Hq + heads[gw]) * HD;
      for (int i = 0; i < HD / 8; ++i) {
        s16x8 v8 = *reinterpret_cast<const s16x8*>(qp + 8 * i);
#pragma unroll
        for (int j = 0; j < 8; ++j) qreg[gw][8 * i + j] = bf2f(v8[j]);
      }
    }
  }

  float m_run[GWMAX], l_run[GWMAX];
  float o_acc[GWMAX][2];  // lane owns d = {2l, 2l+1}
#pragma unroll
  for (int gw = 0; gw < GWMAX; ++gw) {
    m_run[gw] = -1e30f;
    l_run[gw] = 0.f;
    o_acc[gw][0] = o_acc[gw][1] = 0.f;
  }

  const long long row_stride = (long long)Hkv * HD;
  const long long base = ((long long)b * T_alloc) * row_stride + (long long)hkv * HD;

  for (int r0 = s0; r0 < s1; r0 += TILE) {
    const int rows = min(TILE, s1 - r0);
    // paged: pool row index of this tile's row 0 (r0 < t <= max_pages * TILE)
    long long prow0 = 0;
    if (PAGED) {
      const int page = block_table[(long long)b * max_pages + r0 / TILE];
      prow0 = (long long)min(max(page, 0), n_pages - 1) * TILE;
    }
    // ---- cooperative K/V tile staging (8 rows x 512B per instruction;
    //      fp8 mode dequantizes per-row-scaled e4m3 bytes on the way) ----
    if (!QUANT) {
      constexpr int LPR = HD * 2 / 16;  // 16B loads per row
      for (int c = tid; c < TILE * LPR; c += 256) {
        int rr = c / LPR, off = (c % LPR) * 8;  // off in shorts
        if (rr < rows) {
          long long src = PAGED ? (prow0 + rr) * row_stride + (long long)hkv * HD + off
                                : base + (long long)(r0 + rr) * row_stride + off;
          *reinterpret_cast<s16x8*>(k_t + rr * PITCH + off) =
              *reinterpret_cast<const s16x8*>(kg + src);
          *reinterpret_cast<s16x8*>(v_t + rr * PITCH + off) =
              *reinterpret_cast<const s16x8*>(vg + src);
        }
      }
    } else {
      constexpr int LPR = HD / 8;  // 8-byte loads per row
      const unsigned char* k8 = reinterpret_cast<const unsigned char*>(kg);
      const unsigned char* v8 = reinterpret_cast<const unsigned char*>(vg);
      for (int c = tid; c < TILE * LPR; c += 256) {
        int rr = c / LPR, off = (c % LPR) * 8;
        if (rr < rows) {
          long long srow = PAGED ? (prow0 + rr) * Hkv + hkv
                                 : ((long long)b * T_alloc + (r0 + rr)) * Hkv + hkv;
          long long src = srow * HD + off;
          float ks = kscale[srow];
          float vs = vscale[srow];
          uint2 kb = *reinterpret_cast<const uint2*>(k8 + src);
          uint2 vb = *reinterpret_cast<const uint2*>(v8 + src);
          const unsigned char* kbb = reinterpret_cast<const unsigned char*>(&kb);
          const unsigned char* vbb = reinterpret_cast<const unsigned char*>(&vb);
          s16x8 ko, vo;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            ko[j] = f2bf(e4m3_to_f32(kbb[j]) * ks);
            vo[j] = f2bf(e4m3_to_f32(vbb[j]) * vs);
          }
          *reinterpret_cast<s16x8*>(k_t + rr * PITCH + off) = ko;
          *reinterpret_cast<s16x8*>(v_t + rr * PITCH + off) = vo;
        }
      }
    }
    __syncthreads();

#pragma unroll
    for (int gw = 0; gw < GWMAX; ++gw) {
      if (heads[gw] < 0) continue;
      // ---- scores: one kv row per lane ----
      float s = -1e30f;
      if (l < rows) {
        float acc = 0.f;
        const short* kp = k_t + l * PITCH;
        for (int i = 0; i < HD / 8; ++i) {
          s16x8 kv8 = *reinterpret_cast<const s16x8*>(kp + 8 * i);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc += qreg[gw][8 * i + j] * bf2f(kv8[j]);
        }
        s = acc * scale;
      }
      // ---- online softmax (wave-wide) ----
      float m_tile = wave_reduce_max(s);
      float m_new = fmaxf(m_run[gw], m_tile);
      float p = l < rows ? __expf(s - m_new) : 0.f;
      float corr = __expf(m_run[gw] - m_new);
      l_run[gw] = l_run[gw] * corr + wave_reduce_sum(p);
      m_run[gw] = m_new;
      p_t[w][l] = p;
      // lanes covering the head dim rescale their accumulator
      o_acc[gw][0] *= corr;
      o_acc[gw][1] *= corr;
      // ---- o += p * V (lane owns d = {2l, 2l+1}) ----
      if (2 * l < HD) {
        float a0 = 0.f, a1 = 0.f;
        for (int r = 0; r < rows; ++r) {
          float pr = p_t[w][r];
          a0 += pr * bf2f(v_t[r * PITCH + 2 * l]);
          a1 += pr * bf2f(v_t[r * PITCH + 2 * l + 1]);
        }
        o_acc[gw][0] += a0;
        o_acc[gw][1] += a1;
      }
    }
    __syncthreads();
  }

  // ---- write split partials ----
#pragma unroll
  for (int gw = 0; gw < GWMAX; ++gw) {
    if (heads[gw] < 0) continue;
    long long po = (((long long)split * B + b) * Hq + heads[gw]) * HD;
    if (2 * l < HD) {
      partial_o[po + 2 * l] = o_acc[gw][0];
      partial_o[po + 2 * l + 1] = o_acc[gw][1];
    }
    if (l == 0) {
      long long pm = (((long long)split * B + b) * Hq + heads[gw]) * 2;
      partial_ml[pm] = m_run[gw];
      partial_ml[pm + 1] = l_run[gw];
    }
  }
}

// ---- split-merge: one block per (b, hq); thread per head-dim element ----
// An empty split wrote (m=-1e30, l=0, o=0): next to a non-empty one its
// factor exp(-1e30 - m_star) is 0. A sequence of length 0 (varlen: a finished
// sequence) has ONLY empty splits: m_star = -1e30, every f = exp(0) = 1,
// num = 0, den = 0, and 0 / max(den, 1e-30) is an exact +0 in every lane.
template <int HD>
__global__ __launch_bounds__(128) void attn_decode_reduce_kernel(
    const float* __restrict__ partial_o, const float* __restrict__ partial_ml,
    short* __restrict__ out, int B, int Hq, int nsplits) {
  const int bh = blockIdx.x;
  const int d = threadIdx.x;
  float m_star = -1e30f;
  for (int s = 0; s < nsplits; ++s)
    m_star = fmaxf(m_star, partial_ml[((long long)s * B * Hq + bh) * 2]);
  float num = 0.f, den = 0.f;
  for (int s = 0; s < nsplits; ++s) {
    long long pm = ((long long)s * B * Hq + bh) * 2;
    float f = __expf(partial_ml[pm] - m_star);
    den += partial_ml[pm + 1] * f;
    if (d < HD) num += partial_o[((long long)s * B * Hq + bh) * HD + d] * f;
  }
  if (d < HD) out[(long long)bh * HD + d] = f2bf(num / fmaxf(den, 1e-30f));
}

}  // namespace

// q [B, Hq, D] bf16; k/v caches [B, T_alloc, Hkv, D] bf16 (bshd, in-place
// appended); t = valid prefix length INCLUDING the token q was computed
// from. Returns o [B, Hq, D] bf16.
torch::Tensor attn_decode_impl(torch::Tensor q, torch::Tensor kcache,
                               torch::Tensor vcache, long t,
                               const torch::Tensor* t_dev,
                               const torch::Tensor* kscale = nullptr,
                               const torch::Tensor* vscale = nullptr,
                               int t_stride = 0, long max_len = -1,
                               const torch::Tensor* block_table = nullptr) {
  TORCH_CHECK(q.is_cuda() && q.dtype() == torch::kBFloat16 && q.dim() == 3);
  TORCH_CHECK(kcache.dim() == 4 && kcache.is_contiguous() && vcache.is_contiguous());
  const bool quant = kcache.dtype() == torch::kFloat8_e4m3fn;
  TORCH_CHECK(!quant || (kscale && vscale), "fp8 cache needs row scales");
  const int B = q.size(0), Hq = q.size(1), HD = q.size(2);
  const int Hkv = kcache.size(2);
  // paged: kcache/vcache are the pools [n_pages, TILE, Hkv, D] and the
  // logical cache of a sequence is max_pages * TILE rows
  int max_pages = 0, n_pages = 0;
  const int* bt_ptr = nullptr;
  if (block_table) {
    TORCH_CHECK(block_table->is_cuda() && block_table->dtype() == torch::kInt32 &&
                    block_table->is_contiguous() && block_table->dim() == 2 &&
                    block_table->size(0) == B && block_table->size(1) >= 1,
                "decode: block_table must be contiguous int32 [B, max_pages]");
    TORCH_CHECK(kcache.is_cuda() && vcache.is_cuda() && kcache.size(1) == TILE &&
                    kcache.size(0) >= 1 && vcache.sizes() == kcache.sizes() &&
                    vcache.dtype() == kcache.dtype(),
                "decode: pools must be [n_pages, 64, Hkv, D] of one dtype");
    TORCH_CHECK(block_table->size(1) <= (1L << 24) && kcache.size(0) <= (1L << 24),
                "decode: pool or table too large");
    TORCH_CHECK(t_dev && t_stride == 1, "decode: a paged cache needs per-sequence lengths");
    if (quant)
      for (const torch::Tensor* sc : {kscale, vscale})
        TORCH_CHECK(sc->is_cuda() && sc->dtype() == torch::kFloat32 &&
                        sc->is_contiguous() &&
                        sc->numel() == kcache.size(0) * (long)TILE * Hkv,
                    "decode: scales must be contiguous fp32 [n_pages, 64, Hkv]");
    max_pages = block_table->size(1);
    n_pages = kcache.size(0);
    bt_ptr = block_table->data_ptr<int>();
  }
  const int T_alloc = block_table ? max_pages * TILE : (int)kcache.size(1);
  if (block_table) t = T_alloc;
  TORCH_CHECK((block_table || kcache.size(0) == B) && kcache.size(3) == HD);
  TORCH_CHECK(t >= 1 && t <= T_alloc, "decode: bad cache length");
  TORCH_CHECK(Hq % Hkv == 0 && (HD == 64 || HD == 128), "decode: unsupported shape");
  TORCH_CHECK(Hq / Hkv <= 8, "decode: GQA group > 8 not supported");
  TORCH_CHECK(q.is_contiguous());
  TORCH_CHECK(!t_dev || (t_dev->dtype() == torch::kInt32 && t_dev->is_cuda() &&
                         t_dev->is_contiguous() &&
                         t_dev->numel() >= (t_stride ? B : 1)),
              "decode: device lengths must be int32, one per sequence");
  TORCH_CHECK(max_len < 0 || (max_len >= 1 && max_len <= T_alloc),
              "decode: bad max_len");
  const int* t_ptr = t_dev ? t_dev->data_ptr<int>() : nullptr;

  // enough splits to fill the chip, but >= 2 tiles of work per split; in
  // graph mode (t_dev) size for the worst case T_alloc (or the caller's
  // bound max_len) so one capture covers every step. The kernel derives its
  // chunk from the length it reads, so nsplits only sizes the grid.
  long t_sz = t_dev ? (max_len > 0 ? max_len : T_alloc) : t;
  int nsplits = (int)std::min<long>((512 + B * Hkv - 1) / (B * Hkv),
                                    std::max<long>(1, (t_sz + 2 * TILE - 1) / (2 * TILE)));
  auto fopts = q.options().dtype(torch::kFloat32);
  auto partial_o = torch::empty({nsplits, B, Hq, HD}, fopts);
  auto partial_ml = torch::empty({nsplits, B, Hq, 2}, fopts);
  auto out = torch::empty_like(q);
  float scale = 1.0f / sqrtf((float)HD);
  hipStream_t stream = hypha_stream();

  const float* ksp = kscale ? kscale->data_ptr<float>() : nullptr;
  const float* vsp = vscale ? vscale->data_ptr<float>() : nullptr;

#define DECODE_DISPATCH(HDV, QV)                                                       \
  do {                                                                                 \
    if (block_table)                                                                   \
      DECODE_LAUNCH(HDV, QV, true);                                                    \
    else                                                                               \
      DECODE_LAUNCH(HDV, QV, false);                                                   \
  } while (0)
#define DECODE_LAUNCH(HDV, QV, PV)                                                     \
  do {                                                                                 \
    hipLaunchKernelGGL((attn_decode_kernel<HDV, QV, PV>), dim3(nsplits, B* Hkv),       \
                       dim3(256), 0, stream, (const short*)q.data_ptr(),               \
                       (const short*)kcache.data_ptr(),                                \
                       (const short*)vcache.data_ptr(), ksp, vsp,                      \
                       partial_o.data_ptr<float>(),                                    \
                       partial_ml.data_ptr<float>(), B, Hq, Hkv, T_alloc, (int)t,      \
                       t_ptr, t_stride, nsplits, scale, bt_ptr, max_pages, n_pages);   \
    hipLaunchKernelGGL(attn_decode_reduce_kernel<HDV>, dim3(B* Hq), dim3(128), 0,      \
                       stream, partial_o.data_ptr<float>(),                            \
                       partial_ml.data_ptr<float>(), (short*)out.data_ptr(), B, Hq,    \
                       nsplits);                                                       \
  } while (0)

  if (HD == 128 && !quant)
    DECODE_DISPATCH(128, false);
  else if (HD == 128)
    DECODE_DISPATCH(128, true);
  else if (!quant)
    DECODE_DISPATCH(64, false);
  else
    DECODE_DISPATCH(64, true);
#undef DECODE_DISPATCH
#undef DECODE_LAUNCH
  return out;
}

torch::Tensor attn_decode(torch::Tensor q, torch::Tensor kcache, torch::Tensor vcache,
                          long t) {
  return attn_decode_impl(q, kcache, vcache, t, nullptr);
}

// hipGraph-capturable decode: valid length read from t_dev (int32 [1]) at
// kernel time; splits sized for T_alloc once.
torch::Tensor attn_decode_graph(torch::Tensor q, torch::Tensor kcache,
                                torch::Tensor vcache, torch::Tensor t_dev) {
  TORCH_CHECK(t_dev.dtype() == torch::kInt32 && t_dev.is_cuda());
  return attn_decode_impl(q, kcache, vcache, kcache.size(1), &t_dev);
}

// fp8 (OCP e4m3) KV cache variants: per-row fp32 scales [B, T_alloc, Hkv].
torch::Tensor attn_decode_fp8(torch::Tensor q, torch::Tensor kcache,
                              torch::Tensor vcache, torch::Tensor kscale,
                              torch::Tensor vscale, long t) {
  return attn_decode_impl(q, kcache, vcache, t, nullptr, &kscale, &vscale);
}

torch::Tensor attn_decode_fp8_graph(torch::Tensor q, torch::Tensor kcache,
                                    torch::Tensor vcache, torch::Tensor kscale,
                                    torch::Tensor vscale, torch::Tensor t_dev) {
  TORCH_CHECK(t_dev.dtype() == torch::kInt32 && t_dev.is_cuda());
  return attn_decode_impl(q, kcache, vcache, kcache.size(1), &t_dev, &kscale,
                          &vscale);
}

// Per-sequence lengths: lens int32 [B] on the device, lens[b] = valid rows
// of sequence b INCLUDING the current token, read at kernel time (graph-
// capturable as is). lens[b] == 0 returns exact zeros for that sequence and
// reads none of its cache. max_len (host, <= 0: T_alloc) only sizes nsplits.
torch::Tensor attn_decode_varlen(torch::Tensor q, torch::Tensor kcache,
                                 torch::Tensor vcache, torch::Tensor lens,
                                 long max_len) {
  TORCH_CHECK(lens.dim() == 1 && lens.size(0) == q.size(0), "decode: lens must be [B]");
  return attn_decode_impl(q, kcache, vcache, kcache.size(1), &lens, nullptr, nullptr,
                          1, max_len > 0 ? max_len : -1);
}

torch::Tensor attn_decode_varlen_fp8(torch::Tensor q, torch::Tensor kcache,
                                     torch::Tensor vcache, torch::Tensor kscale,
                                     torch::Tensor vscale, torch::Tensor lens,
                                     long max_len) {
  TORCH_CHECK(lens.dim() == 1 && lens.size(0) == q.size(0), "decode: lens must be [B]");
  return attn_decode_impl(q, kcache, vcache, kcache.size(1), &lens, &kscale, &vscale,
                          1, max_len > 0 ? max_len : -1);
}

// Paged cache: kpool/vpool [n_pages, 64, Hkv, D] (bf16, or fp8 with scales
// [n_pages, 64, Hkv]); block_table int32 [B, max_pages] on the device maps
// logical row j of sequence b to row j % 64 of page block_table[b, j / 64].
// lens as in attn_decode_varlen, clamped to [0, max_pages * 64]; table slots
// at or past ceil(lens[b] / 64) are never read. For the same logical cache
// and the same max_len the output equals attn_decode_varlen's bit for bit.
torch::Tensor attn_decode_paged(torch::Tensor q, torch::Tensor kpool, torch::Tensor vpool,
                                std::optional<torch::Tensor> kscale,
                                std::optional<torch::Tensor> vscale,
                                torch::Tensor block_table, torch::Tensor lens,
                                long max_len) {
  TORCH_CHECK(lens.dim() == 1 && lens.size(0) == q.size(0), "decode: lens must be [B]");
  TORCH_CHECK(kscale.has_value() == vscale.has_value(), "decode: give both scales or none");
  return attn_decode_impl(q, kpool, vpool, 0, &lens, kscale ? &*kscale : nullptr,
                          vscale ? &*vscale : nullptr, 1, max_len > 0 ? max_len : -1,
                          &block_table);
}

namespace {

// One row of HD bf16 values -> e4m3 bytes + one fp32 scale, by one wave
// (lane l of 64): the bytes and the scale KVCache._quantize_rows writes for
// this row on the GPU, bit for bit, so that a row appended here and one
// appended through the PyTorch path are the same row: there the scale is amax
// times the fp32 reciprocal of 448 (how a tensor is divided by a host scalar),
// and each element is DIVIDED by the scale. (x * (1 / scale) rounds twice and
// lands on another e4m3 byte in about 2% of bf16 rows.)
template <int HD>
__device__ __forceinline__ void quantize_row_e4m3(const short* __restrict__ src,
                                                  unsigned char* __restrict__ dst8,
                                                  float* __restrict__ dsts,
                                                  long long row, int l) {
  float vals[HD / 64];
  float mx = 0.f;
#pragma unroll
  for (int i = 0; i < HD / 64; ++i) {
    vals[i] = bf2f(src[l + 64 * i]);
    mx = fmaxf(mx, fabsf(vals[i]));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  const float scale = fmaxf(mx, 1e-8f) * (1.0f / 448.0f);
  if (l == 0) dsts[row] = scale;
#pragma unroll
  for (int i = 0; i < HD / 64; ++i) {
    float a = fminf(fmaxf(vals[i] / scale, -448.f), 448.f);
    dst8[row * HD + l + 64 * i] =
        (unsigned char)(__builtin_amdgcn_cvt_pk_fp8_f32(a, a, 0, false) & 0xff);
  }
}

// Fused single-token fp8 KV append: one launch quantizes the new k AND v
// rows (per-row amax -> scale -> e4m3) and writes bytes + scales at the
// device position index — replaces an ~8-launch python chain per layer
// per token inside the captured decode graph.
template <int HD>
__global__ __launch_bounds__(64) void kv_append_fp8_kernel(
    const short* __restrict__ kin, const short* __restrict__ vin,
    unsigned char* __restrict__ k8, unsigned char* __restrict__ v8,
    float* __restrict__ kscale, float* __restrict__ vscale,
    const long long* __restrict__ pos, int pos_stride, int B, int Hkv, int T_alloc) {
  const int bh = blockIdx.x;       // (b * Hkv + h)
  const int which = blockIdx.y;    // 0 = k, 1 = v
  const int l = threadIdx.x;
  const short* src = (which ? vin : kin) + (long long)bh * HD;
  unsigned char* dst8 = which ? v8 : k8;
  float* dsts = which ? vscale : kscale;
  const int b = bh / Hkv, h = bh % Hkv;
  // pos_stride 0: one position for the batch; 1: one per sequence. A
  // position outside the cache writes nothing (uniform over the block): the
  // parking position of a finished sequence.
  const long long p = pos[b * pos_stride];
  if (p < 0 || p >= T_alloc) return;
  const long long row = ((long long)b * T_alloc + p) * Hkv + h;
  quantize_row_e4m3<HD>(src, dst8, dsts, row, l);
}

// Paged append: pool row of logical position p of sequence b, or -1 when the
// row is not to be written: p outside [0, max_pages * TILE) (a parked
// sequence), p at or past lens[b] (a pad row of a right-padded chunk), or a
// page id outside [0, n_pages). A clamped write would land in another
// sequence's page, so an out-of-range id writes nothing. Uniform over the
// workgroup.
__device__ __forceinline__ long long paged_dst_row(const int* __restrict__ block_table,
                                                   const int* __restrict__ lens, int b,
                                                   long long p, int max_pages,
                                                   int n_pages) {
  if (p < 0 || p >= (long long)max_pages * TILE) return -1;
  if (lens && p >= (long long)lens[b]) return -1;
  const int page = block_table[(long long)b * max_pages + (int)(p / TILE)];
  if (page < 0 || page >= n_pages) return -1;
  return (long long)page * TILE + (int)(p % TILE);
}

// k/v [B, s, Hkv, D] bf16 -> fp8 pool: one wave per (b, i, h) row; quantized
// by the device code of kv_append_fp8_kernel. blockIdx.y: 0 = k, 1 = v.
template <int HD>
__global__ __launch_bounds__(64) void kv_append_paged_fp8_kernel(
    const short* __restrict__ kin, const short* __restrict__ vin,
    unsigned char* __restrict__ k8, unsigned char* __restrict__ v8,
    float* __restrict__ kscale, float* __restrict__ vscale,
    const int* __restrict__ block_table, const long long* __restrict__ pos,
    int pos_stride, const int* __restrict__ lens, int s, int Hkv, int max_pages,
    int n_pages) {
  const long long rh = blockIdx.x;  // (b * s + i) * Hkv + h
  const int h = (int)(rh % Hkv);
  const long long bi = rh / Hkv;
  const int b = (int)(bi / s), i = (int)(bi % s);
  const long long prow = paged_dst_row(block_table, lens, b, pos[b * pos_stride] + i,
                                       max_pages, n_pages);
  if (prow < 0) return;
  const int which = blockIdx.y;
  quantize_row_e4m3<HD>((which ? vin : kin) + rh * HD, which ? v8 : k8,
                        which ? vscale : kscale, prow * Hkv + h, threadIdx.x);
}

// k/v [B, s, Hkv, D] bf16 -> bf16 pool: row (b, i) (Hkv * HD contiguous
// elements) is copied as 16-byte vectors. blockIdx.y: 0 = k, 1 = v.
__global__ __launch_bounds__(256) void kv_append_paged_bf16_kernel(
    const short* __restrict__ kin, const short* __restrict__ vin,
    short* __restrict__ kc, short* __restrict__ vc, const int* __restrict__ block_table,
    const long long* __restrict__ pos, int pos_stride, const int* __restrict__ lens,
    int s, int row_elems, int max_pages, int n_pages) {
  const long long bi = blockIdx.x;  // b * s + i
  const int b = (int)(bi / s), i = (int)(bi % s);
  const long long prow = paged_dst_row(block_table, lens, b, pos[b * pos_stride] + i,
                                       max_pages, n_pages);
  if (prow < 0) return;
  const short* src = (blockIdx.y ? vin : kin) + bi * row_elems;
  short* dst = (blockIdx.y ? vc : kc) + prow * row_elems;
  for (int c = threadIdx.x * 8; c < row_elems; c += 256 * 8)
    *reinterpret_cast<s16x8*>(dst + c) = *reinterpret_cast<const s16x8*>(src + c);
}

// bf16 cache: the row of sequence b (Hkv * HD contiguous elements in bshd)
// is copied as 16-byte vectors to cache row pos[b]; blockIdx.y: 0 = k, 1 = v.
__global__ __launch_bounds__(256) void kv_append_rows_bf16_kernel(
    const short* __restrict__ kin, const short* __restrict__ vin,
    short* __restrict__ kc, short* __restrict__ vc,
    const long long* __restrict__ pos, int row_elems, int T_alloc) {
  const int b = blockIdx.x;
  const long long p = pos[b];
  if (p < 0 || p >= T_alloc) return;  // parked sequence: nothing written
  const short* src = (blockIdx.y ? vin : kin) + (long long)b * row_elems;
  short* dst = (blockIdx.y ? vc : kc) + ((long long)b * T_alloc + p) * row_elems;
  for (int c = threadIdx.x * 8; c < row_elems; c += 256 * 8)
    *reinterpret_cast<s16x8*>(dst + c) = *reinterpret_cast<const s16x8*>(src + c);
}

void kv_append_fp8_launch(torch::Tensor k, torch::Tensor v, torch::Tensor k8,
                          torch::Tensor v8, torch::Tensor kscale, torch::Tensor vscale,
                          torch::Tensor pos, int pos_stride) {
  const int B = k8.size(0), T_alloc = k8.size(1), Hkv = k8.size(2), HD = k8.size(3);
  TORCH_CHECK(k.is_cuda() && v.is_cuda() && k.dtype() == torch::kBFloat16 &&
              v.dtype() == torch::kBFloat16);
  TORCH_CHECK(k.numel() == (long long)B * Hkv * HD && k.is_contiguous());
  TORCH_CHECK(v.numel() == k.numel() && v.is_contiguous());
  TORCH_CHECK(pos.dtype() == torch::kInt64 && pos.is_cuda() && pos.is_contiguous() &&
              pos.numel() >= (pos_stride ? B : 1));
  TORCH_CHECK(HD == 64 || HD == 128);
  TORCH_CHECK(k8.dtype() == torch::kFloat8_e4m3fn && k8.is_contiguous() &&
              v8.is_contiguous() && v8.sizes() == k8.sizes() && v8.dtype() == k8.dtype());
  for (const torch::Tensor* sc : {&kscale, &vscale})
    TORCH_CHECK(sc->is_cuda() && sc->dtype() == torch::kFloat32 && sc->is_contiguous() &&
                sc->numel() == (long long)B * T_alloc * Hkv);
  hipStream_t stream = hypha_stream();
  if (HD == 128)
    hipLaunchKernelGGL(kv_append_fp8_kernel<128>, dim3(B * Hkv, 2), dim3(64), 0,
                       stream, (const short*)k.data_ptr(), (const short*)v.data_ptr(),
                       (unsigned char*)k8.data_ptr(), (unsigned char*)v8.data_ptr(),
                       kscale.data_ptr<float>(), vscale.data_ptr<float>(),
                       (const long long*)pos.data_ptr<int64_t>(), pos_stride, B, Hkv,
                       T_alloc);
  else
    hipLaunchKernelGGL(kv_append_fp8_kernel<64>, dim3(B * Hkv, 2), dim3(64), 0,
                       stream, (const short*)k.data_ptr(), (const short*)v.data_ptr(),
                       (unsigned char*)k8.data_ptr(), (unsigned char*)v8.data_ptr(),
                       kscale.data_ptr<float>(), vscale.data_ptr<float>(),
                       (const long long*)pos.data_ptr<int64_t>(), pos_stride, B, Hkv,
                       T_alloc);
}

}  // namespace

// k/v [B, 1, Hkv, D] bf16; caches fp8 [B, T_alloc, Hkv, D]; scales
// [B, T_alloc, Hkv] fp32; pos int64 [1] device tensor (graph-capturable).
void kv_append_fp8_(torch::Tensor k, torch::Tensor v, torch::Tensor k8,
                    torch::Tensor v8, torch::Tensor kscale, torch::Tensor vscale,
                    torch::Tensor pos) {
  kv_append_fp8_launch(k, v, k8, v8, kscale, vscale, pos, 0);
}

// Per-sequence single-row append: k/v [B, 1, Hkv, D] bf16 go to cache row
// pos[b] of sequence b (pos int64 [B] on the device; graph-capturable). bf16
// cache: vector copy; fp8 cache (kscale/vscale given): quantized exactly as
// kv_append_fp8_ does. pos[b] outside [0, T_alloc) writes nothing for b.
void kv_append_rows_(torch::Tensor k, torch::Tensor v, torch::Tensor kcache,
                     torch::Tensor vcache, std::optional<torch::Tensor> kscale,
                     std::optional<torch::Tensor> vscale, torch::Tensor pos) {
  TORCH_CHECK(kcache.dim() == 4 && kcache.is_cuda(), "append_rows: cache [B, T_alloc, Hkv, D]");
  const long B = kcache.size(0), T_alloc = kcache.size(1), Hkv = kcache.size(2),
             HD = kcache.size(3);
  TORCH_CHECK(pos.dim() == 1 && pos.size(0) == B, "append_rows: pos must be int64 [B]");
  if (kcache.dtype() == torch::kFloat8_e4m3fn) {
    TORCH_CHECK(kscale.has_value() && vscale.has_value(),
                "append_rows: fp8 cache needs row scales");
    kv_append_fp8_launch(k, v, kcache, vcache, *kscale, *vscale, pos, 1);
    return;
  }
  TORCH_CHECK(kcache.dtype() == torch::kBFloat16 && kcache.is_contiguous() &&
                  vcache.is_cuda() && vcache.is_contiguous() &&
                  vcache.sizes() == kcache.sizes() && vcache.dtype() == kcache.dtype(),
              "append_rows: caches must be contiguous bf16 of one shape");
  TORCH_CHECK(k.is_cuda() && v.is_cuda() && k.dtype() == torch::kBFloat16 &&
                  v.dtype() == torch::kBFloat16 && k.is_contiguous() && v.is_contiguous() &&
                  k.numel() == B * Hkv * HD && v.numel() == k.numel(),
              "append_rows: k/v must be contiguous bf16 [B, 1, Hkv, D]");
  TORCH_CHECK(pos.dtype() == torch::kInt64 && pos.is_cuda() && pos.is_contiguous());
  TORCH_CHECK(HD % 8 == 0 && Hkv * HD < (1L << 31) && B <= 65535 * 32768L,
              "append_rows: unsupported shape");
  hipLaunchKernelGGL(kv_append_rows_bf16_kernel, dim3((unsigned)B, 2), dim3(256), 0,
                     hypha_stream(), (const short*)k.data_ptr(), (const short*)v.data_ptr(),
                     (short*)kcache.data_ptr(), (short*)vcache.data_ptr(),
                     (const long long*)pos.data_ptr<int64_t>(), (int)(Hkv * HD),
                     (int)T_alloc);
}

// Paged append: row i of k/v [B, s, Hkv, D] bf16 goes to logical position
// p = pos[b * pos_stride] + i of sequence b, i.e. row p % 64 of page
// block_table[b, p / 64] of the pools [n_pages, 64, Hkv, D]. pos int64 on the
// device, 1 entry (the whole batch at one position) or B entries; lens
// (optional int32 [B]): rows with p >= lens[b] are not written. A position
// outside [0, max_pages * 64) or a page id outside [0, n_pages) writes
// nothing. bf16 pool: vector copy; fp8 pool: quantized as kv_append_fp8_ does.
void kv_append_paged_(torch::Tensor k, torch::Tensor v, torch::Tensor kpool,
                      torch::Tensor vpool, std::optional<torch::Tensor> kscale,
                      std::optional<torch::Tensor> vscale, torch::Tensor block_table,
                      torch::Tensor pos, std::optional<torch::Tensor> lens) {
  TORCH_CHECK(k.is_cuda() && v.is_cuda() && k.dim() == 4 && k.dtype() == torch::kBFloat16 &&
                  v.dtype() == torch::kBFloat16 && k.is_contiguous() && v.is_contiguous() &&
                  v.sizes() == k.sizes(),
              "append_paged: k/v must be contiguous bf16 [B, s, Hkv, D]");
  const long B = k.size(0), s = k.size(1), Hkv = k.size(2), HD = k.size(3);
  TORCH_CHECK(kpool.is_cuda() && vpool.is_cuda() && kpool.dim() == 4 &&
                  kpool.is_contiguous() && vpool.is_contiguous() &&
                  vpool.sizes() == kpool.sizes() && vpool.dtype() == kpool.dtype() &&
                  kpool.size(0) >= 1 && kpool.size(1) == TILE && kpool.size(2) == Hkv &&
                  kpool.size(3) == HD,
              "append_paged: pools must be contiguous [n_pages, 64, Hkv, D] of one dtype");
  const long n_pages = kpool.size(0);
  TORCH_CHECK(block_table.is_cuda() && block_table.dtype() == torch::kInt32 &&
                  block_table.is_contiguous() && block_table.dim() == 2 &&
                  block_table.size(0) == B && block_table.size(1) >= 1,
              "append_paged: block_table must be contiguous int32 [B, max_pages]");
  const long max_pages = block_table.size(1);
  TORCH_CHECK(pos.is_cuda() && pos.dtype() == torch::kInt64 && pos.is_contiguous() &&
                  pos.dim() == 1 && (pos.size(0) == 1 || pos.size(0) == B),
              "append_paged: pos must be int64 [1] or [B] on the GPU");
  const int pos_stride = pos.size(0) == B && B > 1 ? 1 : 0;
  const int* lens_p = nullptr;
  if (lens.has_value()) {
    TORCH_CHECK(lens->is_cuda() && lens->dtype() == torch::kInt32 && lens->is_contiguous() &&
                    lens->dim() == 1 && lens->size(0) == B,
                "append_paged: lens must be contiguous int32 [B] on the GPU");
    lens_p = lens->data_ptr<int>();
  }
  TORCH_CHECK(s >= 1 && B >= 1 && B * s * Hkv < (1L << 31) && max_pages <= (1L << 24) &&
                  n_pages <= (1L << 24) && HD % 8 == 0 && Hkv * HD < (1L << 31),
              "append_paged: unsupported shape");
  const int* bt = block_table.data_ptr<int>();
  const long long* pp = (const long long*)pos.data_ptr<int64_t>();
  hipStream_t stream = hypha_stream();
  if (kpool.dtype() == torch::kFloat8_e4m3fn) {
    TORCH_CHECK(kscale.has_value() && vscale.has_value(),
                "append_paged: fp8 pool needs row scales");
    for (const torch::Tensor* sc : {&*kscale, &*vscale})
      TORCH_CHECK(sc->is_cuda() && sc->dtype() == torch::kFloat32 && sc->is_contiguous() &&
                      sc->numel() == n_pages * TILE * Hkv,
                  "append_paged: scales must be contiguous fp32 [n_pages, 64, Hkv]");
    TORCH_CHECK(HD == 64 || HD == 128, "append_paged: fp8 head dim must be 64 or 128");
#define APPEND_PAGED_FP8(HDV)                                                            \
  hipLaunchKernelGGL(kv_append_paged_fp8_kernel<HDV>, dim3((unsigned)(B * s * Hkv), 2),  \
                     dim3(64), 0, stream, (const short*)k.data_ptr(),                    \
                     (const short*)v.data_ptr(), (unsigned char*)kpool.data_ptr(),       \
                     (unsigned char*)vpool.data_ptr(), kscale->data_ptr<float>(),        \
                     vscale->data_ptr<float>(), bt, pp, pos_stride, lens_p, (int)s,      \
                     (int)Hkv, (int)max_pages, (int)n_pages)
    if (HD == 128)
      APPEND_PAGED_FP8(128);
    else
      APPEND_PAGED_FP8(64);
#undef APPEND_PAGED_FP8
    return;
  }
  TORCH_CHECK(kpool.dtype() == torch::kBFloat16, "append_paged: pool must be bf16 or fp8");
  hipLaunchKernelGGL(kv_append_paged_bf16_kernel, dim3((unsigned)(B * s), 2), dim3(256), 0,
                     stream, (const short*)k.data_ptr(), (const short*)v.data_ptr(),
                     (short*)kpool.data_ptr(), (short*)vpool.data_ptr(), bt, pp, pos_stride,
                     lens_p, (int)s, (int)(Hkv * HD), (int)max_pages, (int)n_pages);
}
