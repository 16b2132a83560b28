// Fused temperature / top-k / top-p token sampling: one bf16 logits row to one
// token id, and the Philox4x32-10 uniforms that drive it.
//
// sample_token computes, per row, exactly the function of ops/reference.py
// sample_token: tokens ranked by value descending, ties by index ascending,
// mass exp((z - z_max) / T) in fp32, top-k cut, top-p cut, inverse-CDF pick at u.
// Temperature, top_k, top_p and u are read from device memory at kernel
// time, so one captured graph serves every setting and every step.
//
// A bf16 logit is a 16-bit ordered key, so a row is fully described by one
// count per distinct key and everything after the histogram is independent
// of V. One 1024-thread workgroup per row:
//   build  stream the row (bf16x8 loads) into an int32 count table held in
//          LDS (integer atomics). 65536 counters do not fit, so the table
//          covers one HALF of the key space (32768 keys, 128 KiB): values
//          >= 0 first, values < 0 only when a stage needs them. The row is
//          re-streamed (from L2) for the other half.
//   scan   three stages walk the table in descending key order with
//          fixed-order block scans: (0) top-k cut and kept mass, (1) top-p
//          cut and kept mass, (2) the key that u selects and the rank r
//          inside that key's ties. Equal keys have equal mass, so mass is
//          count * exp(...) and no float atomics exist anywhere.
//   find   rescan the row for the r-th occurrence of that key in index order
//          (per-chunk match counts, a block scan, one wave resolves the chunk).
// Integer atomics plus fixed-order scans: bit-reproducible run to run.
//
// Rows need not be 16-byte aligned (V % 8 != 0): vectors are laid on the
// aligned grid of the row's address and the two edge vectors use guarded
// scalar loads; nothing outside [row, row + V) is read.

#include <torch/extension.h>

#include "hip_common.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kHalf = 32768;                  // keys per table
constexpr int kPerThread = kHalf / kThreads;  // 32 consecutive keys per thread

// bf16 bits -> key with unsigned order == value order. -0.0 joins +0.0; every
// NaN becomes key 0 (below -inf, mass 0), so a NaN can win only an all-NaN row.
__device__ __forceinline__ int ordered_key(short s) {
  unsigned b = (unsigned short)s;
  if ((b & 0x7fffu) > 0x7f80u) return 0;
  if (b == 0x8000u) b = 0;
  return (b & 0x8000u) ? (int)(~b & 0xffffu) : (int)(b | 0x8000u);
}

__device__ __forceinline__ float key_value(int key) {
  unsigned b = (key & 0x8000) ? (unsigned)(key & 0x7fff) : (~(unsigned)key & 0xffffu);
  return bf2f((short)b);
}

// table slot of descending position d (0 = largest key of the half). The
// swizzle spreads a thread's 32 consecutive positions over the banks.
__device__ __forceinline__ int slot(int d) { return d ^ ((d >> 5) & 31); }

struct Row {
  const short* p;  // row start
  int V;
  int shift;  // elements between the aligned grid and the row start, 0..7
  int nvec;   // vectors on the aligned grid that touch the row
};

// grid vector g lies wholly inside the row: one aligned 16-byte load
__device__ __forceinline__ bool interior(const Row& r, int g) {
  const int e0 = g * 8 - r.shift;
  return e0 >= 0 && e0 + 8 <= r.V;
}

__device__ __forceinline__ s16x8 load_vec(const Row& r, int g) {
  return *reinterpret_cast<const s16x8*>(r.p + (g * 8 - r.shift));
}

// keys of grid vector g, v its data if interior (else guarded scalar loads);
// -1 where the element lies outside the row
__device__ __forceinline__ void vec_keys(const Row& r, int g, s16x8 v, int (&key)[8]) {
  if (interior(r, g)) {
#pragma unroll
    for (int j = 0; j < 8; ++j) key[j] = ordered_key(v[j]);
  } else {
    const int e0 = g * 8 - r.shift;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int e = e0 + j;
      key[j] = (e >= 0 && e < r.V) ? ordered_key(r.p[e]) : -1;
    }
  }
}

// Exclusive block scan in thread order; fixed association, so the result is a
// pure function of the inputs. total = sum over the block.
template <typename T>
__device__ __forceinline__ T block_scan(T v, T* s_wave, T& total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    T o = __shfl_up(inc, off, 64);
    if (lane >= off) inc += o;
  }
  T exc = __shfl_up(inc, 1, 64);
  if (lane == 0) exc = 0;
  __syncthreads();
  if (lane == 63) s_wave[wid] = inc;
  __syncthreads();
  T base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    T x = s_wave[w];
    if (w < wid) base += x;
    total += x;
  }
  return base + exc;
}

// A single workgroup streams the row, so a pass is bound by load latency:
// kBatch independent 16-byte loads per thread are in flight at a time.
constexpr int kBatch = 8;

// Count the row's keys of one half into the LDS table; returns the thread's
// largest key.
__device__ __forceinline__ int build_half(const Row& r, int* hist, int half) {
  for (int i = threadIdx.x; i < kHalf; i += kThreads) hist[i] = 0;
  __syncthreads();
  const int top = half ? 0xffff : 0x7fff;
  int kmax = 0;
  for (int g0 = threadIdx.x; g0 < r.nvec; g0 += kThreads * kBatch) {
    s16x8 v[kBatch];
#pragma unroll
    for (int b = 0; b < kBatch; ++b) {
      const int g = g0 + b * kThreads;
      v[b] = s16x8{};
      if (g < r.nvec && interior(r, g)) v[b] = load_vec(r, g);
    }
#pragma unroll
    for (int b = 0; b < kBatch; ++b) {
      const int g = g0 + b * kThreads;
      if (g >= r.nvec) break;
      int key[8];
      vec_keys(r, g, v[b], key);
      int run_key = -1, run = 0;  // merge runs of equal keys into one atomic
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = key[j];
        kmax = max(kmax, k);
        const bool mine = k >= 0 && (k >> 15) == half;
        if (mine && k == run_key) {
          ++run;
        } else {
          if (run) atomicAdd(&hist[slot(top - run_key)], run);
          run_key = mine ? k : -1;
          run = mine ? 1 : 0;
        }
      }
      if (run) atomicAdd(&hist[slot(top - run_key)], run);
    }
  }
  __syncthreads();
  return kmax;
}

struct Params {
  float inv_temp;
  float vmax;
  int kmax;
};

// exp((z - z_max) / T) with the division as a multiplication by 1 / T
__device__ __forceinline__ float key_mass(int key, const Params& q) {
  if (key == q.kmax) return 1.f;
  const float val = key_value(key);
  if (!(val > -INFINITY)) return 0.f;  // -inf and the NaN key
  return __expf((val - q.vmax) * q.inv_temp);
}

__global__ void __launch_bounds__(kThreads)
sample_token_kernel(const short* __restrict__ logits, const float* __restrict__ u_in,
                    const float* __restrict__ temp_in, const int* __restrict__ topk_in,
                    const float* __restrict__ topp_in, long* __restrict__ out, int V) {
  __shared__ int hist[kHalf];
  __shared__ int s_wi[kWaves];
  __shared__ float s_wf[kWaves];
  __shared__ int s_pos;     // descending position found by a stage (min wins)
  __shared__ int s_cnt;     // tokens kept / rank inside the found key
  __shared__ float s_mass;  // kept mass up to and including the cut
  __shared__ int s_last;    // last descending position with kept mass

  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  Row r;
  r.p = logits + (long long)row * V;
  r.V = V;
  r.shift = (int)((reinterpret_cast<uintptr_t>(r.p) & 15) >> 1);
  r.nvec = (V + r.shift + 7) / 8;

  float temp = temp_in[0];
  int k_eff = topk_in[0];
  float top_p = topp_in[0];
  float u = u_in[row];
  if (k_eff <= 0 || k_eff > V) k_eff = V;
  if (!(temp > 0.f)) {  // outside the contract: act greedy
    temp = 1.f;
    k_eff = 1;
  }
  if (!(top_p < 1.f)) top_p = 1.f;
  if (!(u >= 0.f)) u = 0.f;
  if (u >= 1.f) u = 0.99999994f;
  if (tid == 0) out[row] = 0;  // overwritten by the token found below

  // ---- first build (values >= 0) + row maximum --------------------------
  int cached = 1;
  int kmax = build_half(r, hist, 1);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) kmax = max(kmax, __shfl_xor(kmax, off, 64));
  if (lane == 0) s_wi[wid] = kmax;
  __syncthreads();
  kmax = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) kmax = max(kmax, s_wi[w]);
  Params q;
  q.inv_temp = 1.f / temp;
  q.kmax = kmax;
  q.vmax = key_value(kmax);

  // cut: keys above cut_key are kept whole, cut_key keeps cut_cnt tokens,
  // keys below keep none
  int cut_key = -1, cut_cnt = 0;
  float z_kept = 0.f;
  int sel_key = kmax, sel_rank = 0;  // the first ranked token: always kept

  for (int stage = 0; stage < 3; ++stage) {
    if (stage == 1 && top_p >= 1.f) continue;
    const float thresh = stage == 1 ? top_p * z_kept : u * z_kept;
    int base_cnt = 0;
    float base_mass = 0.f;
    bool done = false;
    __syncthreads();
    if (tid == 0) s_last = -1;
    for (int half = 1; half >= 0 && !done; --half) {
      if (half == 1 && kmax < 0x8000) continue;  // no value >= 0 in the row
      if (cached != half) {
        build_half(r, hist, half);
        cached = half;
      }
      const int top = half ? 0xffff : 0x7fff;
      const int d0 = tid * kPerThread;
      if (tid == 0) s_pos = 0x7fffffff;

      // stage 0: tokens ranked before this thread's keys
      int cnt_before = 0, tc = 0;
      if (stage == 0) {
#pragma unroll 8
        for (int i = 0; i < kPerThread; ++i) tc += hist[slot(d0 + i)];
        int tot;
        cnt_before = base_cnt + block_scan<int>(tc, s_wi, tot);
        base_cnt += tot;
      }
      // kept tokens of the key at position d0 + i
      auto kept = [&](int i, int c, int before) {
        const int key = top - (d0 + i);
        if (stage == 0) return min(max(k_eff - before, 0), c);
        return key > cut_key ? c : (key == cut_key ? min(c, cut_cnt) : 0);
      };
      // can this thread's 32 keys hold a kept token at all
      const bool any_kept = stage == 0 ? (tc > 0 && cnt_before < k_eff)
                                       : (top - d0 >= cut_key);
      float tsum = 0.f;
      if (any_kept) {
        int before = cnt_before, last = -1;
#pragma unroll 4
        for (int i = 0; i < kPerThread; ++i) {
          const int c = hist[slot(d0 + i)];
          const int e = kept(i, c, before);
          before += c;
          if (e) {
            const float m = key_mass(top - (d0 + i), q);
            tsum += (float)e * m;
            if (m > 0.f) last = d0 + i;
          }
        }
        if (stage == 2 && last >= 0) atomicMax(&s_last, last + (half ? 0 : kHalf));
      }
      float ftot;
      const float mass_before = base_mass + block_scan<float>(tsum, s_wf, ftot);
      // (block_scan's barriers also publish s_pos = INT_MAX)

      // Only a thread whose keys reach the threshold searches them: the same
      // sums again in the same order, now as a running prefix.
      bool search;
      if (stage == 0) search = tc > 0 && cnt_before < k_eff && cnt_before + tc >= k_eff;
      else if (stage == 1) search = any_kept && mass_before + tsum >= thresh;
      else search = any_kept && mass_before + tsum > thresh;
      int my_pos = 0x7fffffff, my_n = 0;
      float my_mass = 0.f;
      if (search) {
        int before = cnt_before;
        float run = 0.f;
        for (int i = 0; i < kPerThread; ++i) {
          const int c = hist[slot(d0 + i)];
          const int e = kept(i, c, before);
          const float m = e ? key_mass(top - (d0 + i), q) : 0.f;
          const float sb = mass_before + run;
          if (e) run += (float)e * m;
          const float si = mass_before + run;
          bool hit;
          if (stage == 0) hit = c > 0 && before < k_eff && before + c >= k_eff;
          else if (stage == 1) hit = e > 0 && si >= thresh;
          else hit = e > 0 && si > thresh;
          if (hit) {
            my_pos = d0 + i;
            if (stage == 0) {
              my_n = e;
            } else if (stage == 1) {  // fewest tokens of this key reaching thresh
              const float need = (thresh - sb) / m;
              my_n = need >= 1.f ? (need < (float)e ? (int)ceilf(need) : e) : 1;
            } else {  // rank of the first token whose inclusive sum exceeds thresh
              const float need = (thresh - sb) / m;
              my_n = need >= 0.f ? (need < (float)(e - 1) ? (int)floorf(need) : e - 1) : 0;
            }
            my_mass = sb + (float)my_n * m;
            break;
          }
          before += c;
        }
        if (my_pos != 0x7fffffff) atomicMin(&s_pos, my_pos);
      }
      __syncthreads();
      const int pos = s_pos;
      if (pos == my_pos && pos != 0x7fffffff) {
        s_cnt = my_n;
        s_mass = my_mass;
      }
      __syncthreads();
      if (pos != 0x7fffffff) {
        const int key = top - pos;
        if (stage == 2) {
          sel_key = key;
          sel_rank = s_cnt;
        } else {
          cut_key = key;
          cut_cnt = s_cnt;
          z_kept = s_mass;
        }
        done = true;
      } else {
        base_mass += ftot;
      }
      // nothing is kept below the cut: the other half cannot matter
      if (!done && stage > 0 && cut_key >= 0x8000) break;
      __syncthreads();
    }
    if (!done) {
      if (stage == 2) {  // rounding left no hit: last kept token with mass
        __syncthreads();
        const int last = s_last;
        if (last >= 0) {
          // s_last orders positions across halves: upper half first
          sel_key = last < kHalf ? 0xffff - last : 0x7fff - (last - kHalf);
          sel_rank = -1;  // resolved below: last kept token of that key
        }
      } else if (stage == 0) {
        z_kept = base_mass;  // cannot happen (counts sum to V >= k_eff)
      }
      // stage 1 without a hit keeps the top-k cut
    }
  }

  // ---- find the sel_rank-th token with key sel_key, in index order -------
  // A chunk is 64 consecutive vectors (one per lane). Pass 1 counts the
  // matches of every chunk into the (now free) table; a block scan over the
  // chunk counts names the chunk that holds the rank; one wave resolves it.
  __syncthreads();
  int* chunk_cnt = hist;
  const int nchunk = (r.nvec + 63) / 64;  // <= kHalf (host check on V)
  for (int c0 = wid; c0 < nchunk; c0 += kWaves * kBatch) {
    s16x8 v[kBatch];
#pragma unroll
    for (int b = 0; b < kBatch; ++b) {
      const int g = (c0 + b * kWaves) * 64 + lane;
      v[b] = s16x8{};
      if (g < r.nvec && interior(r, g)) v[b] = load_vec(r, g);
    }
#pragma unroll
    for (int b = 0; b < kBatch; ++b) {
      const int c = c0 + b * kWaves;
      if (c >= nchunk) break;  // wave-uniform
      const int g = c * 64 + lane;
      int n = 0;
      if (g < r.nvec) {
        int key[8];
        vec_keys(r, g, v[b], key);
#pragma unroll
        for (int j = 0; j < 8; ++j) n += key[j] == sel_key;
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
      if (lane == 0) chunk_cnt[c] = n;
    }
  }
  __syncthreads();
  const int per_thread = (nchunk + kThreads - 1) / kThreads;
  const int c_lo = min(nchunk, tid * per_thread), c_hi = min(nchunk, c_lo + per_thread);
  int mine = 0;
  for (int c = c_lo; c < c_hi; ++c) mine += chunk_cnt[c];
  int total;
  const int before_me = block_scan<int>(mine, s_wi, total);
  if (total <= 0) {  // cannot happen: sel_key was counted from this row
    if (tid == 0) out[row] = 0;
    return;
  }
  if (sel_rank < 0) {  // "last kept token of the key"
    int kept_n = total;
    if (sel_key == cut_key) kept_n = min(total, cut_cnt);
    sel_rank = kept_n - 1;
  }
  sel_rank = max(0, min(sel_rank, total - 1));
  if (sel_rank >= before_me && sel_rank < before_me + mine) {  // one thread
    int rem = sel_rank - before_me;
    int c = c_lo;
    while (c < c_hi - 1 && rem >= chunk_cnt[c]) rem -= chunk_cnt[c++];
    s_pos = c;
    s_cnt = rem;
  }
  __syncthreads();
  if (wid == 0) {
    const int c = s_pos, rem = s_cnt;
    const int g = c * 64 + lane;
    int key[8];
    int n = 0;
    if (g < r.nvec) {
      s16x8 v = s16x8{};
      if (interior(r, g)) v = load_vec(r, g);
      vec_keys(r, g, v, key);
#pragma unroll
      for (int j = 0; j < 8; ++j) n += key[j] == sel_key;
    }
    int inc = n;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      int o = __shfl_up(inc, off, 64);
      if (lane >= off) inc += o;
    }
    const int exc = inc - n;
    if (rem >= exc && rem < inc) {  // one lane
      int left = rem - exc;
      int found = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (key[j] == sel_key) {
          if (left == 0) found = g * 8 - r.shift + j;
          --left;
        }
      }
      out[row] = (found >= 0 && found < V) ? found : 0;
    }
  }
}

// ---- Philox4x32-10 ---------------------------------------------------------

__device__ __forceinline__ void philox_round(unsigned (&c)[4], unsigned k0, unsigned k1) {
  const unsigned long long p0 = 0xD2511F53ull * c[0];
  const unsigned long long p1 = 0xCD9E8D57ull * c[2];
  const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0;
  const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
  c[1] = (unsigned)p1;
  c[3] = (unsigned)p0;
  c[0] = n0;
  c[2] = n2;
}

__global__ void philox_uniform_kernel(const long* __restrict__ seed_in,
                                      const long* __restrict__ step_in,
                                      float* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long seed = (unsigned long long)seed_in[0];
  const unsigned long long step = (unsigned long long)step_in[0];
  unsigned c[4] = {(unsigned)i, (unsigned)step, (unsigned)(step >> 32), 0u};
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int rnd = 0; rnd < 10; ++rnd) {
    if (rnd) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    philox_round(c, k0, k1);
  }
  out[i] = (float)(c[0] >> 8) * 5.9604644775390625e-8f;  // 2**-24
}

}  // namespace

torch::Tensor sample_token(torch::Tensor logits, torch::Tensor u, torch::Tensor temperature,
                           torch::Tensor top_k, torch::Tensor top_p) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 &&
                  logits.dtype() == torch::kBFloat16 && logits.is_contiguous(),
              "sample_token: logits must be contiguous bf16 [B, V] on the GPU");
  const long long B = logits.size(0);
  TORCH_CHECK(logits.size(1) >= 1 && logits.size(1) <= (1ll << 24) - 16,
              "sample_token: V out of range");  // chunk counts fit the table
  const int V = (int)logits.size(1);
  TORCH_CHECK(u.is_cuda() && u.dtype() == torch::kFloat32 && u.is_contiguous() &&
                  u.numel() == B,
              "sample_token: u must be fp32 [B] on the GPU");
  TORCH_CHECK(temperature.is_cuda() && temperature.dtype() == torch::kFloat32 &&
                  temperature.numel() == 1 && top_p.is_cuda() &&
                  top_p.dtype() == torch::kFloat32 && top_p.numel() == 1 &&
                  top_k.is_cuda() && top_k.dtype() == torch::kInt32 &&
                  top_k.numel() == 1,
              "sample_token: temperature/top_p fp32[1], top_k int32[1] on the GPU");
  auto out = torch::empty({B, 1}, logits.options().dtype(torch::kInt64));
  if (B == 0) return out;
  hipLaunchKernelGGL(sample_token_kernel, dim3((unsigned)B), dim3(kThreads), 0,
                     hypha_stream(), (const short*)logits.data_ptr(),
                     u.data_ptr<float>(), temperature.data_ptr<float>(),
                     top_k.data_ptr<int>(), top_p.data_ptr<float>(),
                     out.data_ptr<long>(), V);
  return out;
}

torch::Tensor philox_uniform(torch::Tensor seed, torch::Tensor step, long n) {
  TORCH_CHECK(seed.is_cuda() && seed.dtype() == torch::kInt64 && seed.numel() == 1 &&
                  step.is_cuda() && step.dtype() == torch::kInt64 && step.numel() == 1,
              "philox_uniform: seed and step must be int64[1] on the GPU");
  TORCH_CHECK(n >= 0 && n < (1ll << 31), "philox_uniform: n out of range");
  auto out = torch::empty({n}, seed.options().dtype(torch::kFloat32));
  if (n == 0) return out;
  hipLaunchKernelGGL(philox_uniform_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256),
                     0, hypha_stream(), seed.data_ptr<long>(), step.data_ptr<long>(),
                     out.data_ptr<float>(), (int)n);
  return out;
}
