// Common helpers for hypha_amd CDNA4 (gfx950) HIP kernels.
// Wave size is 64 on CDNA4; all block sizes are multiples of 64.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#define HYPHA_WAVE 64

#define HIP_CHECK(expr)                                                        \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      TORCH_CHECK(false, "HIP error: ", hipGetErrorString(_e), " at ",        \
                  __FILE__, ":", __LINE__);                                    \
    }                                                                          \
  } while (0)

using bf16 = __hip_bfloat16;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;

__device__ __forceinline__ float bf2f(short u) {
  union {
    float f;
    unsigned int i;
  } c;
  c.i = ((unsigned int)(unsigned short)u) << 16;
  return c.f;
}

__device__ __forceinline__ short f2bf(float f) {
  union {
    float f;
    unsigned int i;
  } c;
  c.f = f;
  unsigned int x = c.i;
  // round-to-nearest-even, NaN-safe
  if ((x & 0x7fffffffu) > 0x7f800000u) return (short)0x7fc0;  // NaN
  unsigned int round = 0x7fffu + ((x >> 16) & 1u);
  return (short)((x + round) >> 16);
}

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

// four e4m3 codes -> four bf16 (two dwords), exactly: v_cvt_pk_f32_fp8 gives
// two exact fp32, one v_perm_b32 keeps their high halves
__device__ __forceinline__ u32x2 e4m3x4_to_bf16x4(unsigned int d) {
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)d, false);
  const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)d, true);
  u32x2 o;
  o[0] = __builtin_amdgcn_perm(__float_as_uint(a[1]), __float_as_uint(a[0]), 0x07060302u);
  o[1] = __builtin_amdgcn_perm(__float_as_uint(b[1]), __float_as_uint(b[0]), 0x07060302u);
  return o;
}

// eight e4m3 codes -> one bf16 MFMA operand
__device__ __forceinline__ s16x8 e4m3x8_to_bf16x8(unsigned int d0, unsigned int d1) {
  const u32x2 lo = e4m3x4_to_bf16x4(d0), hi = e4m3x4_to_bf16x4(d1);
  const u32x4 v = {lo[0], lo[1], hi[0], hi[1]};
  return __builtin_bit_cast(s16x8, v);
}

// eight e2m1 codes (one dword, k order = nibble order) times sc -> one bf16 MFMA operand
__device__ __forceinline__ s16x8 e2m1x8_to_bf16x8(unsigned int d, float sc) {
  u32x4 v;
  v[0] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 0));
  v[1] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 1));
  v[2] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 2));
  v[3] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 3));
  return __builtin_bit_cast(s16x8, v);
}

typedef __attribute__((ext_vector_type(8))) int i32x8;

// One v_mfma_scale_f32_32x32x64_f8f6f4. a: 32 e2m1 codes (cbsz 4), sa: their
// E8M0 scale in byte SEL; b: 32 e4m3 codes (blgp 0), sb: their scale in byte SEL
template <int SEL>
__device__ __forceinline__ f32x16 mfma_e2m1_e4m3(u32x4 a, i32x8 b, f32x16 acc, unsigned int sa,
                                                 unsigned int sb) {
  const i32x8 a8 = {(int)a[0], (int)a[1], (int)a[2], (int)a[3], 0, 0, 0, 0};
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b, acc, 4, 0, SEL, (int)sa, SEL,
                                                         (int)sb);
}

// Grid sizing for memory-bound grid-stride kernels: cap at ~8 blocks/CU.
inline int elementwise_grid(long long n_items, int block = 256) {
  long long blocks = (n_items + block - 1) / block;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

// Wave-level f32 reductions (64 lanes).
__device__ __forceinline__ float wave_reduce_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ float wave_reduce_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// torch current-stream helper (native HIP API, no CUDA masquerade)
#ifdef __HIP_PLATFORM_AMD__
#include <c10/hip/HIPStream.h>
inline hipStream_t hypha_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}
#endif
