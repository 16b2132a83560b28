// Tile geometry and LDS-image helpers shared by the MFMA flash-attention
// forward kernels (attention.hip attn_fwd_kernel, prefill.hip).
#pragma once

#include "hip_common.h"

constexpr int KVB = 64;   // kv tile (fwd)
constexpr int QB = 32;    // q rows per wave
constexpr int NWAVE = 4;  // waves per workgroup
constexpr int WGQ = QB * NWAVE;
constexpr int PADV = 8;   // V^T pitch pad (72 elems -> conflict-free b128)

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
