// What the MXFP8 and the MXFP4 quantise kernels share (mx_quantize.hip,
// mx4_quantize.hip): the block maximum on the bit patterns, the E8M0 scale
// byte from it and the store of a work-group's 64 scale bytes.
#pragma once
#include "cek_kernel.h"

typedef unsigned int u32;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float mxq_float(u32 u) { return __builtin_bit_cast(float, u); }

// |x| bits + 2^23 as a signed int: finite values stay positive and keep their
// order, inf is INT_MIN and NaN lies above it, so a signed max is the maximum
// over the finite values wherever there is one
__device__ __forceinline__ int mxq_key(u32 u) { return (int)((u & 0x7fffffffu) + 0x00800000u); }

// max over the LPB lanes of a block (LPB-aligned lane groups), in every lane
template <int LPB>
__device__ __forceinline__ int mxq_block_max(int m) {
  // quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror (lane i <-> 7 - i
  // of each 8, equal quads by then)
  m = max(m, __builtin_amdgcn_update_dpp(0, m, 0xB1, 0xF, 0xF, true));
  m = max(m, __builtin_amdgcn_update_dpp(0, m, 0x4E, 0xF, 0xF, true));
  if (LPB == 8) m = max(m, __builtin_amdgcn_update_dpp(0, m, 0x141, 0xF, 0xF, true));
  return m;
}

// scale byte e + 127 from a block's maximum key: e = max(E - 127 - EMAX, -127)
// with E the exponent field of the finite |x| maximum and EMAX the exponent of
// the element format's largest binade (e4m3: 8, e2m1: 2), e = 0 when that
// maximum is 0 or no element is finite
template <int EMAX>
__device__ __forceinline__ u32 mxq_scale_byte(int key) {
  const u32 amax = (u32)max(key, 0x00800000) - 0x00800000u;
  return amax == 0u ? 127u : (u32)max((int)(amax >> 23) - EMAX, 0);
}

// The group's 64 scale bytes as 16 dwords.  `mine` is, in every lane, the
// scale byte of the block this lane's group had in step (lane % LPB).  Dword
// j, byte b is block 4j + b: step (4j + b) / GPS, lane group (4j + b) % GPS,
// GPS = 64 / LPB groups per step.
template <int LPB>
__device__ __forceinline__ void mxq_store_scales(u32 mine, u32* scales32, long long group, int lane) {
  constexpr int GPS = 64 / LPB;
  const int j = lane & 15;
  u32 w = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int blk = 4 * j + b, src = (blk % GPS) * LPB + blk / GPS;
    w |= (u32)__builtin_amdgcn_ds_bpermute(src << 2, (int)mine) << (8 * b);
  }
  if (lane < 16) scales32[group * 16 + lane] = w;
}
