// What the MXFP8 and the MXFP4 quantise kernels (mx_quantize.hip,
// mx4_quantize.hip) and the quantising GEMM epilogue (gemm8_out.h) share: the
// block maximum on the bit patterns, the E8M0 scale byte from it, the two
// conversions with their NaN and saturation repairs, and the store of a
// work-group's 64 scale bytes.
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

// ---- e4m3fn (mx_quantize.hip has the measured behaviour of the conversion) ----

typedef u32 u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x2 __attribute__((ext_vector_type(2)));

// 0x80 in byte `k` for the key of a NaN, else 0
__device__ __forceinline__ u32 mxq_nan_bit(int key, int k) {
  return (u32)((int)(0x80000000u - (u32)key) >> 31) & (0x80u << (8 * k));
}

// The conversion's dword made the codec's.  Bytes whose low seven bits are all
// ones came from a NaN (`nan`: 0x80 in that byte) or from a value that rounded
// past 448: the latter become 0x7e under their sign, a NaN loses its sign.
__device__ __forceinline__ u32 mxq_fix(u32 w, u32 nan) {
  const u32 full = ((w & 0x7f7f7f7fu) + 0x01010101u) & 0x80808080u;
  return (w - ((full & ~nan) >> 7)) & ~nan;
}

// four values scaled by 2^-e (`scale` = 2^e) and rounded to e4m3fn
__device__ __forceinline__ u32 mxq_cvt4(float a, float b, float c, float d, float scale) {
  s16x2 r = {0, 0};
  r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(r, a, b, scale, false);
  r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(r, c, d, scale, true);
  return __builtin_bit_cast(u32, r);
}

// ---- e2m1 (mx4_quantize.hip) ----

// 0xF in nibble `k` for the key of a NaN, else 0
__device__ __forceinline__ u32 mx4q_nan_nibble(int key, int k) {
  return (u32)((int)(0x80000000u - (u32)key) >> 31) & (0xFu << (4 * k));
}

// OR over the four lanes of a block (aligned quads), in every lane: quad_perm
// [1,0,3,2], then quad_perm [2,3,0,1]
__device__ __forceinline__ u32 mx4q_block_or(u32 m) {
  m |= (u32)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xF, 0xF, true);
  return m | (u32)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xF, 0xF, true);
}

// eight fp32 bit patterns scaled by 2^-e (`scale` = 2^e) and rounded to e2m1:
// element i in nibble i
__device__ __forceinline__ u32 mx4q_cvt8(const u32 (&f)[8], float scale) {
  u32 w = 0;
  w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, mxq_float(f[0]), mxq_float(f[1]), scale, 0);
  w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, mxq_float(f[2]), mxq_float(f[3]), scale, 1);
  w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, mxq_float(f[4]), mxq_float(f[5]), scale, 2);
  return __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, mxq_float(f[6]), mxq_float(f[7]), scale, 3);
}

// the byte the block stores: 0xFF when one of its elements is a NaN
__device__ __forceinline__ u32 mx4q_stored_byte(u32 sb, u32 nan) { return mx4q_block_or(nan) ? 0xFFu : sb; }
