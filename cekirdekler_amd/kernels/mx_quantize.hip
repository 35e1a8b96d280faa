// MXFP8 quantisation on the device (HBM-bound): fp32 or bf16 in, OCP e4m3fn
// codes plus one E8M0 scale byte per block of 32 consecutive elements out,
// bit for bit what ops/codecs.py's to_mxfp8 computes, and the repack of the
// row-major scale bytes into the dwords the MXFP8 GEMM kernels read
// (sgemm_mxfp8.hip, pack_mx_scales).
//
// Quantise: work item i owns MX block i, the local size is 64, so a
// work-group (one wave) owns 64 consecutive blocks = 2048 elements.  LPB
// lanes share a block (fp32: 8 lanes × float4, bf16: 4 lanes × 8 values; 16 B
// per lane either way), so one step of the wave reads 1 KiB contiguous and
// covers 64 / LPB blocks, and LPB steps cover the group.  All loads are issued
// before the first use.
//
// Per step the block maximum of the finite |x| is taken on the bit patterns
// (integer max: nothing is flushed or canonicalised) with DPP inside the LPB
// lanes, and the scale byte comes from its exponent field.  The elements are
// scaled and rounded by v_cvt_scalef32_pk_fp8_f32 (two values per
// instruction, the scale operand 2^e given by its exponent field alone, so
// e = -127 is field 0 and fp32 denormal inputs are scaled exactly).  Measured
// against the host codec on every designed pattern (profiles/quantize_mxfp8.md)
// the instruction rounds to nearest even exactly like the codec, subnormals
// included, and differs in two places: what rounds past 448 (and inf) becomes
// a NaN code where the codec saturates to ±448, and a NaN keeps a sign where
// the codec writes 0x7f.  Both are put right on the packed dword with the
// per-element NaN bits of the input (mxq_fix).
//
// A lane stores its codes as one dword (fp32) or two (bf16); the group's 64
// scale bytes are collected with four ds_bpermute into lanes 0..15 and stored
// as 16 dwords.  No LDS.
//
// Pack: work item i writes packed dword i = (kt·R/64 + g)·64 + l, whose byte b
// is S[g·64 + b·16 + l % 16][kt·4 + l / 16].  Lane l loads the dword
// S[g·64 + l][kt·4 .. kt·4 + 3]; four ds_bpermute transpose the 64 × 4 bytes.
#include "cek_kernel.h"
#include "mx_quantize_parts.h"

extern "C" __global__ __launch_bounds__(64) void cek_mx_quantize_f32(const u32x4* x, u32* codes, u32* scales,
                                                                      CEK_HIDDEN) {
  const int lane = (int)threadIdx.x;
  const long long group = cek_global_group_id();
  if (group * 64 >= __cek_gsize) return;
  const long long base = group * 512 + lane;  // in units of 4 elements
  u32x4 v[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) v[s] = x[base + s * 64];
  u32 mine = 0;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const int k0 = mxq_key(v[s].x), k1 = mxq_key(v[s].y), k2 = mxq_key(v[s].z), k3 = mxq_key(v[s].w);
    const u32 sb = mxq_scale_byte<8>(mxq_block_max<8>(max(max(k0, k1), max(k2, k3))));
    const u32 nan = mxq_nan_bit(k0, 0) | mxq_nan_bit(k1, 1) | mxq_nan_bit(k2, 2) | mxq_nan_bit(k3, 3);
    const float scale = mxq_float(sb << 23);  // 2^e, e = sb - 127
    codes[base + s * 64] = mxq_fix(
        mxq_cvt4(mxq_float(v[s].x), mxq_float(v[s].y), mxq_float(v[s].z), mxq_float(v[s].w), scale), nan);
    mine = (lane & 7) == s ? sb : mine;
  }
  mxq_store_scales<8>(mine, scales, group, lane);
}

extern "C" __global__ __launch_bounds__(64) void cek_mx_quantize_bf16(const u32x4* x, u32x2* codes, u32* scales,
                                                                       CEK_HIDDEN) {
  const int lane = (int)threadIdx.x;
  const long long group = cek_global_group_id();
  if (group * 64 >= __cek_gsize) return;
  const long long base = group * 256 + lane;  // in units of 8 elements
  u32x4 v[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) v[s] = x[base + s * 64];
  u32 mine = 0;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    u32 f[8];  // bf16 bit patterns are the high halves of fp32's
    int m = 0;
    u32x2 nan = {0, 0};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f[2 * q] = v[s][q] << 16;
      f[2 * q + 1] = v[s][q] & 0xffff0000u;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int key = mxq_key(f[i]);
      m = max(m, key);
      nan[i >> 2] |= mxq_nan_bit(key, i & 3);
    }
    const u32 sb = mxq_scale_byte<8>(mxq_block_max<4>(m));
    const float scale = mxq_float(sb << 23);
    u32x2 c;
    c.x = mxq_fix(mxq_cvt4(mxq_float(f[0]), mxq_float(f[1]), mxq_float(f[2]), mxq_float(f[3]), scale), nan.x);
    c.y = mxq_fix(mxq_cvt4(mxq_float(f[4]), mxq_float(f[5]), mxq_float(f[6]), mxq_float(f[7]), scale), nan.y);
    codes[base + s * 64] = c;
    mine = (lane & 3) == s ? sb : mine;
  }
  mxq_store_scales<4>(mine, scales, group, lane);
}

// dims = {R, K}; S row-major [R][K/32] read as dwords [R][K/128]; P [K/128][R/64][64]
extern "C" __global__ __launch_bounds__(64) void cek_mx_pack_scales(const int* dims, const u32* s, u32* p,
                                                                     CEK_HIDDEN) {
  const int lane = (int)threadIdx.x;
  const long long t = cek_global_group_id();  // kt · R/64 + g
  const long long G = dims[0] / 64, KT = dims[1] / 128;
  if (t * 64 >= __cek_gsize || t >= KT * G) return;
  const u32 kt = (u32)t / (u32)G, g = (u32)t % (u32)G;  // t < KT·G = R·K / 8192 fits 32 bits
  const u32 mine = s[((long long)g * 64 + lane) * KT + kt];  // row g·64 + lane, blocks kt·4 .. kt·4 + 3
  const int fr = lane & 15, fq = lane >> 4;
  u32 w = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const u32 row = (u32)__builtin_amdgcn_ds_bpermute((b * 16 + fr) << 2, (int)mine);
    w |= ((row >> (8 * fq)) & 0xffu) << (8 * b);
  }
  p[t * 64 + lane] = w;
}
