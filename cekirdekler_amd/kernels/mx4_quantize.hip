// MXFP4 quantisation on the device (HBM-bound): fp32 or bf16 in, OCP e2m1
// codes (two per byte: element 2i in bits 0-3 of byte i, element 2i + 1 in
// bits 4-7) plus one E8M0 scale byte per block of 32 consecutive elements
// out, bit for bit what ops/codecs.py's to_mxfp4 computes.  The repack of the
// row-major scale bytes into the dwords the GEMM kernels read is
// mx_quantize.hip's cek_mx_pack_scales, which does not look at the bytes.
//
// Work item i owns MX block i, the local size is 64, so a work-group (one
// wave) owns 64 consecutive blocks = 2048 elements = 1024 bytes of codes.
// Four lanes share a block for both sources: a lane has 8 consecutive
// elements (fp32: two 16-byte loads, bf16: one), whose codes are one whole
// dword.  One step of the wave covers 16 blocks, four steps the group; all
// loads are issued before the first use.
//
// Per step the block maximum of the finite |x| is taken on the bit patterns
// (integer max: nothing is flushed or canonicalised) with DPP inside the four
// lanes, and the scale byte max(E - 2, 0) comes from its exponent field E.
// The elements are scaled and rounded by v_cvt_scalef32_pk_fp4_f32 (two
// values per instruction into one byte of the dword, the first in the low
// nibble; the scale operand 2^e given by its exponent field alone, so
// e = -127 is field 0 and fp32 denormal inputs are scaled exactly).  Measured
// against the host codec on every designed pattern
// (profiles/quantize_mxfp4.md) the instruction is the codec: round to nearest
// even, whatever lies beyond 6 and ±inf saturated to ±6.  Only a NaN differs:
// it comes out as ±6.  e2m1 has no NaN: a NaN element gets code 0 (the
// per-element NaN nibbles of the input, cleared on the packed dword) and its
// block the scale byte 0xFF (an OR over the four lanes beside the maximum);
// the block's other elements keep the codes the finite maximum's scale gives
// them.  The bf16 kernel widens to fp32 (a shift or a mask per element, which
// the maximum needs anyway) and uses the same instruction:
// v_cvt_scalef32_pk_fp4_bf16 measured just as exact and is no shorter (four
// per dword either way), but fed bit casts of the loaded dwordx4's elements
// hipcc gave all four of a dword the first element.
//
// The group's 64 scale bytes are collected with four ds_bpermute into lanes
// 0..15 and stored as 16 dwords.  No LDS.
#include "cek_kernel.h"
#include "mx_quantize_parts.h"

extern "C" __global__ __launch_bounds__(64) void cek_mx4_quantize_f32(const u32x4* x, u32* codes, u32* scales,
                                                                       CEK_HIDDEN) {
  const int lane = (int)threadIdx.x;
  const long long group = cek_global_group_id();
  if (group * 64 >= __cek_gsize) return;
  const long long base = group * 256 + lane;  // in units of 8 elements
  u32x4 v[4][2];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    v[s][0] = x[(base + s * 64) * 2];
    v[s][1] = x[(base + s * 64) * 2 + 1];
  }
  u32 mine = 0;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const u32 f[8] = {v[s][0].x, v[s][0].y, v[s][0].z, v[s][0].w, v[s][1].x, v[s][1].y, v[s][1].z, v[s][1].w};
    int m = 0;
    u32 nan = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int key = mxq_key(f[i]);
      m = max(m, key);
      nan |= mx4q_nan_nibble(key, i);
    }
    const u32 sb = mxq_scale_byte<2>(mxq_block_max<4>(m));
    const float scale = mxq_float(sb << 23);  // 2^e, e = sb - 127
    const u32 w = mx4q_cvt8(f, scale);
    codes[base + s * 64] = w & ~nan;
    const u32 stored = mx4q_stored_byte(sb, nan);
    mine = (lane & 3) == s ? stored : mine;
  }
  mxq_store_scales<4>(mine, scales, group, lane);
}

extern "C" __global__ __launch_bounds__(64) void cek_mx4_quantize_bf16(const u32x4* x, u32* codes, u32* scales,
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
    u32 nan = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f[2 * q] = v[s][q] << 16;
      f[2 * q + 1] = v[s][q] & 0xffff0000u;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int key = mxq_key(f[i]);
      m = max(m, key);
      nan |= mx4q_nan_nibble(key, i);
    }
    const u32 sb = mxq_scale_byte<2>(mxq_block_max<4>(m));
    const float scale = mxq_float(sb << 23);
    const u32 w = mx4q_cvt8(f, scale);
    codes[base + s * 64] = w & ~nan;
    const u32 stored = mx4q_stored_byte(sb, nan);
    mine = (lane & 3) == s ? stored : mine;
  }
  mxq_store_scales<4>(mine, scales, group, lane);
}
