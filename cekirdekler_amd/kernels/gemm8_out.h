// The output modes of gemm8_tile (gemm8_tile.h) other than its own fp32
// store: the tile goes out row-major as the next layer's operand, bf16 or
// quantised to MXFP8 / MXFP4 with blocks of 32 along N (sgemm_mx_out.hip has
// the layouts).  An optional activation is applied to the fp32 accumulator
// first.
//
// Geometry.  A wave owns 16·FM rows × 64 columns (FN = 4: two MX blocks per
// row).  A lane holds 4 consecutive ROWS of one column per fragment, so the
// wave turns each 16-row strip around in LDS exactly as sgemm_bf16.hip's ROWC
// epilogue does (row stride 68 floats, the wave's own 4352 B; the main loop is
// done with LDS behind the caller's barrier) and then reads rows:
//   bf16, MXFP8: lane l reads 16 B = columns 4(l % 16) .. +3 of row 4q + l / 16,
//     q = 0 .. 3.  Eight aligned lanes hold one MX block: the geometry of
//     cek_mx_quantize_f32, whose steps apply as they stand.  A lane stores 8 B
//     of bf16 or one dword of codes.
//   MXFP4: lane l reads 2 × 16 B = columns 8(l % 8) .. +7 of row 8q + l / 8,
//     q = 0, 1.  Four aligned lanes hold one block (cek_mx4_quantize_f32) and
//     a lane's eight codes are one dword.
// The two scale bytes of a row (the wave's two blocks) are joined in the
// row's first lane and stored as one 16-bit word: SY is [M][N/32] row-major,
// N/32 is a multiple of 4 and a wave's first block index is even.
#pragma once
#include "mx_quantize_parts.h"

enum { GEMM8_OUT_F32 = 0, GEMM8_OUT_BF16 = 1, GEMM8_OUT_MXFP8 = 2, GEMM8_OUT_MXFP4 = 3 };

// The activation on the bit pattern.  ReLU: x > 0 → x, NaN → NaN, everything
// else (−0 included) → +0.  Integer compares: v_max_f32(x, 0) would not keep a
// NaN, and nothing here depends on the denormal mode.
__device__ __forceinline__ u32 gemm8_act(u32 u, bool relu) {
  const bool keep = (int)u > 0 || (u & 0x7fffffffu) > 0x7f800000u;
  return relu && !keep ? 0u : u;
}

// fp32 bits → bf16 bits, round to nearest even; a NaN keeps its high half and
// gets a quiet bit (ops/codecs.py to_bf16_bits)
__device__ __forceinline__ u32 gemm8_bf16_bits(u32 u) {
  const u32 r = (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
  return (u & 0x7fffffffu) > 0x7f800000u ? (u >> 16) | 0x40u : r;
}

// row0 / col0: the wave's first row and column in C; Y: [M][N] in the output
// format; SY: [M][N/32] scale bytes (MX modes)
template <int FM, int FN, int OUT>
__device__ __forceinline__ void gemm8_store_out(const f32x4 (&acc)[FM][FN], char* smem, void* __restrict__ Y,
                                                uint8_t* __restrict__ SY, int N, bool relu, int row0, int col0,
                                                int wave, int lane) {
  static_assert(FN == 4, "a wave's 64 columns are two MX blocks");
  static_assert(OUT == GEMM8_OUT_BF16 || OUT == GEMM8_OUT_MXFP8 || OUT == GEMM8_OUT_MXFP4, "output mode");
  constexpr int RS = 16 * FN + 4;
  const int fr = lane & 15, fq = lane >> 4;
  float* strip = reinterpret_cast<float*>(smem) + wave * 16 * RS;
  const int nb = N / 32;
#pragma unroll
  for (int i = 0; i < FM; ++i) {
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) strip[(fq * 4 + r) * RS + j * 16 + fr] = acc[i][j][r];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's strip is written
    if constexpr (OUT == GEMM8_OUT_MXFP4) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int row = q * 8 + (lane >> 3), col = (lane & 7) * 8;
        const u32x4 v0 = __builtin_bit_cast(u32x4, *reinterpret_cast<const f32x4*>(strip + row * RS + col));
        const u32x4 v1 = __builtin_bit_cast(u32x4, *reinterpret_cast<const f32x4*>(strip + row * RS + col + 4));
        const u32 f[8] = {gemm8_act(v0.x, relu), gemm8_act(v0.y, relu), gemm8_act(v0.z, relu),
                          gemm8_act(v0.w, relu), gemm8_act(v1.x, relu), gemm8_act(v1.y, relu),
                          gemm8_act(v1.z, relu), gemm8_act(v1.w, relu)};
        int m = 0;
        u32 nan = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int key = mxq_key(f[e]);
          m = max(m, key);
          nan |= mx4q_nan_nibble(key, e);
        }
        const u32 sb = mxq_scale_byte<2>(mxq_block_max<4>(m));
        const u32 w = mx4q_cvt8(f, mxq_float(sb << 23));
        const size_t grow = (size_t)(row0 + i * 16 + row);
        reinterpret_cast<u32*>(Y)[(grow * N + col0 + col) >> 3] = w & ~nan;
        const u32 stored = mx4q_stored_byte(sb, nan);
        const u32 next = (u32)__builtin_amdgcn_ds_bpermute((lane + 4) << 2, (int)stored);
        if ((lane & 7) == 0)
          *reinterpret_cast<uint16_t*>(SY + grow * nb + (col0 >> 5)) = (uint16_t)(stored | (next << 8));
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = q * 4 + (lane >> 4), col = (lane & 15) * 4;
        const u32x4 v = __builtin_bit_cast(u32x4, *reinterpret_cast<const f32x4*>(strip + row * RS + col));
        const u32 x0 = gemm8_act(v.x, relu), x1 = gemm8_act(v.y, relu), x2 = gemm8_act(v.z, relu),
                  x3 = gemm8_act(v.w, relu);
        const size_t grow = (size_t)(row0 + i * 16 + row);
        if constexpr (OUT == GEMM8_OUT_BF16) {
          u32x2 o;
          o.x = gemm8_bf16_bits(x0) | (gemm8_bf16_bits(x1) << 16);
          o.y = gemm8_bf16_bits(x2) | (gemm8_bf16_bits(x3) << 16);
          reinterpret_cast<u32x2*>(Y)[(grow * N + col0 + col) >> 2] = o;
        } else {
          const int k0 = mxq_key(x0), k1 = mxq_key(x1), k2 = mxq_key(x2), k3 = mxq_key(x3);
          const u32 sb = mxq_scale_byte<8>(mxq_block_max<8>(max(max(k0, k1), max(k2, k3))));
          const u32 nan = mxq_nan_bit(k0, 0) | mxq_nan_bit(k1, 1) | mxq_nan_bit(k2, 2) | mxq_nan_bit(k3, 3);
          const float scale = mxq_float(sb << 23);  // 2^e, e = sb - 127
          reinterpret_cast<u32*>(Y)[(grow * N + col0 + col) >> 2] =
              mxq_fix(mxq_cvt4(mxq_float(x0), mxq_float(x1), mxq_float(x2), mxq_float(x3), scale), nan);
          const u32 next = (u32)__builtin_amdgcn_ds_bpermute((lane + 8) << 2, (int)sb);
          if ((lane & 15) == 0)
            *reinterpret_cast<uint16_t*>(SY + grow * nb + (col0 >> 5)) = (uint16_t)(sb | (next << 8));
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // reads done before the strip is rewritten
  }
}
