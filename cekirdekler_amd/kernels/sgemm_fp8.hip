// fp8 (OCP e4m3fn) GEMM on CDNA4 matrix cores, fp32 accumulate / fp32
// output, range-partitionable by compute() like sgemm_bf16.hip:
//
//   C = A · Bᵀ      A: [M][K] e4m3fn row-major, Bt: [N][K] e4m3fn row-major
//   C is written TILE-MAJOR in MFMA-fragment order, exactly as the bf16
//   kernels write it (ops/tiling.py tile_to_rows restores rows), one work-group
//   per BM×BN tile, dims = the bf16 kernels' 8 words.
//
// The byte geometry is the bf16 kernels' (gemm_parts.h at ESZ = 1): LDS rows
// of 128 B are now BK = 128 elements, staged by global_load_lds_dwordx4 with
// the 16-B chunk XOR-swizzled by (row & 7).  M % BM = N % BN = K % 128 = 0.
//
// Fragments.  A lane reads what the bf16 kernels read: for k block s = 0, 1
// the 16 B of row (l % 16) at logical chunk s·4 + l/16.  The sum over k does
// not depend on the order of k as long as A and Bt use one order, and both
// operands are read with the same map, so
//   - the non-scaled form (v_mfma_f32_16x16x32_fp8_fp8, 8 B per lane) takes
//     the low and the high 8 B of each read as two k steps: four steps per
//     K-tile, at the bf16 rate;
//   - the scaled form (v_mfma_scale_f32_16x16x128_f8f6f4, 32 B per lane, both
//     formats e4m3, both block scales 1 = E8M0 127) takes reads s = 0 and 1
//     together: one instruction per fragment pair and K-tile, at the fp8 rate.
// tests/test_gpu_gemm_fp8.py checks the pairing with exact data.
// The tile function is gemm8_tile.h, shared with sgemm_mxfp8.hip.
#include "gemm8_tile.h"

// 128×128 tiles, 4 waves (2×2, 64×64 each), 64 KiB LDS, one stage in flight:
// the simple kernel the others are judged against.
CEK_GEMM8_KERNEL(cek_sgemm_fp8_128x128, 2, 2, 4, 4, 0, GEMM8_K32, GEMM8_E4M3, GEMM8_E4M3)
// 256×256 tiles, 8 waves (2×4, 128×64 each), balanced-DMA ping-pong, 160 KiB LDS.
CEK_GEMM8_KERNEL(cek_sgemm_fp8_256x256pb, 2, 4, 8, 4, 4, GEMM8_K32, GEMM8_E4M3, GEMM8_E4M3)
// the same with the scaled 16x16x128 instruction (unit scales)
CEK_GEMM8_KERNEL(cek_sgemm_fp8_256x256pbx, 2, 4, 8, 4, 4, GEMM8_UNIT, GEMM8_E4M3, GEMM8_E4M3)
