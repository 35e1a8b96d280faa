// The MXFP8 and MXFP4 GEMMs (sgemm_mxfp8.hip, sgemm_mxfp4.hip) with an output
// the next layer can read where it lies: the same tile function, the same
// loop and therefore the same fp32 accumulators, and instead of the fp32 C in
// fragment order a row-major [M][N] store through gemm8_out.h:
//
//   _bf16:  Y [M][N] bf16 (round to nearest even; a NaN stays a NaN)
//   _mxfp8: Y [M][N] e4m3fn codes, SY [M][N/32] E8M0 bytes, blocks of 32 along
//           N: the layout of an A / SA operand with K = N, bit for bit
//           ops/codecs.py's to_mxfp8 of the fp32 values
//   _mxfp4: Y [M][N/2] e2m1 codes, two per byte, and SY: to_mxfp4, the scale
//           byte 0xFF for a block that holds a NaN included
//
// dims as in sgemm_fp8.hip plus dims[5]: the activation applied to the fp32
// accumulator before the conversion (0: none, 1: ReLU).  Arrays: dims, A, Bt,
// SAp, SBp, Y and, for the MX outputs, SY.  The packed scales a consuming
// GEMM reads are made from SY by mx_quantize.hip's cek_mx_pack_scales.
//
// A device's range of tiles is a block of rows of Y and SY only when it is
// whole tile groups (ops/gemm.py splits that way on several devices).
#include "gemm8_tile.h"

// the tiles of sgemm_mxfp8.hip and sgemm_mxfp4.hip, the three outputs of each
CEK_GEMM8_MX_OUT_TILE(cek_sgemm_mxfp8_128x128, 2, 2, 4, 4, 0, GEMM8_E4M3, GEMM8_E4M3)
CEK_GEMM8_MX_OUT_TILE(cek_sgemm_mxfp8_256x256pbx, 2, 4, 8, 4, 4, GEMM8_E4M3, GEMM8_E4M3)
CEK_GEMM8_MX_OUT_TILE(cek_sgemm_mxfp4_128x128, 2, 2, 4, 4, 0, GEMM8_E2M1, GEMM8_E2M1)
CEK_GEMM8_MX_OUT_TILE(cek_sgemm_mxfp4_256x256pbx, 2, 4, 8, 4, 4, GEMM8_E2M1, GEMM8_E2M1)
