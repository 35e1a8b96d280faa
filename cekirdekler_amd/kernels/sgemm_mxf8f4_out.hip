// The mixed MXFP8 × MXFP4 GEMMs (sgemm_mxf8f4.hip) with an output the next
// layer can read where it lies, as sgemm_mx_out.hip has it for the pure
// formats: the same tile function, loop and fp32 accumulators, and instead of
// the fp32 C in fragment order a row-major [M][N] store through gemm8_out.h:
//
//   _bf16:  Y [M][N] bf16
//   _mxfp8: Y [M][N] e4m3fn codes, SY [M][N/32] E8M0 bytes (an A / SA operand
//           of the next mixed GEMM with K = N)
//   _mxfp4: Y [M][N/2] e2m1 codes, two per byte, and SY
//
// dims as in sgemm_fp8.hip plus dims[5]: the activation (0: none, 1: ReLU).
// Arrays: dims, A, Bt, SAp, SBp, Y and, for the MX outputs, SY.
#include "gemm8_tile.h"

// the tiles of sgemm_mxf8f4.hip, the three outputs of each
CEK_GEMM8_MX_OUT_TILE(cek_sgemm_mxf8f4_128x128, 2, 2, 4, 4, 0, GEMM8_E4M3, GEMM8_E2M1)
CEK_GEMM8_MX_OUT_TILE(cek_sgemm_mxf8f4_128x256pbx, 2, 4, 4, 4, 4, GEMM8_E4M3, GEMM8_E2M1)
