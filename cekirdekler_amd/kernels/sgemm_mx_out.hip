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

#define CEK_SY_PARAMS_0
#define CEK_SY_PARAMS_1 uint8_t *SY,
#define CEK_SY_ARG_0 nullptr
#define CEK_SY_ARG_1 SY
#define CEK_GEMM_MX_OUT_KERNEL(NAME, F4, WM, WN, FM, FN, MODE, OUT, HAS_SY)                                      \
  extern "C" __global__ __launch_bounds__(64 * WM * WN) void NAME(                                               \
      const int* dims, const uint8_t* A, const uint8_t* Bt, const int* SAp, const int* SBp, uint8_t* Y,          \
      CEK_SY_PARAMS_##HAS_SY CEK_HIDDEN) {                                                                        \
    __shared__ __attribute__((aligned(16))) char smem[gemm8_lds_bytes(WM, WN, FM, FN, MODE)];                    \
    gemm8_tile<WM, WN, FM, FN, MODE, true, true, F4, OUT>(dims, A, Bt, reinterpret_cast<float*>(Y), smem,        \
                                                          __cek_off, SAp, SBp, CEK_SY_ARG_##HAS_SY);             \
  }
// the three outputs of one operand format and tile
#define CEK_GEMM_MX_OUT_TILE(STEM, F4, WM, WN, FM, FN, MODE)                                  \
  CEK_GEMM_MX_OUT_KERNEL(STEM##_bf16, F4, WM, WN, FM, FN, MODE, GEMM8_OUT_BF16, 0)            \
  CEK_GEMM_MX_OUT_KERNEL(STEM##_mxfp8, F4, WM, WN, FM, FN, MODE, GEMM8_OUT_MXFP8, 1)          \
  CEK_GEMM_MX_OUT_KERNEL(STEM##_mxfp4, F4, WM, WN, FM, FN, MODE, GEMM8_OUT_MXFP4, 1)

// the tiles of sgemm_mxfp8.hip and sgemm_mxfp4.hip
CEK_GEMM_MX_OUT_TILE(cek_sgemm_mxfp8_128x128, false, 2, 2, 4, 4, 0)
CEK_GEMM_MX_OUT_TILE(cek_sgemm_mxfp8_256x256pbx, false, 2, 4, 8, 4, 4)
CEK_GEMM_MX_OUT_TILE(cek_sgemm_mxfp4_128x128, true, 2, 2, 4, 4, 0)
CEK_GEMM_MX_OUT_TILE(cek_sgemm_mxfp4_256x256pbx, true, 2, 4, 8, 4, 4)
