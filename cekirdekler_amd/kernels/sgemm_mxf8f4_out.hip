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

#define CEK_SY_PARAMS_0
#define CEK_SY_PARAMS_1 uint8_t *SY,
#define CEK_SY_ARG_0 nullptr
#define CEK_SY_ARG_1 SY
#define CEK_GEMM84_OUT_KERNEL(NAME, WM, WN, FM, FN, MODE, OUT, HAS_SY)                                           \
  extern "C" __global__ __launch_bounds__(64 * WM * WN) void NAME(                                               \
      const int* dims, const uint8_t* A, const uint8_t* Bt, const int* SAp, const int* SBp, uint8_t* Y,          \
      CEK_SY_PARAMS_##HAS_SY CEK_HIDDEN) {                                                                        \
    __shared__ __attribute__((aligned(16))) char smem[gemm8_lds_bytes(WM, WN, FM, FN, MODE, true)];              \
    gemm8_tile<WM, WN, FM, FN, MODE, true, true, true, OUT, true>(dims, A, Bt, reinterpret_cast<float*>(Y),      \
                                                                  smem, __cek_off, SAp, SBp,                      \
                                                                  CEK_SY_ARG_##HAS_SY);                           \
  }
// the three outputs of one tile
#define CEK_GEMM84_OUT_TILE(STEM, WM, WN, FM, FN, MODE)                                \
  CEK_GEMM84_OUT_KERNEL(STEM##_bf16, WM, WN, FM, FN, MODE, GEMM8_OUT_BF16, 0)          \
  CEK_GEMM84_OUT_KERNEL(STEM##_mxfp8, WM, WN, FM, FN, MODE, GEMM8_OUT_MXFP8, 1)        \
  CEK_GEMM84_OUT_KERNEL(STEM##_mxfp4, WM, WN, FM, FN, MODE, GEMM8_OUT_MXFP4, 1)

// the tiles of sgemm_mxf8f4.hip
CEK_GEMM84_OUT_TILE(cek_sgemm_mxf8f4_128x128, 2, 2, 4, 4, 0)
CEK_GEMM84_OUT_TILE(cek_sgemm_mxf8f4_128x256pbx, 2, 4, 4, 4, 4)
