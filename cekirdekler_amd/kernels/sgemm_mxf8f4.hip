// Mixed MXFP8 × MXFP4 GEMM ("W4A8": 8-bit activations against 4-bit weights,
// both OCP Microscaling with one E8M0 scale byte per block of 32 consecutive
// k) on CDNA4 matrix cores, fp32 accumulate / fp32 output, range-partitionable
// by compute() like sgemm_mxfp8.hip and sgemm_mxfp4.hip:
//
//   C = (A∘SA) · (Bt∘SB)ᵀ    A: [M][K] e4m3fn bytes, row-major;
//   Bt: [N][K/2] bytes, row-major, element 2i of a row in bits 0–3 of its byte
//   i, element 2i + 1 in bits 4–7 (e2m1);
//   SA: [M][K/32], SB: [N][K/32] E8M0: element = code value · 2^(scale − 127)
//   C tile-major in MFMA-fragment order and dims exactly as sgemm_fp8.hip
//   (dims[2] = K in elements); arrays: dims, A, Bt, SAp, SBp, C.
//   M % BM = N % BN = K % 256 = 0.
// Only this orientation exists; 4-bit A against 8-bit Bt is the same product
// transposed.
//
// The instruction is v_mfma_scale_f32_16x16x128_f8f6f4 with one format
// selector per operand: cbsz = 0 (e4m3, a 32-B operand, 8 VGPRs) for A and
// blgp = 4 (e2m1, 16 B, 4 VGPRs) for Bt.  The tile function is gemm8_tile.h's
// with FA = GEMM8_E4M3 and FB = GEMM8_E2M1.  Bt is sgemm_mxfp4.hip's operand in every respect: LDS
// rows of 128 B = 256 k, row pitch K/2, staging, the ring of three buffers,
// the read b_off[s] of step s.  A is sgemm_mxfp8.hip's operand twice over:
// the K-tile of 256 k is two 128-B sub-tiles [2][BM][128], each staged by
// cek_stage_rows<…, 1> with a row pitch of K at byte K-tile 2·kt + h and the
// usual XOR swizzle, and step s reads a_off[0] and a_off[1] inside sub-tile s,
// exactly the MXFP8 kernel's two reads of that 128-k step.
//
// Operand and scale maps, measured on an MI355X by the single-instruction
// probe (tests/gemm84_oracles.py, tests/test_gpu_gemm_mxf8f4.py; the record is
// profiles/gemm_mxf8f4.md and the probe, not the ISA text, is the authority).
// Each operand keeps the map measured for its own format:
//   - A: lane l (row l % 16, q = l / 16) supplies k ∈ [16q, 16q + 16) in
//     registers 0–3 and k ∈ [64 + 16q, 64 + 16q + 16) in registers 4–7;
//   - Bt: lane l supplies k ∈ [32q, 32q + 32) in natural order, low nibble
//     first, in registers 0–3; registers 4–7 are ignored;
//   - scales, both operands: the byte of lane l applies to row l % 16 and MX
//     block q = l / 16 of the step; op_sel = b picks bits 8b .. 8b+7.
// So both public layouts are the device layouts, and the packed scales are
// pack_mx_scales's for both operands, addressed by 128-k step as in sgemm_mxfp4.hip:
// K-tile kt uses steps 2kt and 2kt + 1, M (N) dwords apart.
//
// Tiles.  128×128 (4 waves, 2×2, one stage in flight): 2·(32 + 16) KiB = 96
// KiB of LDS.  128×256 (8 waves, 2×4, FM = FN = 4, ping-pong): a 256×256 tile
// at a 256-k K-tile would need 2·64 + 3·32 = 224 KiB; 128×256 holds 2·32 +
// 3·32 = 160 KiB and is, byte for byte and instruction for instruction, the
// MXFP8 256x256pbx loop: 32 KiB of A and 32 KiB of Bt per K-tile, A_INSTR =
// B_INSTR = 8 staging loads per staging wave, 384 B of fragment reads per
// lane, 32 matrix instructions per wave, 2·128·256·256 FLOPs.
//
// Hazards of the ping-pong (MODE 4), re-derived for this geometry.  G0 (waves
// 0–3) stages A one K-tile ahead into buffer (k+1) & 1, both sub-tiles, 2·4
// loads; G1 (waves 4–7) stages Bt two K-tiles ahead into buffer (k+2) % 3.
//   WAR: A buffer (k+1) & 1 was last read in the read sections of K-tile k−1,
//     Bt buffer (k+2) % 3 in those of K-tile k−1 too; both groups' read
//     sections of k−1 end before the barrier that precedes iteration k's
//     staging issue in either group.  A sub-tile changes nothing: both halves
//     of a buffer are read in one read section and written by one staging issue.
//   RAW: G0's vmcnt(0) behind its MFMA section retires A k+1 (all 8 loads) and
//     the scales before the barrier after which anyone reads them.  G1, read
//     section k: outstanding at the wait are, oldest first, Bt k+1, the scales
//     of K-tile k+1 (2 + 2 loads: SA_G = SB_G = 1, two steps) and Bt k+2
//     (B_INSTR = 8 loads, the youngest).  vmcnt(B_INSTR) leaves only Bt k+2
//     in flight, so Bt k+1 and the four scale loads have retired: the scale
//     loads are issued at the top of the iteration, ahead of its staging, with
//     a scheduling barrier between.  In the last two iterations nothing is
//     staged and the wait is vmcnt(0).
//   Scale registers: the prefetch lands in registers of its own and becomes
//     current behind the MFMAs that read the current ones.  At the last K-tile
//     the scale pointers stay, so the prefetch re-reads steps K/128 − 2 and
//     K/128 − 1: no load leaves SAp / SBp.
// MODE 0 loads the next scales ahead of the next stage and its vmcnt(0) covers
// both.
//
// The sum over k is the e4m3 path's: inside a group of 8 neighbouring k the
// products are aligned to the largest and 14 bits are kept (measured for the
// mixed form as well); across MX blocks nothing is lost.
//
// Registers (compiler's resource usage, profiles/gemm_mxf8f4.md): 64
// accumulator, 64 + 32 fragment and 4 + 4 scale registers per wave; the
// 128×256 tile comes to 191 VGPRs, the 128×128 tile to 188 + 64 AGPRs; no
// scratch, no spills.
//
// Time (profiles/gemm_mxf8f4.md): at 8192³ the 128×256 tile takes 0.992 of the
// MXFP8 256x256pbx kernel's time per step (2741 TFLOP/s), inside that kernel's
// run-to-run spread: the mixed instruction runs at the 8-bit rate, and what
// the 4-bit B buys is half of B's memory and upload.
#include "gemm8_tile.h"

// 128×128 tiles, 4 waves (2×2, 64×64 each), 96 KiB LDS, one stage in flight:
// the simple kernel the production tile is judged against.
CEK_GEMM8_MX_KERNEL(cek_sgemm_mxf8f4_128x128, 2, 2, 4, 4, 0, GEMM8_E4M3, GEMM8_E2M1)
// 128×256 tiles, 8 waves (2×4, 64×64 each), balanced-DMA ping-pong, 160 KiB LDS.
CEK_GEMM8_MX_KERNEL(cek_sgemm_mxf8f4_128x256pbx, 2, 4, 4, 4, 4, GEMM8_E4M3, GEMM8_E2M1)
