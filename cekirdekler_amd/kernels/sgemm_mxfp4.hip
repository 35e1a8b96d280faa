// MXFP4 GEMM (OCP Microscaling: e2m1 elements, two per byte, one E8M0 scale
// byte per block of 32 consecutive k) on CDNA4 matrix cores, fp32 accumulate /
// fp32 output, range-partitionable by compute() like sgemm_mxfp8.hip:
//
//   C = (A∘SA) · (Bt∘SB)ᵀ    A: [M][K/2], Bt: [N][K/2] bytes, row-major;
//   element 2i of a row is bits 0–3 of its byte i, element 2i + 1 bits 4–7;
//   code s e e m: 0, 0.5, 1, 1.5, 2, 3, 4, 6 and their negatives
//   SA: [M][K/32], SB: [N][K/32] E8M0: element = e2m1(code) · 2^(scale − 127)
//   C tile-major in MFMA-fragment order and dims exactly as sgemm_fp8.hip
//   (dims[2] = K in elements); arrays: dims, A, Bt, SAp, SBp, C.
//   M % BM = N % BN = K % 256 = 0.
//
// The tile function is gemm8_tile.h's with both formats GEMM8_E2M1.  That file is written in
// bytes, and in bytes nothing changes: LDS rows of 128 B, 16-B chunks
// XOR-swizzled by row & 7, staging by cek_stage_rows<…, 1> with a row pitch of
// K/2, the ping-pong loop of MODE 4.  A 128-B row now holds 256 k, which is
// two instructions v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz = blgp = 4
// (e2m1), each with a 16-B operand per lane (4 VGPRs) into the same
// accumulator.
//
// Operand and scale maps, measured on an MI355X by the single-instruction
// probe (tests/gemm4_oracles.py, tests/test_gpu_gemm_mxfp4.py; the record is
// profiles/gemm_mxfp4.md and the probe, not the ISA text, is the authority):
//   - data: lane l (row l % 16, q = l / 16) supplies k ∈ [32q, 32q + 32) of the
//     instruction's 128 k, in natural order: byte b of its 16 B holds k = 32q +
//     2b in bits 0–3 and k = 32q + 2b + 1 in bits 4–7.  Unlike the e4m3 form
//     (two 16×64 halves) a lane's data is exactly one MX block;
//   - scales: the byte of lane l applies to row l % 16 and MX block q = l / 16
//     of the step, which here IS the lane's own data; op_sel = b picks bits
//     8b .. 8b+7 of the scale register.
// So the public layout is the device layout, and step s of a K-tile reads the
// 16 B of row l % 16 at logical chunk 4s + q: sgemm_fp8.hip's read map
// a_off[s] / b_off[s] unchanged, and with it the bank argument of
// sgemm_mxfp8.hip (the two q of a 16-lane group read logical chunks that
// differ in bit 0: conflict-free).
//
// Packed scales.  pack_mx_scales's layout, unchanged, with "K-tile" read as
// "128-k step": SAp[K/128][M/64][64], byte i of dword (st·M/64 + g)·64 + l =
// SA[g·64 + i·16 + l % 16][st·4 + l / 16].  K-tile kt of 256 k uses steps
// st = 2kt and 2kt + 1, M dwords apart.  A wave reads dword g + d of both
// steps for fragments 4d .. 4d+3 and issues fragment i with op_sel = i & 3.
// 256×256: (2 + 1)·2 = 6 loads per wave and K-tile; 128×128: (1 + 1)·2 = 4.
//
// Scale loads and the ping-pong's vmcnt argument, re-derived for twice the
// loads.  As in sgemm_mxfp8.hip the scales go global → VGPR one K-tile ahead:
// iteration k loads the scales of K-tile k + 1 into registers of their own,
// at the TOP of the iteration, ahead of its staging, with a scheduling barrier
// between, and they become current after iteration k's MFMAs.  The two scale
// pointers stand at step 2·min(kt, nk − 1) and step 2M (2N) dwords per K-tile
// while there is one; the loads of step 1 add M (N) dwords.  At the last
// K-tile the pointers stay, so the prefetch re-reads steps 2(nk − 1) and
// 2(nk − 1) + 1 = K/128 − 1, the last of the array: every iteration issues the
// same six loads and none leaves SAp / SBp.  Vector memory loads retire in
// order and `s_waitcnt vmcnt(n)` waits until at most n are outstanding, so:
//   G1, read section k: outstanding at the wait are, oldest first, Bt k+1
//     (issued in iteration k−1), the scales of k+1 (6 loads where MXFP8 has 3)
//     and Bt k+2 (B_INSTR loads, the youngest).  The count names what may stay
//     in flight, not what must retire: vmcnt(B_INSTR) leaves only Bt k+2 and
//     therefore still retires Bt k+1 and the six scale loads.  The argument
//     B_INSTR does not change with the number of scale loads, because they are
//     older than every load it leaves outstanding.  In the last two iterations
//     nothing is staged and the wait is vmcnt(0).
//   G0: its vmcnt(0) behind the MFMA section retires A k+1 and the scales.
//   WAR on the scale registers: the prefetch lands in its own registers; the
//     copy to the current ones follows the MFMAs that read them.
// MODE 0 loads the next scales ahead of the next stage and its vmcnt(0)
// covers both.
//
// Registers (compiler's resource usage, profiles/gemm_mxfp4.md): the 256×256
// tile holds 128 accumulator, 96 fragment and 6 + 6 scale registers and comes
// to 245 VGPRs (MXFP8: 239), the 128×128 tile to 144 + 64 AGPRs; no scratch,
// no spills, so the prefetch structure is MXFP8's as it stands.
//
// Time.  Staging bytes, LDS reads and (by the instruction tables) matrix
// cycles per 128-B K-tile equal the MXFP8 kernel's, so the loop was expected
// to take the same time for twice the FLOPs.  Measured it takes 1.25× as long
// per K-tile (4164 TFLOP/s at 8192³, 1.54× MXFP8; profiles/gemm_mxfp4.md has
// the figures and what they point to: about a quarter of the gap is the three
// extra scale loads, the rest the matrix section, 64 instructions where MXFP8
// has 32, which this loop hardly hides behind anything).
#include "gemm8_tile.h"

// 128×128 tiles, 4 waves (2×2, 64×64 each), 64 KiB LDS, one stage in flight:
// the simple kernel the production tile is judged against.
CEK_GEMM8_MX_KERNEL(cek_sgemm_mxfp4_128x128, 2, 2, 4, 4, 0, GEMM8_E2M1, GEMM8_E2M1)
// 256×256 tiles, 8 waves (2×4, 128×64 each), balanced-DMA ping-pong, 160 KiB LDS.
CEK_GEMM8_MX_KERNEL(cek_sgemm_mxfp4_256x256pbx, 2, 4, 8, 4, 4, GEMM8_E2M1, GEMM8_E2M1)
