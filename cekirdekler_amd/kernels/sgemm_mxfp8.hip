// MXFP8 GEMM (OCP Microscaling: e4m3fn elements, one E8M0 scale byte per
// block of 32 consecutive k) on CDNA4 matrix cores, fp32 accumulate / fp32
// output, range-partitionable by compute() like sgemm_fp8.hip:
//
//   C = (A∘SA) · (Bt∘SB)ᵀ    A: [M][K], Bt: [N][K] e4m3fn row-major
//   SA: [M][K/32], SB: [N][K/32] E8M0: element = e4m3(code) · 2^(scale − 127)
//   C tile-major in MFMA-fragment order and dims exactly as sgemm_fp8.hip;
//   arrays: dims, A, Bt, SAp, SBp, C.  M % BM = N % BN = K % 128 = 0.
//
// The tile function, the byte geometry (LDS rows of 128 B = one K-tile of 128
// elements, 16-B chunks XOR-swizzled by row & 7) and the ping-pong loop are
// gemm8_tile.h's, shared with sgemm_fp8.hip; what is particular to MX:
//
// Fragment read map and which scale meets which bytes.  The instruction
// v_mfma_scale_f32_16x16x128_f8f6f4 takes 32 operand bytes and ONE scale byte
// per lane and operand.  Measured on an MI355X with single scale entries set
// (tests/test_gpu_gemm_mxfp8.py, test_scale_mapping_probe, is the standing
// check and the authority; the ISA text can be read as "a lane's 32 bytes are
// one block", which the hardware does not do):
//   - data: lane l (row l % 16, q = l / 16) supplies k ∈ [16q, 16q + 16) in
//     its low 16 B and k ∈ [64 + 16q, 64 + 16q + 16) in its high 16 B — the
//     operand is two 16×64 halves, registers 0–3 and 4–7;
//   - scales: the byte of lane l applies to row l % 16 and MX block q = l / 16,
//     that is to k ∈ [32q, 32q + 32) of the K-tile: the low halves of lanes
//     q' = 2q, 2q + 1 for q < 2, the high halves of q' = 2(q − 2), 2(q − 2) + 1
//     otherwise.  A lane's scale byte thus does not scale the lane's own data.
// So the natural order of k is the one that works, and the map is
// sgemm_fp8.hip's unchanged: read s = 0, 1 takes the 16 B of row l % 16 at
// logical chunk 4s + q.  (Any other map would have to keep every 32-k block
// together under the hardware's k numbering; there is nothing to gain.)
//
// LDS banks.  The map being sgemm_fp8.hip's, so is its bank behaviour:
// ds_read_b128 is served in four groups of 16 lanes ({0–3, 12–15, 20–27},
// {4–11, 16–19, 28–31} and the same + 32); the bank of a 16-B read is
// ((row & 1)·8 + physical chunk)·4 .. +3 of 64, so a group is conflict-free
// when its 16 lanes hit 16 different (row & 1, physical chunk) pairs.  Every
// group has 8 lanes of an even q whose rows & 7 are 0..7 and 8 lanes of q + 1
// whose rows & 7 are 0..7 again.  With physical = logical ^ (row & 7), the
// four even rows of one q take logical ^ {0, 2, 4, 6}: the four chunks that
// share the logical chunk's bit 0 (odd rows: the other four).  Logical chunks
// 4s + q and 4s + q + 1 differ in bit 0, so the 16 lanes cover all 16 pairs:
// conflict-free.  (Reading one MX block per lane, chunks 2q and 2q + 1 in
// read s = 0, 1, would give both q of a group the same bit 0 and a 2-way
// conflict on every read — one more reason the hardware's layout is welcome.)
//
// Packed scales.  The 256×256 tile has 8 A and 4 Bt fragments per wave; one
// scale dword per fragment, double-buffered, does not fit beside 233 VGPRs.
// The instruction's op_sel picks one of the four bytes of its scale VGPR, so
// the host packs the scales of four fragments into one dword:
//
//   SAp[kt][g][l] (uint32, kt < K/128, g < M/64, l < 64):
//     byte i (bits 8i .. 8i+7) = SA[g·64 + i·16 + l % 16][kt·4 + l / 16]
//   dword index = (kt · M/64 + g)·64 + l; SBp the same from SB with N for M.
//
// (ops/tiling.py pack_mx_scales / unpack_mx_scales; private to that file and
// this one.)  A wave whose rows start at 64·g reads dword g + d for fragments
// 4d .. 4d+3 and issues fragment i with op_sel = i & 3 (op_sel = b picks bits
// 8b .. 8b+7, checked by the same probe): one coalesced 256-B
// load per dword, 2 + 1 per wave and K-tile for 256×256, 1 + 1 for 128×128.
//
// Scale loads and the ping-pong's vmcnt argument.  LDS is full in MODE 4
// (160 KiB), so the scales go global → VGPR, one K-tile ahead: iteration k
// loads the scales of K-tile k + 1 (clamped to the last K-tile, so every
// iteration issues the same loads and none leaves the arrays) and they become
// current after iteration k's MFMAs.  The two scale pointers step one K-tile
// per load instead of being recomputed (the 64-bit multiplies ahead of the
// staging issue cost 4 % at 8192³).  The loads are issued at the TOP of the
// iteration, ahead of its staging, with a scheduling barrier between.  Vector
// memory loads retire in order, and `s_waitcnt vmcnt(n)` waits until at most
// n are outstanding, so:
//   G1, read section k: outstanding at the wait are, oldest first, Bt k+1
//     (issued in iteration k−1), the scales of k+1 (3 loads) and Bt k+2
//     (B_INSTR loads, the youngest).  vmcnt(B_INSTR) therefore still retires
//     Bt k+1 — the RAW argument is unchanged — and the scales of k+1 with it;
//     the count B_INSTR does not change.  In the last two iterations nothing
//     is staged and the wait is vmcnt(0).
//   G0: its vmcnt(0) behind the MFMA section retires A k+1 and the scales.
//   WAR on the scale registers: the prefetch lands in its own registers; the
//     copy to the current ones follows the MFMAs that read them.
// MODE 0 loads the next scales ahead of the next stage and its vmcnt(0)
// covers both.
#include "gemm8_tile.h"

// 128×128 tiles, 4 waves (2×2, 64×64 each), 64 KiB LDS, one stage in flight:
// the simple kernel the production tile is judged against.
CEK_GEMM8_MX_KERNEL(cek_sgemm_mxfp8_128x128, 2, 2, 4, 4, 0, GEMM8_E4M3, GEMM8_E4M3)
// 256×256 tiles, 8 waves (2×4, 128×64 each), balanced-DMA ping-pong, 160 KiB LDS.
CEK_GEMM8_MX_KERNEL(cek_sgemm_mxfp8_256x256pbx, 2, 4, 8, 4, 4, GEMM8_E4M3, GEMM8_E4M3)
