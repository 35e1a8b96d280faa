// Parts the GEMM tile functions (sgemm_bf16.hip, sgemm_f32.hip) have in
// common, each written once.  The byte geometry is
// the same for every element size ESZ: LDS rows are 128 B (BK = 128 / ESZ
// elements), one wave instruction of global_load_lds_dwordx4 fills 8 rows =
// 1 KiB, and the 16-B chunk index is XOR-swizzled with (row & 7) on the
// global source address and on the ds_read_b128 address.
//
// A change here or in a tile function that is meant to leave a kernel alone
// is checked with tools/kernel_identity.py: the device code must not change
// by a byte.  Not every way of writing a helper passes it: these take their
// operands by reference where that is what keeps the code identical, and the
// fragment offsets, accumulator zeroing and C stores of the tile functions
// are not here because no shared form of them passed.
#pragma once
#include "cek_kernel.h"

// K-tile index of a stage load of the K-split that starts at K-tile ks;
// tools/microbench/gemm_loop.hip redefines it to re-read two K-tiles (an
// L2-resident operand stream) as a probe.
#ifndef CEK_KTILE
#define CEK_KTILE(ks, kt) ((ks) + (kt))
#endif

// Tile t of an ntm × ntn tile grid (dims[6]: the shell order's P): its
// coordinates in the grouped (or shell) order.  False for a surplus
// work-group: a launch wider than the tile grid (a host-side range error)
// must not read or write past A, B or C, so such a work-group leaves at once.
__device__ __forceinline__ bool cek_tile_lookup(const int* __restrict__ dims, int GM, long long t, int ntm, int ntn, int& tm,
                                                int& tn) {
  if (t >= (long long)ntm * ntn) return false;
  cek_tile_coords(t, ntm, ntn, GM, dims[6], tm, tn);
  return true;
}

// Staging: instruction `ins` of a wave fills LDS bytes [ins·1 KiB, +1 KiB)
// = 8 rows × 128 B; lane l lands at row ins·8 + l/8, physical chunk l%8,
// which holds logical chunk (l%8) ^ (row & 7).  Within one wave instruction
// the 8 rows are ins·8 .. ins·8+7, so the logical chunk (l%8) ^ (l/8) is the
// same for every instruction: one per-lane 32-bit byte offset (returned
// here) plus a wave-uniform 64-bit base (saddr form).
template <int ESZ>
__device__ __forceinline__ unsigned cek_stage_lane_off(int lane, int K) {
  const int lrow = lane >> 3, lchunk = (lane & 7) ^ (lrow & 7);
  return (unsigned)(lrow * K + lchunk * (16 / ESZ)) * (unsigned)ESZ;
}

// The issue loop: N row blocks of 1 KiB, global → LDS, by staging wave w of
// an operand whose waves take PER blocks each.  Block j (j0 ≤ j < j0 + N) is
// rows [8j, 8j + 8) below `rows` (row pitch K elements) at K-tile `ktile`,
// and lands at lds + (w·PER + j) KiB.
// The operands come by reference on purpose: as in a lambda that captures by
// reference, the compiler then sees them as loop-invariant only after the
// loop is unrolled.  What it emits (gfx950, -O3): the saddr form
// (global_load_lds_dwordx4 vOFF, s[BASE:BASE+1]) only where the lane offset's
// zero-extension sits in the block of the load, which is the prologues and
// some MODE 0 / 2 loops; inside the ping-pong K loops the zero-extension is
// hoisted out, and every load takes a 64-bit VGPR address made by one
// v_lshl_add_u64 (uniform base + extended offset) in front of it.  The flat
// loops of sgemm_bf16.hip (FLAT 2) form the offset again inside the loop and
// get the saddr form there; the byte-identity of the other kernels is why
// this helper is left as it is.
template <int N, int ESZ, int PER = N>
__device__ __forceinline__ void cek_stage_rows(const char* const& rows, const unsigned& lane_off, const int& K,
                                               const int& ks, const int& kt, char* lds, const int& w, int j0 = 0) {
  constexpr int BK = 128 / ESZ;
#pragma unroll
  for (int j = j0; j < j0 + N; ++j) {
    const char* src = rows + ((size_t)j * 8 * K + (size_t)CEK_KTILE(ks, kt) * BK) * ESZ;
    __builtin_amdgcn_global_load_lds((glb_cvoid*)(src + lane_off), (lds_void*)(lds + (w * PER + j) * 1024), 16, 0, 0);
  }
}
