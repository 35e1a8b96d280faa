// The tile function of the GEMMs whose operands are staged as bytes:
// sgemm_fp8.hip (plain e4m3fn), sgemm_mxfp8.hip (e4m3fn with E8M0 block
// scales), sgemm_mxfp4.hip (e2m1, two per byte) and sgemm_mxf8f4.hip (e4m3fn
// A against e2m1 Bt).  A kernel states the element format of each operand
// and how the sum over k is issued; byte geometry, staging and the ping-pong
// structure are written once here and follow from those three, and the
// kernel-definition macros of the six files are at the end.  sgemm_fp8.hip's
// device code is byte-identical to what it was when this function lived in
// that file (tools/kernel_identity.py).
#pragma once
#include "gemm8_out.h"
#include "gemm_parts.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef long i64x2 __attribute__((ext_vector_type(2)));

namespace {

// Element format of an operand: the format selector (cbsz / blgp) of
// v_mfma_scale_f32_16x16x128_f8f6f4, as the instruction numbers it.
enum : int { GEMM8_E4M3 = 0, GEMM8_E2M1 = 4 };
// How the sum over k is issued: four non-scaled 16x16x32 steps per K-tile,
// the scaled instruction with every scale 2^0, or with MX block scales.
enum : int { GEMM8_K32, GEMM8_UNIT, GEMM8_MX };

// What follows from the formats.  Bt's K-tile is always one LDS row of 128 B,
// so a K-tile is 1024 / bits(Bt) k (128 for e4m3, 256 for e2m1: STEPS = 1 or 2
// scaled instructions of 128 k), an operand's row pitch is K·bits/8 bytes, and
// A's K-tile is bits(A) / bits(Bt) sub-tiles [BM][128] of 128-B rows: one,
// or two for e4m3 A against e2m1 Bt, sub-tile h staged as A's byte K-tile
// subs·kt + h.  A lane's 16-B reads of an operand's K-tile are numbered in k
// order, two per sub-tile, and a step takes bits / 4 of them: an e4m3 operand
// two (32 B, registers 0-3 and 4-7), an e2m1 operand one (16 B).
constexpr int gemm8_bits(int fmt) { return fmt == GEMM8_E2M1 ? 4 : 8; }
constexpr int gemm8_a_subs(int fa, int fb) { return gemm8_bits(fa) / gemm8_bits(fb); }

// LDS bytes of a tile.  MODE 0: two whole stages (A rows, then Bt rows).
// MODE 4: two A buffers and three Bt buffers.
constexpr int gemm8_lds_bytes(int WM, int WN, int FM, int FN, int MODE, int FA, int FB) {
  const int a = WM * 16 * FM * 128 * gemm8_a_subs(FA, FB), b = WN * 16 * FN * 128;
  return MODE == 4 ? 2 * a + 3 * b : 2 * (a + b);
}

// The 32-B operand of the scaled instruction from its low and high 16 B.  An
// e2m1 operand has no high half: the instruction takes the low four registers
// and ignores the rest.
template <int FMT>
__device__ __forceinline__ i32x8 gemm8_operand(i32x4 lo, i32x4 hi) {
  if constexpr (FMT == GEMM8_E2M1)
    return __builtin_shufflevector(lo, lo, 0, 1, 2, 3, -1, -1, -1, -1);
  else
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// f(cek_int<I>{}) for I = 0 .. N-1: an index the callee can use where the
// compiler wants an immediate (the op_sel of the scaled MFMA)
template <int V>
struct cek_int {
  static constexpr int value = V;
};
template <int I, int N, class F>
__device__ __forceinline__ void cek_static_for(F&& f) {
  if constexpr (I < N) {
    f(cek_int<I>{});
    cek_static_for<I + 1, N>(f);
  }
}

// MODE 0: one LDS stage in flight, all waves stage, one barrier per K-tile.
// MODE 4: ping-pong wave groups with balanced DMA (G0 = waves < NWAVES/2
// stages A one K-tile ahead, G1 stages Bt two K-tiles ahead), the structure
// and the hazard reasoning of sgemm_bf16.hip's MODE 4.
// SCALE: GEMM8_K32, GEMM8_UNIT or GEMM8_MX.  GEMM8_MX: block scales
// (sgemm_mxfp8.hip has the map, the packed scale layout and the vmcnt
// argument); SAp / SBp are the packed scales, unused otherwise.
// FA, FB: the element formats of A and Bt.  e2m1 Bt (sgemm_mxfp4.hip): the row
// pitch is K/2 bytes and a K-tile of 128 B holds 256 k: two scaled
// instructions per fragment pair, step s on the 16 B of read s with the scales
// of 128-k step 2·kt + s.  Everything written in bytes stays as it is.
// e4m3 A against it (sgemm_mxf8f4.hip): A's row pitch is K bytes and its
// K-tile of 256 k two sub-tiles; step s multiplies the two 16-B reads of
// sub-tile s (the MXFP8 operand of that 128-k step) by the 16 B of Bt's read s.
// OUT: what is stored.  GEMM8_OUT_F32 (the default): C as fp32, tile-major in
// fragment order.  Otherwise (gemm8_out.h) `C` points to the row-major [M][N]
// output in that mode's format, `SY` to its row-major scale bytes (MX modes)
// and dims[5] selects the activation (0: none, 1: ReLU), a word the other
// kernels do not read.  Nothing above the store depends on OUT, so the
// accumulators are those of the plain kernel with the same tile.
template <int WM, int WN, int FM, int FN, int MODE, int SCALE, int FA, int FB, int OUT = GEMM8_OUT_F32>
__device__ __forceinline__ void gemm8_tile(const int* __restrict__ dims, const uint8_t* __restrict__ A,
                                           const uint8_t* __restrict__ Bt, float* __restrict__ C, char* smem,
                                           long long off, const int* __restrict__ SAp = nullptr,
                                           const int* __restrict__ SBp = nullptr,
                                           uint8_t* __restrict__ SY = nullptr) {
  static_assert(MODE == 0 || MODE == 4, "MODE is 0 or 4");
  constexpr bool MX = SCALE == GEMM8_MX;
  static_assert((FA == GEMM8_E4M3 || FA == GEMM8_E2M1) && (FB == GEMM8_E4M3 || FB == GEMM8_E2M1) &&
                    (FA == FB || (FA == GEMM8_E4M3 && FB == GEMM8_E2M1)),
                "formats: equal, or e4m3 A against e2m1 Bt");
  static_assert(FB == GEMM8_E4M3 || MX, "e2m1: block-scaled only");
  static_assert(SCALE == GEMM8_UNIT || MX || (SCALE == GEMM8_K32 && FA == GEMM8_E4M3 && FB == GEMM8_E4M3),
                "the non-scaled steps: e4m3 x e4m3 only");
  static_assert(!MX || (FM % 4 == 0 && FN % 4 == 0), "MX: 64-row scale groups");
  constexpr int BM = WM * 16 * FM, BN = WN * 16 * FN, BK = 128;
  constexpr int NWAVES = WM * WN, NT = 64 * NWAVES;
  constexpr int A_SUBS = gemm8_a_subs(FA, FB), STEPS = 8 / gemm8_bits(FB);
  constexpr int RA = gemm8_bits(FA) / 4, RB = gemm8_bits(FB) / 4;  // 16-B reads of one step's operand
  constexpr int A_SUB = BM * BK;  // one 128-B sub-tile of A
  constexpr int A_BYTES = A_SUB * A_SUBS, B_BYTES = BN * BK, STAGE = A_BYTES + B_BYTES;
  constexpr int STAGERS = MODE == 4 ? NWAVES / 2 : NWAVES;
  constexpr int A_INSTR = A_SUB / 1024 / STAGERS;  // per sub-tile
  constexpr int B_INSTR = B_BYTES / 1024 / STAGERS;

  const int M = dims[0], N = dims[1], K = dims[2], GM = dims[3] > 0 ? dims[3] : 1;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave / WN, wc = wave % WN;
  const long long t = (long long)cek_xcd_remap(blockIdx.x, gridDim.x) + off / NT;
  const int ntn = N / BN, ntm = M / BM;
  int tm, tn;
  if (!cek_tile_lookup(dims, GM, t, ntm, ntn, tm, tn)) return;
  const int m0 = tm * BM, n0 = tn * BN;
  const int KA = K / (8 / gemm8_bits(FA)), KB = K / (8 / gemm8_bits(FB));  // row pitches in bytes
  const int nk = KB / BK, ks = 0;

  // ---- staging (geometry: gemm_parts.h) ----
  const unsigned lane_off_b = cek_stage_lane_off<1>(lane, KB), lane_off_a = cek_stage_lane_off<1>(lane, KA);
  const int sw = MODE == 4 ? wave % (NWAVES / 2) : wave;  // staging wave index
  const char* a_wave = (const char*)(A + (size_t)(m0 + sw * A_INSTR * 8) * KA);
  const char* b_wave = (const char*)(Bt + (size_t)(n0 + sw * B_INSTR * 8) * KB);
  // A's K-tile kt to `dst`: its sub-tiles, A's byte K-tiles A_SUBS·kt + h
  auto stage_a = [&](int kt, char* dst) {
#pragma unroll
    for (int h = 0; h < A_SUBS; ++h) {
      const int kb = A_SUBS * kt + h;
      cek_stage_rows<A_INSTR, 1>(a_wave, lane_off_a, KA, ks, kb, dst + h * A_SUB, sw);
    }
  };
  // MODE 0: K-tile kt into whole stage `buf` (A rows, then Bt rows)
  auto stage = [&](int buf, int kt) {
    stage_a(kt, smem + buf * STAGE);
    cek_stage_rows<B_INSTR, 1>(b_wave, lane_off_b, KB, ks, kt, smem + buf * STAGE + A_BYTES, sw);
  };
  // MODE 4: two A buffers followed by three Bt buffers
  char* const a_base = smem;
  char* const b_base = smem + 2 * A_BYTES;
  auto stage_a4 = [&](int kt) { stage_a(kt, a_base + (kt & 1) * A_BYTES); };
  auto stage_b4 = [&](int kt) {
    cek_stage_rows<B_INSTR, 1>(b_wave, lane_off_b, KB, ks, kt, b_base + (kt % 3) * B_BYTES, sw);
  };

  // Fragment read offsets (bytes) inside a stage: row (wr·16FM + i·16 + l%16),
  // logical chunk s·4 + l/16, physical = logical ^ (l & 7).  (MX: the same
  // map; sgemm_mxfp8.hip says which scale meets which chunk.)  a_off is the
  // offset inside a sub-tile of A.
  const int fr = lane & 15, fq = lane >> 4;
  int a_off[2], b_off[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int pc = (s * 4 + fq) ^ (lane & 7);
    a_off[s] = (wr * 16 * FM + fr) * 128 + pc * 16;
    b_off[s] = A_BYTES + (wc * 16 * FN + fr) * 128 + pc * 16;
  }

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // MX: packed scales of this wave's fragments, global → VGPR.  Dword d of A
  // holds fragments 4d .. 4d+3 (byte i & 3) for this lane's (row fr, MX block
  // fq); `sa` / `sb` are those of the K-tile being multiplied, `sa_n` / `sb_n`
  // the prefetch of the next one.
  // Two steps: the dwords of step 0, then those of step 1 (index s · F/4 + d).
  constexpr int SA_G = MX ? FM / 4 : 1, SB_G = MX ? FN / 4 : 1;
  constexpr int SA_N = SA_G * STEPS, SB_N = SB_G * STEPS;
  int sa[SA_N], sb[SB_N], sa_n[SA_N], sb_n[SB_N];
  // The loads are inline assembly on purpose.  A load the compiler knows of
  // makes it guard the scale registers with a wait of its own, and among the
  // LDS-DMA staging loads it does not count: it puts `s_waitcnt vmcnt(0)` in
  // front of the MFMA section, where G1 would wait for Bt k+2 and G0 for A
  // k+1.  Written this way the only waits are the loop's own: next_scales()
  // follows one of them in every path, and its empty asm ties the prefetch
  // registers to that place so that no copy can move ahead of the wait.
  // ld_scales is called for kt = 0, 1, .. nk in turn.  The two pointers stand
  // at K-tile min(kt, nk − 1) of this wave's scale groups — the prefetch past
  // the end re-reads the last K-tile, so every iteration issues the same
  // number of loads and none is out of bounds — and step one K-tile (M and N
  // dwords) per call while there is one, instead of being recomputed: the
  // 64-bit multiplies would sit ahead of the staging issue in every iteration.
  // Two steps: a K-tile is two 128-k steps, M (N) dwords apart; the pointers step both.
  const int lane4 = lane * 4;
  const int* pa = SAp + (MX ? (m0 + wr * 16 * FM) / 64 * 64 : 0);
  const int* pb = SBp + (MX ? (n0 + wc * 16 * FN) / 64 * 64 : 0);
  auto ld_scales = [&](int kt) {
#pragma unroll
    for (int d = 0; d < SA_N; ++d)
      asm volatile("global_load_dword %0, %1, %2"
                   : "=v"(sa_n[d])
                   : "v"(lane4), "s"(pa + (d / SA_G) * M + (d % SA_G) * 64)
                   : "memory");
#pragma unroll
    for (int d = 0; d < SB_N; ++d)
      asm volatile("global_load_dword %0, %1, %2"
                   : "=v"(sb_n[d])
                   : "v"(lane4), "s"(pb + (d / SB_G) * N + (d % SB_G) * 64)
                   : "memory");
    const bool more = kt + 1 < nk;
    pa += more ? STEPS * M : 0;
    pb += more ? STEPS * N : 0;
  };
  // after a vmcnt wait that covers the prefetch: the prefetch becomes current
  auto next_scales = [&] {
#pragma unroll
    for (int d = 0; d < SA_N; ++d) {
      asm volatile("" : "+v"(sa_n[d]));
      sa[d] = sa_n[d];
    }
#pragma unroll
    for (int d = 0; d < SB_N; ++d) {
      asm volatile("" : "+v"(sb_n[d]));
      sb[d] = sb_n[d];
    }
  };

  // A lane's 16-B reads of a K-tile, in k order: two of Bt, 2·A_SUBS of A.
  i32x4 fa[2 * A_SUBS][FM], fb[2][FN];
  // Half s of the K-tile: read s of Bt and reads A_SUBS·s + h of A, A rows
  // from ab, Bt rows from bb (b_off includes A_BYTES).  Read r of A is read
  // r % 2 of sub-tile r / 2: with one sub-tile read s of it, with two read h of
  // sub-tile s.  Both are written as multiples of s, because the compiler
  // meets a division before it knows s and then orders the address sums
  // differently.
  auto ld = [&](int s, const char* ab, const char* bb) {
#pragma unroll
    for (int j = 0; j < FN; ++j) fb[s][j] = *(const i32x4*)(bb + b_off[s] + j * 2048);
#pragma unroll
    for (int ih = 0; ih < FM * A_SUBS; ++ih) {  // fragment i, then its reads
      const int i = ih / A_SUBS, h = ih % A_SUBS;
      const int sub = (A_SUBS - 1) * s, rd = (2 - A_SUBS) * s + h;
      fa[A_SUBS * s + h][i] = *(const i32x4*)(ab + sub * A_SUB + a_off[rd] + i * 2048);
    }
  };
  // the two 16x16x32 steps of k block s: the low, then the high 8 B of the read
  auto mma = [&](int s) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(__builtin_bit_cast(i64x2, fa[s][i])[h],
                                                                 __builtin_bit_cast(i64x2, fb[s][j])[h], acc[i][j], 0,
                                                                 0, 0);
  };
  // The scaled instruction, STEPS steps of 128 k per fragment pair.  Step s
  // takes reads R·s .. R·s + R − 1 of each operand as its low and high 16 B
  // (e4m3: k blocks 0 and 1 of its 128 B; e2m1: the one read).  The scales are
  // the lane's bytes of step s, picked by op_sel = fragment & 3 (MX), or every
  // scale byte 127 = 2^0.  Step 0 runs over every fragment pair before step 1,
  // so that the two instructions on one accumulator are FM·FN issues apart.
  auto mma_scaled = [&] {
    cek_static_for<0, STEPS>([&](auto sc) {
      cek_static_for<0, FM>([&](auto ic) {
        cek_static_for<0, FN>([&](auto jc) {
          constexpr int s = decltype(sc)::value, i = decltype(ic)::value, j = decltype(jc)::value;
          constexpr int ONE = 0x7F7F7F7F;
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              gemm8_operand<FA>(fa[RA * s][i], fa[RA * s + RA - 1][i]),
              gemm8_operand<FB>(fb[RB * s][j], fb[RB * s + RB - 1][j]), acc[i][j], FA, FB, MX ? i & 3 : 0,
              MX ? sa[s * SA_G + i / 4] : ONE, MX ? j & 3 : 0, MX ? sb[s * SB_G + j / 4] : ONE);
        });
      });
    });
  };
  auto mmaall = [&] {
    __builtin_amdgcn_s_setprio(1);
    if constexpr (SCALE != GEMM8_K32) {
      mma_scaled();
    } else {
#pragma unroll
      for (int s = 0; s < 2; ++s) mma(s);
    }
    // Pin the MFMAs here: left alone, the compiler sinks the 32 scaled MFMAs
    // below the caller's s_setprio(0) and vmcnt(0), and G0 then waits for its
    // staging before its matrix section instead of behind it.
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) asm volatile("" : "+v"(acc[i][j]));
    __builtin_amdgcn_s_setprio(0);
  };
  auto bar = [] {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };

  if constexpr (MODE == 0) {
    if constexpr (MX) ld_scales(0);
    stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (MX) next_scales();
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      if constexpr (MX) ld_scales(kt + 1);
      if (kt + 1 < nk) stage(cur ^ 1, kt + 1);
      const char* base = smem + cur * STAGE;
      if constexpr (SCALE != GEMM8_K32) {
        ld(0, base, base);
        ld(1, base, base);
        mmaall();
      } else {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          ld(s, base, base);
          __builtin_amdgcn_s_setprio(1);
          mma(s);
          __builtin_amdgcn_s_setprio(0);
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if constexpr (MX) next_scales();
      __syncthreads();
    }
  } else {
    // Ping-pong (sgemm_bf16.hip, MODE 4): between two block barriers one
    // group runs the MFMAs of K-tile k while the other reads its fragments.
    //   WAR: both staging targets were last read in the previous read sections.
    //   RAW: G0's vmcnt(0) closes its MFMA section (A k+1 before G0 reads it);
    //        G1 ends its read section k with Bt k+1 retired (only k+2 in flight).
    // MX: the scale loads of K-tile k+1 are issued at the top of iteration k,
    // AHEAD of that iteration's staging, so they are older than every staging
    // operation the counted wait leaves in flight (sgemm_mxfp8.hip).
    const bool g1 = wave >= NWAVES / 2;
    if constexpr (MX) ld_scales(0);
    if (!g1) {
      stage_a4(0);
    } else {
      stage_b4(0);
      if (nk > 1) stage_b4(1);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (MX) next_scales();
    bar();
    if (g1) bar();  // G1 runs one section behind
    for (int kt = 0; kt < nk; ++kt) {
      const bool g1_issued = g1 && kt + 2 < nk;
      if constexpr (MX) {
        ld_scales(kt + 1);
        __builtin_amdgcn_sched_barrier(0);  // the scale loads stay ahead of the staging
      }
      if (!g1) {
        if (kt + 1 < nk) stage_a4(kt + 1);
      } else if (g1_issued) {
        stage_b4(kt + 2);
      }
      const char* ab = a_base + (kt & 1) * A_BYTES;
      const char* bb = b_base + (kt % 3) * B_BYTES - A_BYTES;
      ld(0, ab, bb);
      ld(1, ab, bb);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (g1) {
        if (g1_issued)
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(B_INSTR) : "memory");
        else
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      bar();
      mmaall();
      if (!g1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if constexpr (MX) next_scales();
      bar();
    }
    if (!g1) bar();  // equal barrier counts for both groups
  }

  if constexpr (OUT != GEMM8_OUT_F32) {
    __syncthreads();  // every wave is done with the operand stages: LDS is free
    gemm8_store_out<FM, FN, OUT>(acc, smem, C, SY, N, dims[5] == 1, m0 + wr * 16 * FM, n0 + wc * 16 * FN, wave,
                                 lane);
    return;
  }
  // C tile in fragment order (sgemm_bf16.hip): acc[i][j][r] is
  // C(row = wr·16FM + i·16 + fq·4 + r, col = wc·16FN + j·16 + fr), stored at
  // ((((wr·WN + wc)·FM + i)·FN + j)·64 + lane)·4 + r of the tile.
  f32x4* ct = reinterpret_cast<f32x4*>(C + (size_t)t * BM * BN);
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) ct[(((wr * WN + wc) * FM + i) * FN + j) * 64 + lane] = acc[i][j];
}

}  // namespace

// The kernels of the six files: tile numbers, then the operand formats.
// Plain (four arrays: dims, A, Bt, C; SCALE is GEMM8_K32 or GEMM8_UNIT):
#define CEK_GEMM8_KERNEL(NAME, WM, WN, FM, FN, MODE, SCALE, FA, FB)                                             \
  extern "C" __global__ __launch_bounds__(64 * WM * WN) void NAME(const int* dims, const uint8_t* A,            \
                                                                    const uint8_t* Bt, float* C, CEK_HIDDEN) {    \
    __shared__ __attribute__((aligned(16))) char smem[gemm8_lds_bytes(WM, WN, FM, FN, MODE, FA, FB)];            \
    gemm8_tile<WM, WN, FM, FN, MODE, SCALE, FA, FB>(dims, A, Bt, C, smem, __cek_off);                            \
  }
// MX (six arrays: dims, A, Bt, SAp, SBp, C):
#define CEK_GEMM8_MX_KERNEL(NAME, WM, WN, FM, FN, MODE, FA, FB)                                                 \
  extern "C" __global__ __launch_bounds__(64 * WM * WN) void NAME(const int* dims, const uint8_t* A,            \
                                                                    const uint8_t* Bt, const int* SAp,            \
                                                                    const int* SBp, float* C, CEK_HIDDEN) {       \
    __shared__ __attribute__((aligned(16))) char smem[gemm8_lds_bytes(WM, WN, FM, FN, MODE, FA, FB)];            \
    gemm8_tile<WM, WN, FM, FN, MODE, GEMM8_MX, FA, FB>(dims, A, Bt, C, smem, __cek_off, SAp, SBp);               \
  }
// MX with an output mode (dims, A, Bt, SAp, SBp, Y and, with HAS_SY = 1, SY):
#define CEK_SY_PARAMS_0
#define CEK_SY_PARAMS_1 uint8_t *SY,
#define CEK_SY_ARG_0 nullptr
#define CEK_SY_ARG_1 SY
#define CEK_GEMM8_MX_OUT_KERNEL(NAME, WM, WN, FM, FN, MODE, FA, FB, OUT, HAS_SY)                                \
  extern "C" __global__ __launch_bounds__(64 * WM * WN) void NAME(                                               \
      const int* dims, const uint8_t* A, const uint8_t* Bt, const int* SAp, const int* SBp, uint8_t* Y,          \
      CEK_SY_PARAMS_##HAS_SY CEK_HIDDEN) {                                                                        \
    __shared__ __attribute__((aligned(16))) char smem[gemm8_lds_bytes(WM, WN, FM, FN, MODE, FA, FB)];            \
    gemm8_tile<WM, WN, FM, FN, MODE, GEMM8_MX, FA, FB, OUT>(dims, A, Bt, reinterpret_cast<float*>(Y), smem,      \
                                                            __cek_off, SAp, SBp, CEK_SY_ARG_##HAS_SY);           \
  }
// the three outputs of one tile
#define CEK_GEMM8_MX_OUT_TILE(STEM, WM, WN, FM, FN, MODE, FA, FB)                               \
  CEK_GEMM8_MX_OUT_KERNEL(STEM##_bf16, WM, WN, FM, FN, MODE, FA, FB, GEMM8_OUT_BF16, 0)         \
  CEK_GEMM8_MX_OUT_KERNEL(STEM##_mxfp8, WM, WN, FM, FN, MODE, FA, FB, GEMM8_OUT_MXFP8, 1)       \
  CEK_GEMM8_MX_OUT_KERNEL(STEM##_mxfp4, WM, WN, FM, FN, MODE, FA, FB, GEMM8_OUT_MXFP4, 1)
