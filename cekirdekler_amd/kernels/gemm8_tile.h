// The tile function of the GEMMs whose operands are staged as bytes:
// sgemm_fp8.hip (plain e4m3fn), sgemm_mxfp8.hip (e4m3fn with E8M0 block
// scales, MX = true), sgemm_mxfp4.hip (e2m1, two per byte, F4 = true) and
// sgemm_mxf8f4.hip (e4m3fn A against e2m1 Bt, F4 and A8 = true).
// Byte geometry, staging and the ping-pong structure are written once here;
// the two fp8 files differ in the scale operands of the 16x16x128 instruction
// (and the loads that feed them) and in nothing else, and the 4-bit one in
// what F4 says below.  sgemm_fp8.hip's device code is
// byte-identical to what it was when this function lived in that file
// (tools/kernel_identity.py).
#pragma once
#include "gemm8_out.h"
#include "gemm_parts.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef long i64x2 __attribute__((ext_vector_type(2)));

namespace {

// LDS bytes of a tile.  MODE 0: two whole stages (A rows, then Bt rows).
// MODE 4: two A buffers and three Bt buffers.  A8: A's K-tile is two 128-B
// sub-tiles.
constexpr int gemm8_lds_bytes(int WM, int WN, int FM, int FN, int MODE, bool A8 = false) {
  const int a = WM * 16 * FM * 128 * (A8 ? 2 : 1), b = WN * 16 * FN * 128;
  return MODE == 4 ? 2 * a + 3 * b : 2 * (a + b);
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
// X128: the scaled 16x16x128 instruction instead of four 16x16x32 steps.
// MX: block scales (sgemm_mxfp8.hip has the map, the packed scale layout and
// the vmcnt argument); SAp / SBp are the packed scales, unused otherwise.
// F4: e2m1 operands, two per byte (sgemm_mxfp4.hip).  The row pitch is K/2
// bytes and a K-tile of 128 B holds 256 k: two scaled instructions per
// fragment pair, step s on the 16 B of read s with the scales of 128-k step
// 2·kt + s.  Everything written in bytes stays as it is.
// A8 (with F4): A alone is e4m3fn, one element per byte (sgemm_mxf8f4.hip).
// Bt, its staging and both scale arrays are F4's.  A's row pitch is K bytes
// and its K-tile of 256 k two 128-B sub-tiles [2][BM][128], sub-tile h staged
// as byte K-tile 2·kt + h; step s multiplies the two 16-B reads of sub-tile s
// (the MXFP8 operand of that 128-k step) by the 16 B of Bt's read s.
// OUT: what is stored.  GEMM8_OUT_F32 (the default): C as fp32, tile-major in
// fragment order.  Otherwise (gemm8_out.h) `C` points to the row-major [M][N]
// output in that mode's format, `SY` to its row-major scale bytes (MX modes)
// and dims[5] selects the activation (0: none, 1: ReLU), a word the other
// kernels do not read.  Nothing above the store depends on OUT, so the
// accumulators are those of the plain kernel with the same tile.
template <int WM, int WN, int FM, int FN, int MODE, bool X128, bool MX = false, bool F4 = false,
          int OUT = GEMM8_OUT_F32, bool A8 = false>
__device__ __forceinline__ void gemm8_tile(const int* __restrict__ dims, const uint8_t* __restrict__ A,
                                           const uint8_t* __restrict__ Bt, float* __restrict__ C, char* smem,
                                           long long off, const int* __restrict__ SAp = nullptr,
                                           const int* __restrict__ SBp = nullptr,
                                           uint8_t* __restrict__ SY = nullptr) {
  static_assert(MODE == 0 || MODE == 4, "MODE is 0 or 4");
  static_assert(!MX || (X128 && FM % 4 == 0 && FN % 4 == 0), "MX: scaled instruction, 64-row scale groups");
  static_assert(!F4 || MX, "F4: block-scaled only");
  static_assert(!A8 || F4, "A8: e4m3 A against e2m1 Bt");
  constexpr int BM = WM * 16 * FM, BN = WN * 16 * FN, BK = 128;
  constexpr int NWAVES = WM * WN, NT = 64 * NWAVES;
  constexpr int A_SUB = BM * BK;  // one 128-B sub-tile of A (A8: two per K-tile)
  constexpr int A_BYTES = A_SUB * (A8 ? 2 : 1), B_BYTES = BN * BK, STAGE = A_BYTES + B_BYTES;
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
  const int KB = F4 ? K / 2 : K;  // row pitch in bytes
  const int KA = A8 ? K : KB;     // A's, where it differs
  const int nk = KB / BK, ks = 0;

  // ---- staging (geometry: gemm_parts.h) ----
  const unsigned lane_off = cek_stage_lane_off<1>(lane, KB);
  const unsigned lane_off_a = A8 ? cek_stage_lane_off<1>(lane, KA) : lane_off;
  const int sw = MODE == 4 ? wave % (NWAVES / 2) : wave;  // staging wave index
  const char* a_wave = (const char*)(A + (size_t)(m0 + sw * A_INSTR * 8) * KA);
  const char* b_wave = (const char*)(Bt + (size_t)(n0 + sw * B_INSTR * 8) * KB);
  // A's K-tile kt to `dst` (A8: its two sub-tiles, byte K-tiles 2·kt and 2·kt + 1)
  auto stage_a = [&](int kt, char* dst) {
    if constexpr (A8) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int kb = 2 * kt + h;
        cek_stage_rows<A_INSTR, 1>(a_wave, lane_off_a, KA, ks, kb, dst + h * A_SUB, sw);
      }
    } else {
      cek_stage_rows<A_INSTR, 1>(a_wave, lane_off, KB, ks, kt, dst, sw);
    }
  };
  // MODE 0: K-tile kt into whole stage `buf` (A rows, then Bt rows)
  auto stage = [&](int buf, int kt) {
    stage_a(kt, smem + buf * STAGE);
    cek_stage_rows<B_INSTR, 1>(b_wave, lane_off, KB, ks, kt, smem + buf * STAGE + A_BYTES, sw);
  };
  // MODE 4: two A buffers followed by three Bt buffers
  char* const a_base = smem;
  char* const b_base = smem + 2 * A_BYTES;
  auto stage_a4 = [&](int kt) { stage_a(kt, a_base + (kt & 1) * A_BYTES); };
  auto stage_b4 = [&](int kt) {
    cek_stage_rows<B_INSTR, 1>(b_wave, lane_off, KB, ks, kt, b_base + (kt % 3) * B_BYTES, sw);
  };

  // Fragment read offsets (bytes) inside a stage: row (wr·16FM + i·16 + l%16),
  // logical chunk s·4 + l/16, physical = logical ^ (l & 7).  (MX: the same
  // map; sgemm_mxfp8.hip says which scale meets which chunk.)
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
  // F4: the dwords of step 0, then those of step 1 (index s · F/4 + d).
  constexpr int SA_G = MX ? FM / 4 : 1, SB_G = MX ? FN / 4 : 1, STEPS = F4 ? 2 : 1;
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
  // F4: a K-tile is two 128-k steps, M (N) dwords apart; the pointers step both.
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

  i32x4 fa[2][FM], fb[2][FN];
  i32x4 fah[2][FM];  // A8: the high 16 B of step s's A operand (fa[s]: the low)
  // k block s of a K-tile: A rows from ab, Bt rows from bb (b_off includes A_BYTES)
  // A8: step s, A's two reads inside sub-tile s
  auto ld = [&](int s, const char* ab, const char* bb) {
#pragma unroll
    for (int j = 0; j < FN; ++j) fb[s][j] = *(const i32x4*)(bb + b_off[s] + j * 2048);
    if constexpr (A8) {
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        fa[s][i] = *(const i32x4*)(ab + s * A_SUB + a_off[0] + i * 2048);
        fah[s][i] = *(const i32x4*)(ab + s * A_SUB + a_off[1] + i * 2048);
      }
    } else {
#pragma unroll
      for (int i = 0; i < FM; ++i) fa[s][i] = *(const i32x4*)(ab + a_off[s] + i * 2048);
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
  // the whole K-tile in one scaled instruction per fragment pair: k blocks 0
  // and 1 are the low and high 16 B of the 32-B operand; formats 0 = e4m3,
  // every scale byte 127 = 2^0
  auto mma128 = [&] {
    constexpr int ONE = 0x7F7F7F7F;
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            __builtin_shufflevector(fa[0][i], fa[1][i], 0, 1, 2, 3, 4, 5, 6, 7),
            __builtin_shufflevector(fb[0][j], fb[1][j], 0, 1, 2, 3, 4, 5, 6, 7), acc[i][j], 0, 0, 0, ONE, 0, ONE);
  };
  // MX: the same with the lane's scale bytes, picked by op_sel = fragment & 3
  auto mma128mx = [&] {
    cek_static_for<0, FM>([&](auto ic) {
      cek_static_for<0, FN>([&](auto jc) {
        constexpr int i = decltype(ic)::value, j = decltype(jc)::value;
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            __builtin_shufflevector(fa[0][i], fa[1][i], 0, 1, 2, 3, 4, 5, 6, 7),
            __builtin_shufflevector(fb[0][j], fb[1][j], 0, 1, 2, 3, 4, 5, 6, 7), acc[i][j], 0, 0, i & 3, sa[i / 4],
            j & 3, sb[j / 4]);
      });
    });
  };
  // F4: two steps of 128 k, each the 16 B of one read (formats 4 = e2m1: the
  // instruction takes the low four registers of the operand and ignores the
  // rest), step 0 over every fragment pair before step 1, so that the two
  // instructions on one accumulator are FM·FN issues apart
  auto mma128f4 = [&] {
    cek_static_for<0, 2>([&](auto sc) {
      cek_static_for<0, FM>([&](auto ic) {
        cek_static_for<0, FN>([&](auto jc) {
          constexpr int s = decltype(sc)::value, i = decltype(ic)::value, j = decltype(jc)::value;
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              __builtin_shufflevector(fa[s][i], fa[s][i], 0, 1, 2, 3, -1, -1, -1, -1),
              __builtin_shufflevector(fb[s][j], fb[s][j], 0, 1, 2, 3, -1, -1, -1, -1), acc[i][j], 4, 4, i & 3,
              sa[s * SA_G + i / 4], j & 3, sb[s * SB_G + j / 4]);
        });
      });
    });
  };
  // A8: the same two steps with A's 32-B e4m3 operand (format 0) against
  // Bt's 16 B of e2m1 (format 4), in mma128f4's issue order
  auto mma128f8f4 = [&] {
    cek_static_for<0, 2>([&](auto sc) {
      cek_static_for<0, FM>([&](auto ic) {
        cek_static_for<0, FN>([&](auto jc) {
          constexpr int s = decltype(sc)::value, i = decltype(ic)::value, j = decltype(jc)::value;
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              __builtin_shufflevector(fa[s][i], fah[s][i], 0, 1, 2, 3, 4, 5, 6, 7),
              __builtin_shufflevector(fb[s][j], fb[s][j], 0, 1, 2, 3, -1, -1, -1, -1), acc[i][j], 0, 4, i & 3,
              sa[s * SA_G + i / 4], j & 3, sb[s * SB_G + j / 4]);
        });
      });
    });
  };
  auto mmaall = [&] {
    __builtin_amdgcn_s_setprio(1);
    if constexpr (A8) {
      mma128f8f4();
    } else if constexpr (F4) {
      mma128f4();
    } else if constexpr (MX) {
      mma128mx();
    } else if constexpr (X128) {
      mma128();
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
      if constexpr (X128) {
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
