"""Cases for the mixed MXFP8 × MXFP4 GEMM (kernels/sgemm_mxf8f4.hip,
gemm8_tile.h with e4m3 A and e2m1 Bt, ops.gemm.GemmMxFp8Fp4), in the manner of
gemm4_oracles.py: the shapes, the exact data, a numpy emulation of the tile
under the hypothesised read maps, the scale-mapping probe with its wrong maps,
and the single-instruction probe of v_mfma_scale_f32_16x16x128_f8f6f4 with an
e4m3 A (cbsz = 0) against an e2m1 Bt (blgp = 4).

No GPU use here.  The CPU tier (test_mxf8f4_host.py) checks the builders and
shows that every wrong map changes more than half of C; the GPU tier
(test_gpu_gemm_mxf8f4.py) applies the same builders and comparisons to what
the kernels and the instruction return.

A's element values are given as numbers (checked to be e4m3 values) or as
codes, Bt's as numbers (checked to be e2m1 values), scales as exponents or
bytes; every expectation is exact float64 arithmetic on them, rounded once to
fp32 where it says so.
"""
from __future__ import annotations

import functools

import numpy as np

import gemm4_oracles as g4
import gemm8_oracles as g8
from cekirdekler_amd.ops import gemm
from gemm4_oracles import DECOY, E8M0_NAN, NONZERO, VALUES, _b_asym, _emu, _lane_scales, pack_values, scaled  # noqa: F401
from gemm_oracles import FINITE, NAN

# --------------------------------------------------------------------------- shapes
# K/256 = 1, 2, 3, 5: the ping-pong prologue stages two K-tiles ahead, the Bt
# ring has three buffers and the scales are prefetched one K-tile ahead
# (clamped at the end), so these are the counts at which the loop ends can go wrong
SHAPES = {"128x128": [(128, 128, 256), (384, 128, 512), (256, 256, 256), (256, 512, 768)],
          "128x256pbx": [(128, 256, 256), (256, 512, 512), (384, 256, 768), (512, 768, 1280)]}
RANDOM_SHAPE = (512, 512, 512)
HOST_SHAPE = (512, 512, 512)       # host-resident, streamed and re-upload paths: 8 tiles of 128×256
TWO_DEVICE_SHAPE = (512, 1024, 512)
OUT_SHAPE = (256, 512, 512)        # the output modes
# (shape, group_m) with M / BM = 3: a last tile group shorter than group_m
RAGGED = [((384, 512, 256), 2), ((384, 512, 256), 4)]

# --------------------------------------------------------------------------- helpers


def a_codes(x):
    """Exactly representable values ``[rows][K]`` → e4m3fn codes (checked)."""
    return g8._codes(x)


def set_operands(g, a, b, ea, eb):
    """Fill a GemmMxFp8Fp4 from element values (A exact in e4m3, B in e2m1)
    and scale exponents (one per row and block of 32, or one for all)."""
    g.A.array[:] = a_codes(a).ravel()
    g.B.array[:] = pack_values(b).ravel()
    g.SA.array[:] = np.broadcast_to(127 + np.asarray(ea), (g.M, g.K // 32)).ravel()
    g.SB.array[:] = np.broadcast_to(127 + np.asarray(eb), (g.N, g.K // 32)).ravel()


@functools.lru_cache(maxsize=None)
def int_case(shape):
    """A: integers in [-8, 8]; Bt: all 15 e2m1 values; scale exponents in
    {-1, 0, 1} per row and block, independently for A and Bt; and the float64
    product, once per shape.

    In units of 2^-3 (A's elements are integers, Bt's multiples of 2^-1, the
    scales at least 2^-1 each) every product is an integer of at most
    8·6·2·2·2^3 = 1536 and every partial sum an integer below K·1536 < 2^24:
    exact in fp32 in any summation order.  The products inside a group of 8
    neighbouring k share one block, so one pair of scales: before the scales
    the non-zero ones lie between 1·0.5 = 2^-1 and 8·6 = 48 < 2^6, and each is
    a multiple of 2^-1, so all their bits lie within the 7 positions 2^5 …
    2^-1, far inside the 14 the e4m3 path keeps below the largest of them
    (profiles/gemm8_specials.md)."""
    M, N, K = shape
    rng = np.random.default_rng(sum(shape))
    a = rng.integers(-8, 9, (M, K)).astype(np.float32)
    b = VALUES[rng.integers(0, 15, (N, K))]
    ea = rng.integers(-1, 2, (M, K // 32))
    eb = rng.integers(-1, 2, (N, K // 32))
    assert K * 1536 < 2 ** 24
    assert float(np.abs(a).max()) == 8 and float(np.abs(b).max()) == 6 and len(np.unique(b)) == 15
    nz_a, nz_b = np.abs(a[a != 0]), np.abs(b[b != 0])
    lo, hi = float(nz_a.min() * nz_b.min()), float(nz_a.max() * nz_b.max())
    assert lo == 0.5 and hi == 48 and np.array_equal(np.rint(b * 2), b * 2) and np.array_equal(np.rint(a), a)
    assert np.log2(hi) < 6 and 6 - np.log2(lo) <= 7 < 14
    ref = scaled(a, ea) @ scaled(b, eb).T
    assert np.array_equal(np.rint(ref * 8), ref * 8) and np.abs(ref * 8).max() < 2 ** 24
    assert (np.abs(scaled(a, ea)) @ np.abs(scaled(b, eb)).T * 8).max() < 2 ** 24
    for x in (a, b, ea, eb, ref):
        x.setflags(write=False)
    return a, b, ea, eb, ref


# --------------------------------------------------------------------------- the tile, emulated
# What kernels/sgemm_mxf8f4.hip does with its LDS bytes under the hypothesised
# maps, written out lane by lane: it shows that staging layout, read offsets,
# register order and scale addressing together give reference().


def hw_a_k(q, p):
    """Hypothesis, A (e4m3): byte p (0 … 31) of lane group q's operand is k of the instruction's 128."""
    return np.where(p < 16, 16 * q + p, 64 + 16 * q + (p - 16))


def hw_b_k(q, p, nib):
    """Hypothesis, Bt (e2m1): nibble `nib` of byte p (0 … 15) of lane group q's operand."""
    return 32 * q + 2 * p + nib


def emu_tile(a, b, sa, sb, *, a_order="e4m3", swap_nibbles=False, swap_steps=None, sa_tile_step=False,
             sa_shift_rows=0):
    """C [M][N] float64 of one pass of the tile's data path over whole
    matrices (the tile split does not enter: rows are independent).

    ``a`` [M][K] e4m3 codes, ``b`` [N][K/2] packed bytes, ``sa`` / ``sb``
    scale bytes [rows][K/32].  Per K-tile kt of 256 k and step s: A's
    sub-tile s is bytes [(2kt + s)·128, +128) of the row; lane group q reads
    its bytes [16q, 16q + 16) (registers 0–3) and [64 + 16q, 64 + 16q + 16)
    (registers 4–7); Bt's row of 128 B is bytes [kt·128, +128) and lane group q
    reads bytes [64s + 16q, +16); the scale byte of (row, lane group q) is that
    of block (2kt + s)·4 + q.  The instruction is emulated under hw_a_k /
    hw_b_k with the scale of lane group q applied to the k block q.

    Wrong maps: ``a_order="e2m1"``: A's lane group q reads 32 contiguous bytes
    [32q, 32q + 32); ``swap_nibbles``: Bt's nibbles exchanged;
    ``swap_steps="a"`` / ``"b"``: that operand's data reads sub-tile / step 1 − s
    (its scales in place); ``sa_tile_step``: SA's step index is kt + s;
    ``sa_shift_rows``: SA taken from the row that many below (a wrong op_sel
    is 16)."""
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    M, K = a.shape
    N = b.shape[0]
    av = gemm.from_fp8_e4m3_bits(a).astype(np.float64).reshape(M, K)
    codes = gemm.unpack_fp4(b).reshape(N, K)
    if swap_nibbles:
        codes = codes.reshape(N, K // 2, 2)[:, :, ::-1].reshape(N, K)
    bv = gemm.from_fp4_e2m1_codes(codes).astype(np.float64)
    ea = np.asarray(sa, np.int64).reshape(M, K // 32) - 127
    eb = np.asarray(sb, np.int64).reshape(N, K // 32) - 127
    ea = np.roll(ea, -sa_shift_rows, axis=0)
    out = np.zeros((M, N))
    p32, p16 = np.arange(32), np.arange(16)
    for kt in range(K // 256):
        for s in range(2):
            sda = 1 - s if swap_steps == "a" else s
            sdb = 1 - s if swap_steps == "b" else s
            a_sub = av[:, (2 * kt + sda) * 128:(2 * kt + sda) * 128 + 128]
            b_sub = bv[:, kt * 256 + sdb * 128:kt * 256 + sdb * 128 + 128]  # 64 B = 128 k
            a_hw, b_hw = np.zeros((M, 128)), np.zeros((N, 128))
            ea_hw, eb_hw = np.zeros((M, 128), np.int64), np.zeros((N, 128), np.int64)
            sta = kt + s if sa_tile_step else 2 * kt + s
            for q in range(4):
                src = hw_a_k(q, p32) if a_order == "e4m3" else 32 * q + p32  # bytes of the sub-tile the lane reads
                a_hw[:, hw_a_k(q, p32)] = a_sub[:, src]
                for nib in range(2):
                    b_hw[:, hw_b_k(q, p16, nib)] = b_sub[:, 32 * q + 2 * p16 + nib]
                ea_hw[:, 32 * q:32 * q + 32] = ea[:, sta * 4 + q][:, None]
                eb_hw[:, 32 * q:32 * q + 32] = eb[:, (2 * kt + s) * 4 + q][:, None]
            out += np.ldexp(a_hw, ea_hw) @ np.ldexp(b_hw, eb_hw).T
    return out


# --------------------------------------------------------------------------- the scale-mapping probe
# gemm4_oracles' construction at K = 768 (three K-tiles, six 128-k steps, 24
# blocks): A one-hot (value 1) at k = (37m + 11) % K, SA and SB varying with row
# and block, Bt the 14 nonzero e2m1 values, asymmetric in n and k.  The
# coefficients are gemm4_oracles' (its blind spots are in the block arithmetic,
# which is the same here); test_mxf8f4_host.py shows that each wrong map below
# changes more than half of C under both.
PROBE_SA_BLOCK_COEFF = [2, 4]
PROBE_SHAPE = g4.PROBE_SHAPE


def probe_case(c):
    """gemm4_oracles.probe_case(c): A's values (0 and 1) are e4m3 values too."""
    return g4.probe_case(c)


def probe_expected_and_wrong(c):
    """(want, {name: C a wrong map would give}) for probe_case(c), in closed
    form (test_mxf8f4_host.py checks several against emu_tile): gemm4_oracles'
    wrong maps that apply here, and those particular to the mixed form."""
    (M, N, K), pick, a, b, ea, eb = probe_case(c)
    nb = K // 32
    pb = pick // 32
    m, n = np.arange(M), np.arange(N)

    def c_of(k_at, ea_at, eb_at):  # the k of Bt that A's one meets [M], exponents [M] and [M][N]
        return b[:, k_at].T.astype(np.float64) * np.ldexp(1.0, ea_at[:, None] + eb_at)

    want = c_of(pick, ea[m, pb], eb[:, pb].T)
    np.testing.assert_array_equal(want, scaled(a, ea) @ scaled(b, eb).T)
    # A read with the e2m1 k order: byte p of 32 contiguous ones at 32q is taken for k = hw_a_k(q, p);
    # the scales are the hardware's: those of the block the element lands in
    kk = pick % 128
    landed = pick - kk + hw_a_k(kk // 32, kk % 32)
    # SA stepped by the 256-k tile: step 2kt + s is read at kt + s
    st = pb // 4
    sa_blk = (st // 2 + st % 2) * 4 + pb % 4
    wrong = {
        "unit scales": b[:, pick].T.astype(np.float64),
        "A block + 1": c_of(pick, ea[m, (pb + 1) % nb], eb[:, pb].T),
        "B block + 1": c_of(pick, ea[m, pb], eb[:, (pb + 1) % nb].T),
        "A row + 16 (op_sel)": c_of(pick, ea[(m + 16) % M, pb], eb[:, pb].T),
        "B row + 16 (op_sel)": c_of(pick, ea[m, pb], eb[(n + 16) % N][:, pb].T),
        "SA <-> SB": c_of(pick, eb[m % N, pb], ea[n % M][:, pb].T),
        "A in e2m1 k order": c_of(landed, ea[m, landed // 32], eb[:, landed // 32].T),
        "B nibbles swapped": c_of(pick ^ 1, ea[m, pb], eb[:, pb].T),
        "A steps exchanged": c_of(pick ^ 128, ea[m, pb], eb[:, (pick ^ 128) // 32].T),
        "B steps exchanged": c_of(pick ^ 128, ea[m, pb], eb[:, pb].T),
        "SA steps exchanged": c_of(pick, ea[m, pb ^ 4], eb[:, pb].T),
        "SB steps exchanged": c_of(pick, ea[m, pb], eb[:, pb ^ 4].T),
        "SA stepped by the K-tile": c_of(pick, ea[m, sa_blk], eb[:, pb].T),
    }
    return want, wrong


# --------------------------------------------------------------------------- the single-instruction probe
# One wave per problem does one v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz =
# 0, blgp = 4 on a 16×128 A (128 B per row, e4m3), a 16×128 Bt (64 B per row,
# e2m1) and one scale dword per lane and operand.  Each operand has the loader
# of its own format's probe: A lane l (row r = l % 16, q = l / 16) takes bytes
# [16q, 16q + 16) into registers 0–3 and [64 + 16q, 64 + 16q + 16) into 4–7
# (gemm8_oracles); Bt takes bytes [16q, 16q + 16) of its row into registers 0–3
# and 0x77 (two 6.0 per byte) into 4–7 (gemm4_oracles).  The scale dwords come
# as they are and SEL[p] = 4·op_sel(A) + op_sel(B).  The four results of a lane
# are C[4q + v][l % 16].  The answers are in profiles/gemm_mxf8f4.md.
PROBE_SRC = r"""
typedef int p84_i32x8 __attribute__((ext_vector_type(8)));
typedef float p84_f32x4 __attribute__((ext_vector_type(4)));
#define P84_CASE(OA, OB)                                                                            \
  case OA * 4 + OB:                                                                                 \
    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fa, fb, acc, 0, 4, OA, sa, OB, sb);     \
    break;
#define P84_ROW(OA) P84_CASE(OA, 0) P84_CASE(OA, 1) P84_CASE(OA, 2) P84_CASE(OA, 3)
__global__ void mx84_probe(const unsigned char* A, const unsigned char* Bt, const unsigned char* SA,
                           const unsigned char* SB, const int* SEL, float* C) {
  long long gid = get_global_id(0);
  long long p = gid >> 6;
  int l = (int)(gid & 63), r = l & 15, q = l >> 4;
  const int* a = (const int*)(A + p * 2048 + r * 128);
  const int* b = (const int*)(Bt + p * 1024 + r * 64);
  p84_i32x8 fa, fb;
  for (int w = 0; w < 4; ++w) {
    fa[w] = a[4 * q + w];
    fa[4 + w] = a[16 + 4 * q + w];
    fb[w] = b[4 * q + w];
    fb[4 + w] = 0x77777777;
  }
  int sa = ((const int*)SA)[p * 64 + l], sb = ((const int*)SB)[p * 64 + l];
  p84_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  switch (SEL[p]) {
    P84_ROW(0) P84_ROW(1) P84_ROW(2) P84_ROW(3)
  }
  for (int v = 0; v < 4; ++v) C[p * 256 + (4 * q + v) * 16 + r] = acc[v];
}
"""
PROBE_KERNEL = "mx84_probe"
K_MAP_PROBLEMS = g4.K_MAP_PROBLEMS


@functools.lru_cache(maxsize=None)
def probe_problems():
    """name → dict(a: e4m3 codes [16][128]; b: e2m1 values [16][128]; sa, sb:
    scale bytes [16][4]; sel: (op_sel A, op_sel B); decoy; want: (cls,
    expected) under the hypothesised maps (IEEE / OCP, one rounding to fp32);
    show: (row, col) sites the record keeps).  The questions and the names of
    the k-map and scale-map problems are gemm4_oracles', so that its read-back
    helpers apply as they stand."""
    rng = np.random.default_rng(43)
    out = {}
    one = np.full((16, 4), 127)

    def ints(lo=-4, hi=4):  # e2m1 holds the integers 0 … 4 (and 6); e4m3 every one to 16
        return rng.integers(lo, hi + 1, (16, 128)).astype(np.float32)

    def add(name, a, b, sa, sb, show, sel=(0, 0), decoy=False, poke=()):
        a, b = a_codes(a).reshape(16, 128).copy(), np.asarray(b, np.float32)
        for i, k, code in poke:
            a[i, k] = code
        sa, sb = np.asarray(sa, np.uint8).reshape(16, 4).copy(), np.asarray(sb, np.uint8).reshape(16, 4).copy()
        with np.errstate(invalid="ignore"):
            want = _emu(gemm.from_fp8_e4m3_bits(a).reshape(16, 128), b, sa, sb)
        p = dict(a=a, b=b, sa=sa, sb=sb, sel=sel, decoy=decoy, want=want, show=tuple(show))
        for v in (a, b, sa, sb) + p["want"]:
            v.setflags(write=False)
        out[name] = p

    r = np.arange(16)
    asym = _b_asym()  # e2m1 values: exact in e4m3 as well
    # question 1: which k each byte of A and each nibble of Bt supplies
    for j in range(K_MAP_PROBLEMS):
        hot = np.zeros((16, 128), np.float32)
        hot[r, 16 * j + r] = 1
        add(f"k_map_a{j}", hot, asym, one, one, [(0, 0), (5, 9), (15, 15)])
        add(f"k_map_b{j}", asym, hot, one, one, [(0, 0), (5, 9), (15, 15)])
    # question 2: which (row, block) a lane's scale byte applies to, per operand, and which byte op_sel picks
    hot = np.zeros((16, 128), np.float32)
    hot[r, (37 * r + 11) % 128] = 1
    distinct = 127 + 4 * r[:, None] + np.arange(4)[None, :] - 32
    for o in range(4):
        add(f"scale_map_a{o}", hot, asym, distinct, one, [(0, 0), (5, 9), (15, 15)], sel=(o, (o + 1) % 4), decoy=True)
        add(f"scale_map_b{o}", asym, hot, one, distinct, [(0, 0), (9, 5), (15, 15)], sel=((o + 2) % 4, o), decoy=True)
    add("baseline", rng.integers(-8, 9, (16, 128)), ints(), 127 + rng.integers(-2, 3, (16, 4)),
        127 + rng.integers(-2, 3, (16, 4)), [(0, 0), (5, 9), (15, 15)])
    # question 3a: scale byte 0xFF on one block of A, of Bt, and on a block of A that is all zeros
    ai, bi = ints(), ints()
    ai[12, 96:] = 0
    sa, sb = one.copy(), one.copy()
    sa[4, 1] = sa[12, 3] = sb[7, 2] = E8M0_NAN
    add("scale_nan", ai, bi, sa, sb, [(4, 0), (4, 1), (12, 0), (0, 7), (1, 7), (0, 0)], sel=(1, 2))
    # question 3b: the e4m3 NaN codes in A, in the low and the high half of a lane's bytes, against zeros too
    ai, bi = ints(), ints()
    bi[::3, 5] = 0
    bi[1::4, 100] = 0
    add("element_nan", ai, bi, one, one, [(3, 0), (3, 1), (9, 1), (0, 0)],
        poke=[(3, 5, g8.NAN_POS), (9, 100, g8.NAN_NEG)])
    # question 3c: exponent sums +254, 0 (254 with 0) and -254: positive A, every row of Bt of one sign
    ai = rng.integers(1, 9, (16, 128)).astype(np.float32)
    sign = np.where(r % 3 == 0, -1, 1)[:, None]
    bi = rng.integers(0, 5, (16, 128)).astype(np.float32) * sign
    bi[:, 1] = sign[:, 0]
    ends = np.repeat(np.where(r < 8, 254, 0), 4)
    add("scale_sums", ai, bi, ends, ends, [(0, 0), (0, 1), (0, 8), (8, 0), (8, 8), (8, 9)], sel=(2, 3))
    # question 3d: results in fp32's subnormal range: ea + eb = -140 (rows 0 … 11) and -149 (rows 12 … 15)
    sa = np.repeat(np.where(r < 12, 127 - 70, 127 - 79), 4)
    add("subnormal", ints(), ints(), sa, np.full(64, 127 - 70), [(0, 0), (1, 2), (12, 0), (13, 5)], sel=(3, 1))
    # question 4: two products of very different magnitude at neighbouring k.  Inside a block: 256·4 = 2^10 at
    # k = 0 beside 2^(7-i) · 2^(2 - j%4) = 2^(9 - i - j%4) at k = 1 (e4m3 reaches 2^-8 as a subnormal): 1 … 21
    # bits below the larger one's top …
    ai, bi = np.zeros((16, 128), np.float32), np.zeros((16, 128), np.float32)
    ai[:, 0], bi[:, 0] = 256, 4
    ai[:, 1] = 2.0 ** (7 - r)
    bi[:, 1] = 2.0 ** (2 - r % 4)
    add("adjacent_k", ai, bi, one, one, [(0, 0), (5, 6), (9, 3), (10, 3), (11, 3), (15, 15)])
    # … and across the boundary of blocks 0 and 1, gemm4_oracles' adjacent_blocks: 2^16 at k = 31 beside
    # 2^(14-i-j) at k = 32, the range made by the scales
    ai, bi = np.zeros((16, 128), np.float32), np.zeros((16, 128), np.float32)
    ai[:, 31] = bi[:, 31] = 4
    ai[:, 32] = bi[:, 32] = 1
    sa = one.copy()
    sa[:, 0] = 127 + 6
    sa[:, 1] = 127 + 7 - r
    add("adjacent_blocks", ai, bi, sa, sa, [(0, 0), (5, 6), (6, 6), (11, 10), (11, 11), (15, 15)])
    sub = out["subnormal"]["want"][1]
    assert (np.abs(sub) < 2.0 ** -126).all() and (sub != 0).mean() > 0.9
    ss = out["scale_sums"]["want"]
    assert (ss[0][:8, :8] != FINITE).all() and (ss[0][8:] == FINITE).all() and (ss[1][8:, 8:] == 0).all()
    assert (ss[1][:8, 8:] != 0).mean() > 0.9
    assert (out["scale_nan"]["want"][0] == NAN).sum() == 2 * 16 + 14
    assert (out["element_nan"]["want"][0] == NAN).sum() == 2 * 16
    return out


# the questions whose IEEE / OCP answer the instruction must give
PROBE_IEEE = ("baseline", "scale_nan", "element_nan", "scale_sums", "subnormal")
# measured (profiles/gemm_mxf8f4.md): inside a group of 8 neighbouring k the mixed form keeps this many bits
# from the top of the largest product down, as the pure e4m3 form does
ADJACENT_K_BITS = 14


def adjacent_k_as_measured():
    """What the matrix core returns for "adjacent_k": 2^10 plus 2^(9 - i - j%4)
    where that lies within ADJACENT_K_BITS bits from 2^10 down, else 2^10 alone."""
    e = 9 - np.add.outer(np.arange(16), np.arange(16) % 4)
    return 2.0 ** 10 + np.where(e > 10 - ADJACENT_K_BITS, 2.0 ** e, 0.0)


def probe_buffers():
    """The problems concatenated for one launch: (names, A, Bt, SA, SB, SEL);
    A e4m3 codes, Bt packed bytes, SA / SB one dword per lane as bytes, SEL int32."""
    pr = probe_problems()
    names = list(pr)
    a = np.concatenate([pr[n]["a"].ravel() for n in names])
    b = np.concatenate([pack_values(pr[n]["b"]).ravel() for n in names])
    sa = np.concatenate([_lane_scales(pr[n]["sa"], pr[n]["sel"][0], pr[n]["decoy"]) for n in names])
    sb = np.concatenate([_lane_scales(pr[n]["sb"], pr[n]["sel"][1], pr[n]["decoy"]) for n in names])
    sel = np.array([4 * pr[n]["sel"][0] + pr[n]["sel"][1] for n in names], np.int32)
    return names, a, b, sa, sb, sel


def probe_report(name, c):
    """One line of raw answers for a problem: class counts got / expected,
    finite mismatches and the values at the problem's `show` sites."""
    import gemm_oracles as go

    p = probe_problems()[name]
    cls, expected = p["want"]
    got = go.classify(c)
    fin = (cls == FINITE) & (got == FINITE)
    wrong = int((fin & (np.where(fin, c, 0).astype(np.float64) != expected)).sum())
    counts = lambda x: [int((x == k).sum()) for k in (FINITE, go.POS_INF, go.NEG_INF, NAN)]  # noqa: E731
    vals = ", ".join(f"C[{i}][{j}] = {float(c[i, j])!r} (0x{int(c.view(np.uint32)[i, j]):08X})" for i, j in p["show"])
    return (f"probe84 {name}: finite/+inf/-inf/nan got {counts(got)} expected {counts(cls)}, "
            f"{wrong} finite values differ; {vals}")


# read back with gemm4_oracles' helpers: the problems carry its names and its one-hot and exponent patterns
measured_k_map = g4.measured_k_map
measured_scale_map = g4.measured_scale_map
