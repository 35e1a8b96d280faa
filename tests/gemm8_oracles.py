"""Non-finite, overflow, underflow and scale-end cases for the fp8 and MXFP8
GEMM kernels (kernels/sgemm_fp8.hip, kernels/sgemm_mxfp8.hip, gemm8_tile.h),
in the manner of gemm_oracles.py.

No GPU use: the CPU tier (test_gemm8_oracles.py) shows that an honest kernel
passes every case and that each named wrong behaviour is rejected in every
element it affects; the GPU tier (test_gpu_gemm_fp8.py, test_gpu_gemm_mxfp8.py)
applies the same builders and comparisons to what the kernels return.

Every builder returns ``(a, b, sa, sb, want)``: ``a`` ``[M][K]`` and ``b``
``[N][K]`` e4m3fn codes (uint8), ``sa`` ``[M][K/32]`` and ``sb`` ``[N][K/32]``
E8M0 scale bytes (exponent + 127, ``0xFF`` = NaN; ``None`` for plain fp8) and
``want`` = ``(cls, expected)`` as gemm_oracles.assert_nonfinite takes it.
Expectations are exact arithmetic on the decoded codes and 2^e (integers, or
float64 where every term is a multiple of one power of two), rounded once to
fp32; never from_mxfp8, whose float32 result overflows at 448·2^127.

"Exact in any summation order" below means: every partial sum is a value
fp32 holds.  The matrix core adds the 8 products of neighbouring k in 14 bits
under the largest of them (profiles/gemm8_specials.md), so every case also
keeps the non-zero products of any 8 neighbouring k (one MX block, so one
pair of scales) within 2^6 of each other, with 8 significant bits at the
most: nothing of them lies below the cut.
"""
from __future__ import annotations

import functools

import numpy as np

from cekirdekler_amd.ops import gemm
from gemm_oracles import FINITE, NAN, NEG_INF, POS_INF, _int_product

NAN_POS, NAN_NEG = 0x7F, 0xFF   # the two e4m3fn NaN codes
E8M0_NAN = 0xFF
F32_MAX = float(np.finfo(np.float32).max)

# --------------------------------------------------------------------------- shapes
CLASS_SHAPES = [(256, 256, 128), (512, 256, 384)]   # one tile and K-tile; two tile rows and three K-tiles
UNDERFLOW_SHAPES = [(256, 256, 128), (256, 256, 256)]
SPLIT_SHAPE = (1024, 512, 256)                      # two logical devices, host-resident
# (shape, group_m) per tile size with M / BM = 3: a last tile group shorter
# than group_m, the gsz = min(rows - first, gm) branch of tile_coords; at
# group_m = 2 it follows a full group
RAGGED_GROUPS = {256: [((768, 512, 128), 2), ((768, 512, 128), 4)], 128: [((384, 256, 128), 2)]}


def ragged_groups(tile: str):
    """The (shape, group_m) pairs of RAGGED_GROUPS for a tile name."""
    return RAGGED_GROUPS[128 if tile == "128x128" else 256]


def nan_sites(shape):
    """(m1, k1), (m2, k2), (n3, k3), m4 of the non-finite cases.  In a 256×256
    tile (2×4 waves of 128×64, fragments of 16 rows) m1 is wave row 0 fragment
    2, m2 wave row 1 fragment 5, m4 wave row 1 fragment 3 and n3 wave column 2;
    with more than one tile row (column), m2 (n3) is in the last one.  In a
    128×128 tile (2×2 waves of 64×64) m1 and m2 are again in different wave
    rows and fragments.  k1 is in the first K-tile, k2 in the last, k3 in the
    middle one."""
    M, N, K = shape
    assert M % 128 == 0 and N % 128 == 0 and K % 128 == 0 and M >= 256 and N >= 256
    k3 = (K // 128 // 2) * 128 + 70
    return (35, 5), (M - 39, K - 3), (N - 106, k3), 177


def _codes(x):
    """Exactly representable values → e4m3fn codes (checked)."""
    x = np.asarray(x, np.float32)
    c = gemm.to_fp8_e4m3_bits(x)
    assert np.array_equal(gemm.from_fp8_e4m3_bits(c), x), "value not exact in e4m3"
    return c


def _freeze(*xs):
    for x in xs:
        if isinstance(x, tuple):
            _freeze(*x)
        elif x is not None:
            x.setflags(write=False)
    return xs


def _block_exp(e, K):
    """[rows][K/32] exponents → [rows][K]."""
    return np.repeat(np.asarray(e, np.int64), 32, axis=1)[:, :K]


def _want(ref, nan_rows=(), nan_cols=()):
    """(cls, expected) from an exact float64 product: what overflows fp32 is
    ±Inf, the rest must be an fp32 value already."""
    cls = np.where(ref > F32_MAX, POS_INF, np.where(ref < -F32_MAX, NEG_INF, FINITE)).astype(np.int8)
    for m in nan_rows:
        cls[m] = NAN
    for n in nan_cols:
        cls[:, n] = NAN
    expected = np.where(cls == FINITE, ref, 0.0)
    assert np.array_equal(expected.astype(np.float32).astype(np.float64), expected), "expectation not an fp32 value"
    return cls, expected


# --------------------------------------------------------------------------- cases

@functools.lru_cache(maxsize=None)
def fp8_nonfinite(shape):
    """Integers in [-8, 8]; A[m1][k1] = 0x7F, A[m2][k2] = 0xFF, Bt[n3][k3] =
    0x7F (nan_sites).  Bt has exact zeros in columns k1 and k2 and A in column
    k3, so 0·NaN occurs.  Rows m1, m2 and column n3 of C are NaN, every other
    element is FINITE and the int64 product of the remaining data."""
    M, N, K = shape
    assert K <= 1024
    (m1, k1), (m2, k2), (n3, k3), _ = nan_sites(shape)
    assert k1 < 128 and k2 >= K - 128 and (K < 384 or 128 <= k3 < K - 128) and len({k1, k2, k3}) == 3
    assert m1 // 16 % 8 != m2 // 16 % 8 and m1 % 256 // 128 != m2 % 256 // 128 and m1 % 128 // 64 != m2 % 128 // 64
    assert (M == 256 or m1 // 256 != m2 // 256) and (N == 256 or n3 // 256 > 0)
    rng = np.random.default_rng(17 + sum(shape))
    ai = rng.integers(-8, 9, (M, K))
    bi = rng.integers(-8, 9, (N, K))
    bi[::5, k1] = 0
    bi[2::7, k2] = 0
    ai[1::6, k3] = 0
    a, b = _codes(ai), _codes(bi)
    a[m1, k1], a[m2, k2], b[n3, k3] = NAN_POS, NAN_NEG, NAN_POS
    ai[m1, k1] = ai[m2, k2] = bi[n3, k3] = 0  # they touch the NaN rows and column only
    cls = np.full((M, N), FINITE, np.int8)
    cls[[m1, m2]] = NAN
    cls[:, n3] = NAN
    expected = np.where(cls == FINITE, _int_product(ai, bi), 0)
    return _freeze(a, b, None, None, (cls, expected))


MX_NF_EXP = 2  # block scale exponents of mx_nonfinite: -2 … 2


@functools.lru_cache(maxsize=None)
def mx_nonfinite(shape):
    """fp8_nonfinite with integers in [-4, 4] under block scales 2^-2 … 2^2,
    drawn independently for A and Bt.  The NaN element of row m1 sits in a
    block of scale byte 0, that of row m2 in a block of scale byte 254.  Row
    m4 has finite elements only, some of them zero, and scale byte 0xFF on its
    middle block: by the OCP MX rule (and e8m0_to_f64) the whole block is NaN,
    so row m4 of C is NaN.  Every other element is exact: in units of 2^-4
    every product is an integer <= 2^12 and every partial sum below K·2^12 <
    2^24."""
    M, N, K = shape
    assert K * 2 ** 12 < 2 ** 24
    (m1, k1), (m2, k2), (n3, k3), m4 = nan_sites(shape)
    assert len({m1, m2, m4}) == 3 and m4 // 16 % 8 not in (m1 // 16 % 8, m2 // 16 % 8)
    rng = np.random.default_rng(19 + sum(shape))
    ai = rng.integers(-4, 5, (M, K))
    bi = rng.integers(-4, 5, (N, K))
    ea = rng.integers(-MX_NF_EXP, MX_NF_EXP + 1, (M, K // 32))
    eb = rng.integers(-MX_NF_EXP, MX_NF_EXP + 1, (N, K // 32))
    bi[::5, k1] = 0
    bi[2::7, k2] = 0
    ai[1::6, k3] = 0
    blk4 = K // 32 // 2
    ai[m4, 32 * blk4:32 * blk4 + 32:3] = 0
    assert (ai[m4, 32 * blk4:32 * blk4 + 32] != 0).any()
    a, b = _codes(ai), _codes(bi)
    a[m1, k1], a[m2, k2], b[n3, k3] = NAN_POS, NAN_NEG, NAN_POS
    sa, sb = (127 + ea).astype(np.uint8), (127 + eb).astype(np.uint8)
    sa[m1, k1 // 32], sa[m2, k2 // 32], sa[m4, blk4] = 0, 254, E8M0_NAN
    assert not (a[m4] & 0x7F == 0x7F).any()
    ai[[m1, m2, m4]] = 0
    bi[n3] = 0
    ref = np.ldexp(ai.astype(np.float64), _block_exp(ea, K)) @ np.ldexp(bi.astype(np.float64), _block_exp(eb, K)).T
    assert np.array_equal(np.rint(ref * 16), ref * 16) and np.abs(ref * 16).max() < 2 ** 24
    return _freeze(a, b, sa, sb, _want(ref, nan_rows=(m1, m2, m4), nan_cols=(n3,)))


SCALE_END_KINDS = ("cancel_hi_lo", "cancel_lo_hi", "overflow", "underflow", "underflow_zero")
UNDERFLOW_SUM = -140  # ea + eb of every block pair in the "underflow" kind
CANCEL_MAGS = np.arange(256, 449, 32)  # e4m3's top binade: the magnitudes of the cancelling kinds


def overflow_sites(shape):
    """(m5, m6) of the overflow kind: different wave rows of a 256×256 tile."""
    return 21, shape[0] - 100


@functools.lru_cache(maxsize=None)
def mx_scale_ends(shape, kind):
    """The ends of the E8M0 range, integer-valued elements throughout.

    "cancel_hi_lo" / "cancel_lo_hi": SA = 254 with SB = 0 (and the reverse),
    uniform.  Elements are 0 or ±CANCEL_MAGS, the values of e4m3's top binade
    (256 … 448 in steps of 32), ±448 in every row.  2^127·2^-127 = 1: C is the
    unit-scale integer product.  Every product is a multiple of 2^10 between
    2^16 and 448² < 2^18, that is an 8-bit integer times 2^10: an adder that
    aligns its addends to the largest and keeps no more bits than one e4m3
    product has still holds each of them whole (the matrix core's first adder
    stage is that narrow, profiles/gemm8_specials.md: data that mixes ±448
    with small integers is NOT summed exactly, under any scales), and Σ|a·b| <
    2^24·2^10, so every partial sum is exact in fp32 in any order.  A scale
    applied to its operand in fp32 first overflows every non-zero element.

    "overflow": scales uniform along K.  Row m5 of A is all +448 under byte
    254; row m6 all +2^-9 under byte 227 (2^100); the other rows hold integers
    in [-8, 8] under 2^-20 … 2^-18.  Rows n % 4 == 0 of Bt hold j·2^-9, j in
    0 … 8, under byte 254, the others integers 0 … 8 under 2^-1 … 2^1; every
    row of Bt times one sign that varies with n, with exact zeros and at
    least one non-zero.  C[m5][n] = ±Inf by the sign of row n (every single
    product is beyond fp32, and a row has one sign: no Inf − Inf in any
    order), byte 254 + byte 254 included; C[m6][n] = ±Inf at n % 4 == 0
    (2^-18·2^227), where an exponent sum clamped to 127 stays finite; all
    other elements finite and exact.

    "underflow": integers in [-4, 4]; ea[m][blk] = -70 + t[blk], eb[n][blk] =
    -70 - t[blk], t in [-57, 57] per block, so ea + eb = -140 on every block
    pair while single scales span 2^-127 … 2^-13.  Every product is an integer
    times 2^-140 and Σ|a·b| <= 16·K·2^-140 < 2^-126: every partial sum in any
    order is an exact fp32 subnormal.  Inputs, products or sums flushed to
    zero give 0.

    "underflow_zero": the same elements under SA = SB = 0: every product is
    below 2^-250 and every sum far below 2^-150, so C is ±0 everywhere, and
    nowhere NaN.  (Products that are no multiple of 2^-149 but not negligible
    are left out on purpose: their rounding inside the instruction is not
    specified.)"""
    M, N, K = shape
    assert kind in SCALE_END_KINDS, kind
    rng = np.random.default_rng(23 + sum(shape) + SCALE_END_KINDS.index(kind))
    nb = K // 32
    if kind.startswith("cancel"):
        def operand(rows):
            x = rng.choice(CANCEL_MAGS, (rows, K)) * rng.choice([-1, 1], (rows, K))
            x[rng.random((rows, K)) < 0.25] = 0
            return x

        ai, bi = operand(M), operand(N)
        assert (np.abs(ai) == 448).any(axis=1).all() and (np.abs(bi) == 448).any(axis=1).all()
        assert _int_product(np.abs(ai), np.abs(bi)).max() < 2 ** 24 * 2 ** 10  # in units of 2^10
        ref = _int_product(ai, bi).astype(np.float64)
        assert (ref != 0).mean() > 0.99
        hi, lo = np.full((M, nb), 254, np.uint8), np.full((N, nb), 0, np.uint8)
        sa, sb = (hi, lo) if kind == "cancel_hi_lo" else (hi * 0, lo + 254)
        return _freeze(_codes(ai), _codes(bi), sa, sb, _want(ref))
    if kind == "overflow":
        m5, m6 = overflow_sites(shape)
        assert m5 % 256 // 128 != m6 % 256 // 128 and m5 != m6
        av = rng.integers(-8, 9, (M, K)).astype(np.float64)
        av[m5], av[m6] = 448.0, 2.0 ** -9
        ea = -20 + np.arange(M) % 3
        ea[m5], ea[m6] = 127, 100
        big = np.arange(N) % 4 == 0
        sign = np.where((np.arange(N) // 2) % 3 == 0, -1.0, 1.0)
        assert len({(bool(g), s) for g, s in zip(big, sign)}) == 4  # both signs under both kinds of scale
        mag = rng.integers(0, 9, (N, K)).astype(np.float64)
        mag[:, ::9] = 0
        mag[:, 1] = 1 + np.arange(N) % 8
        assert (mag == 0).any(axis=1).all() and (mag != 0).any(axis=1).all()
        bv = sign[:, None] * np.where(big[:, None], mag * 2.0 ** -9, mag)
        eb = np.where(big, 127, np.arange(N) % 3 - 1)
        # exact in float64: scales uniform along K, so every element of C sums
        # integer multiples of one power of two, fewer than 2^53 of them
        ref = np.ldexp(av, ea[:, None]) @ np.ldexp(bv, eb[:, None]).T
        cls, expected = _want(ref)
        inf = np.where(sign > 0, POS_INF, NEG_INF)
        assert np.array_equal(cls[m5], inf) and np.array_equal(cls[m6], np.where(big, inf, FINITE))
        rest = np.ones(M, bool)
        rest[[m5, m6]] = False
        assert (cls[rest] == FINITE).all() and np.abs(expected[rest][:, big]).max() > 2.0 ** 100
        # finite elements: every term an integer multiple of one power of two
        # (2^-9 finer for row m6 and for the rows of Bt under byte 254), Σ|a·b|
        # below 2^24 of them: exact in fp32 in any order
        unit = np.where(np.arange(M) == m6, 2.0 ** -9, 1.0)[:, None] * np.where(big, 2.0 ** -9, 1.0)[None, :]
        fin = cls == FINITE
        assert ((np.abs(av) @ np.abs(bv).T)[fin] / unit[fin] < 2 ** 24).all()
        sa = np.broadcast_to((127 + ea).astype(np.uint8)[:, None], (M, nb)).copy()
        sb = np.broadcast_to((127 + eb).astype(np.uint8)[:, None], (N, nb)).copy()
        return _freeze(_codes(av), _codes(bv), sa, sb, (cls, expected))
    assert K in (128, 256)
    ai = rng.integers(-4, 5, (M, K))
    bi = rng.integers(-4, 5, (N, K))
    prod = _int_product(ai, bi)
    if kind == "underflow":
        t = np.linspace(-57, 57, nb).astype(np.int64)
        ea = np.broadcast_to(-70 + t, (M, nb))
        eb = np.broadcast_to(-70 - t, (N, nb))
        assert ((ea[:, None, :] + eb[None, :, :]) == UNDERFLOW_SUM).all() and ea.min() == -127 and eb.min() == -127
        # every product an integer times 2^-140, every partial sum below 2^-126
        assert _int_product(np.abs(ai), np.abs(bi)).max() * 2.0 ** UNDERFLOW_SUM < 2.0 ** -126
        ref = prod.astype(np.float64) * 2.0 ** UNDERFLOW_SUM
        assert np.array_equal(ref / 2.0 ** -149, np.rint(ref / 2.0 ** -149)) and (ref != 0).mean() > 0.9
        assert (np.abs(ref[ref != 0]) < 2.0 ** -126).all()  # all of C is subnormal
    else:
        ea, eb = np.full((M, nb), -127), np.full((N, nb), -127)
        assert _int_product(np.abs(ai), np.abs(bi)).max() * 2.0 ** -254 < 2.0 ** -200
        ref = np.zeros((M, N))
    return _freeze(_codes(ai), _codes(bi), (127 + ea).astype(np.uint8), (127 + eb).astype(np.uint8), _want(ref))


# --------------------------------------------------------------------------- emulators
# plain numpy on the codes and scale bytes: what an honest kernel returns, and
# the named wrong behaviours

def decode(codes, nan_as_480=False):
    """e4m3fn codes → float64.  `nan_as_480` (wrong): the value the NaN codes
    would hold in an e4m3 without NaN, ±480."""
    v = gemm.from_fp8_e4m3_bits(codes).astype(np.float64)
    if nan_as_480:
        v = np.where(np.asarray(codes) == NAN_POS, 480.0, np.where(np.asarray(codes) == NAN_NEG, -480.0, v))
    return v


def scale_exp(s, K, nan_as_128=False):
    """Scale bytes [rows][K/32] (None: unit) → (exponent [rows][K] int64, NaN
    mask [rows][K]).  `nan_as_128` (wrong): 0xFF read as 2^128."""
    s = np.asarray(s, np.int64)
    nan = _block_exp(s == E8M0_NAN, K).astype(bool)
    if nan_as_128:
        nan[:] = False
    return _block_exp(s - 127, K), nan


def _f32(x):
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return np.asarray(x, np.float64).astype(np.float32)


def emu_gemm8(a, b, sa=None, sb=None, *, nan_as_480=False, nan_as_128=False, operand_f32=False, exp_sum=None,
              flush=False):
    """C = (a∘sa)·(b∘sb)ᵀ element by element over k: products exact in
    float64 (the exponents of the two scales are added as integers first),
    summed in float64, rounded once to fp32; NaN wherever a term is NaN, as
    IEEE has it (0·NaN included).  Wrong behaviours: `operand_f32`: each scale
    applied to its operand in fp32 before the multiply; `exp_sum`: a function
    of the summed exponent (wrap, clamp); `flush`: subnormal results → 0."""
    M, K = a.shape
    N = b.shape[0]
    av, bv = decode(a, nan_as_480), decode(b, nan_as_480)
    one = np.full((1, K // 32), 127)
    ea, na = scale_exp(np.broadcast_to(one, (M, K // 32)) if sa is None else sa, K, nan_as_128)
    eb, nb_ = scale_exp(np.broadcast_to(one, (N, K // 32)) if sb is None else sb, K, nan_as_128)
    av = np.where(na, np.nan, av)
    bv = np.where(nb_, np.nan, bv)
    out = np.empty((M, N), np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if operand_f32:
            av, ea = _f32(np.ldexp(av, ea)).astype(np.float64), np.zeros_like(ea)
            bv, eb = _f32(np.ldexp(bv, eb)).astype(np.float64), np.zeros_like(eb)
        for m in range(M):
            e = ea[m][None, :] + eb
            if exp_sum is not None:
                e = exp_sum(e)
            # 2^e in two steps: float64 holds 2^254 and 2^-254, and the sums here are exact by the cases' design
            row = _f32((np.ldexp(av[m][None, :] * bv, e)).sum(axis=1))
            out[m] = row
    if flush:
        out = np.where(np.abs(out) < 2.0 ** -126, np.float32(0), out)
    return out


def wrap8(e):
    """An exponent sum kept in 8 signed bits."""
    return (np.asarray(e, np.int64) + 128) % 256 - 128


def clamp8(e):
    """An exponent sum clamped to E8M0's own range."""
    return np.clip(e, -127, 127)


# --------------------------------------------------------------------------- the single-instruction probe
# One wave per problem does one v_mfma_scale_f32_16x16x128_f8f6f4 on a 16×128
# A, a 16×128 Bt and their 16×4 scale bytes, with the lane maps written out
# in the header of kernels/sgemm_mxfp8.hip: lane l holds row l % 16; its low
# 16 B are k in [16q, 16q + 16) and its high 16 B k in [64 + 16q, 64 + 16q +
# 16), q = l / 16; its scale byte is that of row l % 16 and block q; its four
# results are C[4q + v][l % 16].  It says what the instruction does, apart
# from everything the GEMM kernels add.
PROBE_SRC = r"""
typedef int probe_i32x8 __attribute__((ext_vector_type(8)));
typedef float probe_f32x4 __attribute__((ext_vector_type(4)));
__global__ void mx_probe(const unsigned char* A, const unsigned char* Bt, const unsigned char* SA,
                         const unsigned char* SB, float* C) {
  long long gid = get_global_id(0);
  long long p = gid >> 6;
  int l = (int)(gid & 63), r = l & 15, q = l >> 4;
  const int* a = (const int*)(A + p * 2048 + r * 128);
  const int* b = (const int*)(Bt + p * 2048 + r * 128);
  probe_i32x8 fa, fb;
  for (int h = 0; h < 2; ++h)
    for (int w = 0; w < 4; ++w) {
      fa[4 * h + w] = a[16 * h + 4 * q + w];
      fb[4 * h + w] = b[16 * h + 4 * q + w];
    }
  int sa = SA[p * 64 + r * 4 + q], sb = SB[p * 64 + r * 4 + q];
  probe_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fa, fb, acc, 0, 0, 0, sa, 0, sb);
  for (int v = 0; v < 4; ++v) C[p * 256 + (4 * q + v) * 16 + r] = acc[v];
}
"""
PROBE_KERNEL = "mx_probe"


@functools.lru_cache(maxsize=None)
def probe_problems():
    """name → (a, b, sa, sb, (cls, expected), show): 16×16×128 problems, one
    per question, the expectation being IEEE / OCP (emu_gemm8, exact by
    design: integer elements, and per element of C either one exponent sum or
    a spread of a few bits); `show` lists the (row, col) whose raw values the
    record keeps."""
    rng = np.random.default_rng(29)
    out = {}

    def ints(lo=-4, hi=4):
        return rng.integers(lo, hi + 1, (16, 128))

    def add(name, ai, bi, sa, sb, show, poke=()):
        a, b = _codes(ai), _codes(bi)
        for arr, i, k, code in poke:
            (a if arr == "a" else b)[i, k] = code
        sa, sb = np.asarray(sa, np.uint8).reshape(16, 4).copy(), np.asarray(sb, np.uint8).reshape(16, 4).copy()
        c = emu_gemm8(a, b, sa, sb)
        cls = np.where(np.isnan(c), NAN, np.where(c == np.inf, POS_INF, np.where(c == -np.inf, NEG_INF, FINITE)))
        want = (cls.astype(np.int8), np.where(cls == FINITE, c, 0).astype(np.float64))
        out[name] = _freeze(a, b, sa, sb, want) + (tuple(show),)

    # the probe's own lane maps: mixed block scales, exact
    add("baseline", ints(), ints(), 127 + rng.integers(-2, 3, (16, 4)), 127 + rng.integers(-2, 3, (16, 4)),
        [(0, 0), (5, 9), (15, 15)])
    # element NaN, both codes, in the low and the high half of a lane's bytes, against zeros too
    ai, bi = ints(), ints()
    bi[::3, 5] = 0
    bi[1::4, 100] = 0
    ai[::2, 70] = 0
    add("element_nan", ai, bi, np.full(64, 127), np.full(64, 127), [(3, 0), (3, 1), (9, 1), (0, 6), (2, 6), (0, 0)],
        poke=[("a", 3, 5, NAN_POS), ("a", 9, 100, NAN_NEG), ("b", 6, 70, NAN_POS)])
    # scale byte 0xFF on one block of A, of Bt, and on a block of A that is all zeros
    ai, bi = ints(), ints()
    ai[12, 96:] = 0
    sa, sb = np.full((16, 4), 127), np.full((16, 4), 127)
    sa[4, 1] = sa[12, 3] = sb[7, 2] = E8M0_NAN
    add("scale_nan", ai, bi, sa, sb, [(4, 0), (4, 1), (12, 0), (0, 7), (1, 7), (0, 0)])
    # exponent sums +254, 0 (254 with 0) and -254: positive A, every row of Bt of one sign
    ai = ints(1, 8)
    bi = ints(0, 8) * np.where(np.arange(16) % 3 == 0, -1, 1)[:, None]
    bi[:, 1] = np.where(np.arange(16) % 3 == 0, -1, 1)
    sa = np.repeat(np.where(np.arange(16) < 8, 254, 0), 4)
    add("scale_sums", ai, bi, sa, sa, [(0, 0), (0, 1), (0, 8), (8, 0), (8, 8), (8, 9)])
    # subnormal results: ea + eb = -140 (rows 0 … 11) and -149 (rows 12 … 15)
    sa = np.repeat(np.where(np.arange(16) < 12, 127 - 70, 127 - 79), 4)
    add("subnormal", ints(), ints(), sa, np.full(64, 127 - 70), [(0, 0), (1, 2), (12, 0), (13, 5)])
    # two products at neighbouring k, 2^16 and 2^(14-i-j): how many bits below the larger does the sum keep?
    ai, bi = np.zeros((16, 128)), np.zeros((16, 128))
    ai[:, 0] = bi[:, 0] = 256
    ai[:, 1] = bi[:, 1] = 2.0 ** (7 - np.arange(16))
    add("adjacent_k", ai, bi, np.full(64, 127), np.full(64, 127), [(0, 0), (5, 6), (6, 6), (11, 10), (15, 15)])
    sub = out["subnormal"][4][1]
    assert (np.abs(sub) < 2.0 ** -126).all() and (sub != 0).mean() > 0.9
    ss = out["scale_sums"][4][0]
    assert (ss[:8, :8] != FINITE).all() and (ss[8:] == FINITE).all() and (out["scale_sums"][4][1][8:, 8:] == 0).all()
    assert (out["element_nan"][4][0] == NAN).sum() == 2 * 16 + 14 and (out["scale_nan"][4][0] == NAN).sum() == 2 * 16 + 14
    return out


# the questions whose IEEE / OCP answer the instruction gives; "adjacent_k" it does not
PROBE_IEEE = ("baseline", "element_nan", "scale_nan", "scale_sums", "subnormal")
ADJACENT_K_BITS = 14  # measured: bits 2^16 … 2^3 of the sum of two neighbouring products survive


def adjacent_k_as_measured():
    """What the matrix core returns for the "adjacent_k" question (MI355X,
    profiles/gemm8_specials.md): the products of 8 neighbouring k are aligned
    to the largest and cut below its 14th bit before they are summed, so
    2^(14-i-j) is lost whole once it is below 2^3."""
    e = 14 - np.add.outer(np.arange(16), np.arange(16))
    return 2.0 ** 16 + np.where(e > 16 - ADJACENT_K_BITS, 2.0 ** e, 0.0)


def probe_buffers():
    """The problems concatenated for one launch: (names, A, Bt, SA, SB)."""
    pr = probe_problems()
    names = list(pr)
    cat = lambda i: np.concatenate([pr[n][i].ravel() for n in names])  # noqa: E731
    return names, cat(0), cat(1), cat(2), cat(3)


def probe_report(name, c):
    """One line of raw answers for a problem: class counts got / expected,
    finite mismatches and the values at the problem's `show` sites."""
    import gemm_oracles as go

    *_, (cls, expected), show = probe_problems()[name]
    got = go.classify(c)
    fin = (cls == FINITE) & (got == FINITE)
    wrong = int((fin & (np.where(fin, c, 0).astype(np.float64) != expected)).sum())
    counts = lambda x: [int((x == k).sum()) for k in (FINITE, POS_INF, NEG_INF, NAN)]  # noqa: E731
    vals = ", ".join(f"C[{i}][{j}] = {float(c[i, j])!r} (0x{int(c.view(np.uint32)[i, j]):08X})" for i, j in show)
    return (f"probe {name}: finite/+inf/-inf/nan got {counts(got)} expected {counts(cls)}, "
            f"{wrong} finite values differ; {vals}")


# --------------------------------------------------------------------------- the 14-bit sum of 8 neighbouring products
# (a measured property of the matrix core, not IEEE: profiles/gemm8_specials.md)

GROUP_K, GROUP_BITS = 8, 14


@functools.lru_cache(maxsize=None)
def wide_groups(shape):
    """Integers in [-8, 8] with two ±448 per row of A and of Bt at k from a
    shared pool of four: in most groups of 8 neighbouring k a product of
    ±3584 or ±200704 stands beside products of 1 … 64, more than 14 bits
    below its top.  `want` is what the matrix core returns by the measured
    rule (emu_group_sums), `exact` the integer product it misses."""
    M, N, K = shape
    rng = np.random.default_rng(31 + sum(shape))
    pool = np.unique(np.linspace(0, K - 1, 4).astype(np.int64))

    def operand(rows):
        x = rng.integers(-8, 9, (rows, K))
        pos = np.argsort(rng.random((rows, len(pool))), axis=1)[:, :2]
        x[np.arange(rows)[:, None], pool[pos]] = rng.choice([-448, 448], (rows, 2))
        return x

    ai, bi = operand(M), operand(N)
    assert _int_product(np.abs(ai), np.abs(bi)).max() < 2 ** 24
    a, b = _codes(ai), _codes(bi)
    want = emu_group_sums(a, b)
    exact = _int_product(ai, bi)
    assert (want != exact).mean() > 0.5 and np.abs(want - exact).max() < 8 * (K // GROUP_K)
    return _freeze(a, b, want, exact)


def emu_group_sums(a, b):
    """a·bᵀ as the fp8 matrix instructions add it: in every group of 8
    neighbouring k the products are cut (towards zero) to multiples of
    2^(E − 13), E the largest sum of the two operands' exponents among the
    group's non-zero products; everything else is added exactly (integer data
    with Σ|a·b| < 2^24, no e4m3 subnormals).  Returns float64."""
    av, bv = decode(a), decode(b)
    assert np.isfinite(av).all() and np.isfinite(bv).all()
    assert (np.abs(av[av != 0]) >= 2.0 ** -6).all() and (np.abs(bv[bv != 0]) >= 2.0 ** -6).all()
    M, K = av.shape
    N = bv.shape[0]
    ea, eb = np.frexp(av)[1] - 1, np.frexp(bv)[1] - 1
    out = np.empty((M, N))
    for m in range(M):
        p = (av[m][None, :] * bv).reshape(N, K // GROUP_K, GROUP_K)
        e = np.where(p != 0, (ea[m][None, :] + eb).reshape(p.shape), -1000)
        cut = np.ldexp(1.0, e.max(axis=2) - (GROUP_BITS - 1))[..., None]
        out[m] = (np.trunc(p / cut) * cut).sum(axis=(1, 2))
    return out
