"""Exact-data cases, derived bounds and numpy emulators for the bf16 and fp32
GEMM kernels (kernels/sgemm_bf16.hip, kernels/sgemm_f32.hip).

No GPU use: the CPU tier (test_gemm_oracles.py) shows that honest kernels pass
every case and that subtly wrong ones are rejected, the GPU tier
(test_gpu_gemm_oracles.py) applies the same builders and comparison functions
to what the kernels return.

Every builder returns ``(a, b, expected)`` with ``a`` ``[M][K]`` and ``b``
``[N][K]`` as float32 values and ``C = a · bᵀ``.  ``fmt`` is ``"bf16"`` or
``"f32"``: for bf16 the builders assert that the operands survive the trip
through bf16 bit patterns, so the kernel multiplies exactly these numbers.
"""
from __future__ import annotations

import functools

import numpy as np

from cekirdekler_amd.ops import gemm
from kernel_oracles import check_bound as check_within_bound  # noqa: F401  (the per-element comparison, shared)

# the two tolerances of the GEMM oracle tests, both derived (accumulation_bound)
UNIT_F32 = 2.0 ** -24
UNIT_BF16 = 2.0 ** -23
UNIT = {"f32": UNIT_F32, "bf16": UNIT_BF16}

# --------------------------------------------------------------------------- shapes
# (shared by both tiers, so the CPU tier validates exactly what the GPU tier runs)

# K/64 = 1, 2, 3, 5, 16: below, at and above the prefetch depths of the
# one-stage, ping-pong and balanced-DMA loops
BF16_SHAPES = [(256, 256, 64), (512, 256, 128), (256, 512, 192), (768, 512, 320), (1024, 768, 1024)]
BF16_SMALL_TILE_SHAPES = [(128, 128, 64), (384, 128, 128)]  # for the 128x128 tile
BF16_GROUPED_SHAPE = (768, 512, 320)  # three 256-row tile rows: a short last tile group at group_m 2 (and 4 at 128 rows)
BF16_MULTI = (768, 512, 320)          # the multi-tile shape of the one-shape cases
BF16_RANDOM = (1024, 512, 512)
F32_SHAPES = [(m, n, k) for (m, n) in [(512, 256), (768, 512), (512, 512)] for k in (32, 64, 96, 160, 256)]
F32_MULTI = (768, 512, 96)
F32_RANDOM = (512, 512, 256)
SPLIT_MN = (768, 512)
SPLIT_K_CASES = [(128, 2), (256, 4), (384, 2), (1024, 2), (1024, 4)]  # (K, S): 1, 1, 3, 8, 4 K-tiles per split
HANDOVER_K = [128, 256, 640, 1024]  # K/64 = 2, 4, 10, 16
HOST_SHAPE = (1024, 512, 256)  # the host-resident and verify paths: four tile groups at group_m 1 (four blobs)


def bf16_shapes(tile: str):
    """The bf16 shapes `tile` can run: the two small ones for the 128x128 tile
    only, and an even K/64 for the hand-over tiles (two K-splits)."""
    shapes = BF16_SHAPES + (BF16_SMALL_TILE_SHAPES if tile == "128x128" else [])
    return [s for s in shapes if tile not in gemm.EXCHANGE_TILES or (s[2] // 64) % 2 == 0]


def bf16_multi(tile: str):
    """The multi-tile shape of the one-shape cases (K/64 = 6 for the hand-over
    tiles: helper/owner 1/5, and 3/3 for the even split)."""
    return (768, 512, 384) if tile in gemm.EXCHANGE_TILES else BF16_MULTI


def f32_shapes(tile: str):
    """The fp32 shapes that are whole tiles of `tile` (filtered here, when the
    parameter lists are built)."""
    BM, BN = gemm.F32_TILES[tile][:2]
    return [s for s in F32_SHAPES if s[0] % BM == 0 and s[1] % BN == 0]


def handover_ktiles(tile: str, K: int):
    """(helper, owner) K-tiles of an exchange tile at K, with the shift clamp
    of GemmBf16.__init__ (the helper keeps at least one K-tile)."""
    shift = max(0, min(gemm.EXCHANGE_SHIFT[tile], K // 128 - 1))
    return K // 128 - shift, K // 128 + shift


# --------------------------------------------------------------------------- helpers

def _check_fmt(fmt, *ops):
    assert fmt in UNIT, fmt
    out = []
    for x in ops:
        x = np.ascontiguousarray(x, np.float32)
        if fmt == "bf16":
            back = gemm.from_bf16_bits(gemm.to_bf16_bits(x))
            assert np.array_equal(back.view(np.uint32), x.view(np.uint32)), "operand not exact in bf16"
        out.append(x)
    return out


def _frozen(a, b, expected):
    for x in (a, b, expected):
        x.setflags(write=False)
    return a, b, expected


def _int_product(ai, bi):
    """ai · biᵀ as int64, through float64 (exact: every sum is far below 2^53)."""
    return (ai.astype(np.float64) @ bi.astype(np.float64).T).astype(np.int64)


def round_mantissa(x, bits):
    """float32 values rounded (nearest even) to `bits` explicit mantissa bits
    (7: bf16), returned as float64.  Finite inputs."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    drop = 23 - bits
    r = (u + ((1 << (drop - 1)) - 1) + ((u >> drop) & 1)) >> drop << drop
    return r.astype(np.uint32).view(np.float32).astype(np.float64)


def trunc_mantissa(x, bits):
    """float32 values truncated to `bits` explicit mantissa bits (10: the
    TF32 operand format), returned as float64."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return (u & np.uint32((0xFFFFFFFF << (23 - bits)) & 0xFFFFFFFF)).view(np.float32).astype(np.float64)


# --------------------------------------------------------------------------- cases

@functools.lru_cache(maxsize=None)
def exact_integers(shape, seed=None, fmt="bf16"):
    """Integers in [-8, 8] and their int64 product.  Every product and partial
    sum is an integer of magnitude <= 64·K <= 2^16 (K <= 1024): the fp32
    result is exact in any summation order."""
    M, N, K = shape
    assert K <= 1024
    rng = np.random.default_rng(sum(shape) if seed is None else seed)
    ai = rng.integers(-8, 9, (M, K))
    bi = rng.integers(-8, 9, (N, K))
    a, b = _check_fmt(fmt, ai, bi)
    return _frozen(a, b, _int_product(ai, bi))


WIDE_BIG = 2.0 ** 11
WIDE_PER_ROW = 3      # ±2^11 entries per row of A and of B
WIDE_POOL = 6         # drawn from this many k positions, spread over K (first and last k included)
# Share of elements with Σ|a·b| >= 2^23 and an odd expected value that the
# builder guarantees.  Two rows share >= 2 of their 3 positions out of 6 with
# probability 10/20, and about half of the values are odd: about 0.25.
WIDE_MIN_SHARE = 0.2


@functools.lru_cache(maxsize=None)
def wide_integers(shape, seed=0, fmt="bf16"):
    """The tolerance-free precision case.  Integers in [-4, 4], plus
    WIDE_PER_ROW entries of ±2^11 per row of A and of B at k positions drawn
    from a pool of WIDE_POOL, so they coincide (a product of ±2^22) for some
    (m, n) and not for others.  Σ_k |a·b| < 2^24 for every element, so every
    partial sum in any order is an integer that fp32 holds exactly, while a
    stated share of elements needs all 24 bits: an accumulator, a partial-tile
    workspace or a hand-over buffer narrower than fp32 fails bit for bit."""
    M, N, K = shape
    rng = np.random.default_rng(seed + sum(shape))
    pool = np.unique(np.linspace(0, K - 1, WIDE_POOL).astype(np.int64))
    assert len(pool) == WIDE_POOL

    def operand(rows):
        x = rng.integers(-4, 5, (rows, K)).astype(np.int64)
        pos = np.argsort(rng.random((rows, WIDE_POOL)), axis=1)[:, :WIDE_PER_ROW]
        sign = rng.choice([-1, 1], (rows, WIDE_PER_ROW))
        x[np.arange(rows)[:, None], pool[pos]] = sign * int(WIDE_BIG)
        return x

    ai, bi = operand(M), operand(N)
    expected = _int_product(ai, bi)
    mass = _int_product(np.abs(ai), np.abs(bi))
    assert mass.max() < 2 ** 24, int(mass.max())
    share = float(((mass >= 2 ** 23) & (expected % 2 != 0)).mean())
    assert share >= WIDE_MIN_SHARE, share
    a, b = _check_fmt(fmt, ai, bi)
    return _frozen(a, b, expected)


def k_pick(M, K):
    return (37 * np.arange(M) + 11) % K


@functools.lru_cache(maxsize=None)
def k_pairing(shape, fmt="bf16"):
    """The k-pairing and orientation probe.  A has one 1 per row, at
    k = (37m + 11) % K; B is asymmetric in n and k, so C[m][n] must be
    B[n][pick(m)]: a lane map that pairs A's k with another k of B fails, and
    so does a C store with row and column swapped.  B's values are an odd
    integer times a power of two: 8 significant bits for bf16, all 24 for fp32
    (odd integers just below 2^24), so any truncation or rounding of an fp32
    operand fails exactly too."""
    M, N, K = shape
    a = np.zeros((M, K), np.float32)
    pick = k_pick(M, K)
    a[np.arange(M), pick] = 1
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    if fmt == "bf16":
        mant = 129 + 2 * ((3 * n + 5 * k) % 64)               # odd, 129 … 255
    else:
        mant = 2 ** 24 - 1 - 2 * ((3 * n + 5 * k) % 4093)     # odd, just below 2^24
    sign = np.where((n + 2 * k) % 3 == 0, -1.0, 1.0)
    bv = sign * np.ldexp(mant.astype(np.float64), (n + 2 * k) % 13 - 6)
    assert (bv[:, 0::2] != bv[:, 1::2]).all()  # k and k^1 are told apart everywhere
    a, b = _check_fmt(fmt, a, bv)
    assert np.array_equal(b.astype(np.float64), bv)
    return _frozen(a, b, bv[:, pick].T.copy())


RANGE_KINDS = ("large", "subnormal")
# (|a|, |b|) per format and kind
RANGE_MAGS = {("bf16", "large"): (2.0 ** 63, 2.0 ** 63), ("bf16", "subnormal"): (2.0 ** -130, 2.0 ** 100),
              ("f32", "large"): (2.0 ** 63, 2.0 ** 63), ("f32", "subnormal"): (2.0 ** -140, 2.0 ** 110)}
RANGE_LARGE_TERMS = 3  # non-zero k per row of B in the "large" kind


@functools.lru_cache(maxsize=None)
def range_ends(shape, seed=5, fmt="bf16", kind="large"):
    """±1 sign patterns times a magnitude; expected = count · |a|·|b|.

    "large": products of ±2^126.  Four of them already overflow fp32 in some
    summation order, so B keeps RANGE_LARGE_TERMS signs per row (at k that
    vary with n and span K) and zeros elsewhere: Σ|a·b| <= 3·2^126 and every
    partial sum stays finite in any order.
    "subnormal": A holds subnormal values of its format (bf16 ±2^-130, fp32
    ±2^-140) against ±2^100 / ±2^110 in B: the products are ±2^-30 and every
    sum is a multiple of 2^-30 below 2^-20, exact.  Inputs flushed to zero
    would give 0."""
    M, N, K = shape
    rng = np.random.default_rng(seed + sum(shape))
    ma, mb = RANGE_MAGS[fmt, kind]
    sa = rng.choice([-1.0, 1.0], (M, K))
    sb = rng.choice([-1.0, 1.0], (N, K))
    if kind == "large":
        keep = np.zeros((N, K), bool)
        for j in range(RANGE_LARGE_TERMS):
            keep[np.arange(N), (j * K // RANGE_LARGE_TERMS + 7 * np.arange(N) + j) % K] = True
        sb = np.where(keep, sb, 0.0)
    count = sa @ sb.T
    assert np.abs(count).max() > 0
    expected = count * (ma * mb)
    assert np.isfinite(expected).all() and (np.abs(sa) @ np.abs(sb).T).max() * (ma * mb) < 2.0 ** 128
    a, b = _check_fmt(fmt, sa * ma, sb * mb)
    assert np.array_equal(a.astype(np.float64), sa * ma) and np.array_equal(b.astype(np.float64), sb * mb)
    return _frozen(a, b, expected)


FINITE, POS_INF, NEG_INF, NAN = 0, 1, 2, 3
SIGNALLING_NAN = np.uint32(0x7F800001)


@functools.lru_cache(maxsize=None)
def nonfinite(shape, fmt="bf16"):
    """Integers in [-8, 8] with one +Inf in A at (m1, k1), k1 in the first
    K-tile (the first K-split, the helper's range), and one NaN in A at
    (m2, k2), k2 in the last K-tile (the last K-split, the owner's range).  B
    has exact zeros in those two columns.  Returns (a, b, (cls, expected)):
    cls[m][n] is the class every element must have — row m1 ±Inf by the sign
    of b[n][k1] and NaN where it is 0, row m2 all NaN, every other element
    FINITE and equal to `expected` (the int64 product of the finite data)."""
    M, N, K = shape
    rng = np.random.default_rng(11 + sum(shape))
    ai = rng.integers(-8, 9, (M, K))
    bi = rng.integers(-8, 9, (N, K))
    m1, k1, m2, k2 = 3, 5, M - 6, K - 3
    assert m1 != m2 and k1 < 32 and k2 >= K - 32
    bi[::5, k1] = 0
    bi[2::7, k2] = 0
    assert (bi[:, k1] > 0).any() and (bi[:, k1] < 0).any()
    a = ai.astype(np.float32)
    a[m1, k1] = np.inf
    # a signalling NaN with the lowest payload bit only (0x7F800001): an
    # encoder that adds its rounding increment to it returns +Inf
    a.view(np.uint32)[m2, k2] = SIGNALLING_NAN
    assert np.isnan(a[m2, k2])
    ai[m1, k1] = ai[m2, k2] = 0
    expected = _int_product(ai, bi)
    cls = np.full((M, N), FINITE, np.int8)
    cls[m1] = np.where(bi[:, k1] > 0, POS_INF, np.where(bi[:, k1] < 0, NEG_INF, NAN))
    cls[m2] = NAN
    b = bi.astype(np.float32)
    if fmt == "bf16":
        ok = np.isfinite(a)
        _check_fmt(fmt, np.where(ok, a, 0), b)
        assert gemm.from_bf16_bits(gemm.to_bf16_bits(a))[m1, k1] == np.inf
        assert np.isnan(gemm.from_bf16_bits(gemm.to_bf16_bits(a))[m2, k2])
    cls.setflags(write=False)
    expected.setflags(write=False)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b, (cls, expected)


ROW_SCALE_EXP = 20


@functools.lru_cache(maxsize=None)
def row_scaled_random(shape, seed=3, fmt="bf16"):
    """uniform(-1, 1) operands (rounded to bf16 first for that format), every
    row of A and of B times its own power of two from 2^-20 … 2^20: exact, and
    far from overflow and underflow at these K.  expected is the float64
    product.  A whole-matrix max-norm sees only the largest rows of this."""
    M, N, K = shape
    rng = np.random.default_rng(seed + sum(shape))
    ops = []
    for rows in (M, N):
        x = rng.uniform(-1, 1, (rows, K)).astype(np.float32)
        if fmt == "bf16":
            x = gemm.from_bf16_bits(gemm.to_bf16_bits(x))
        ops.append(np.ldexp(x, rng.integers(-ROW_SCALE_EXP, ROW_SCALE_EXP + 1, (rows, 1))).astype(np.float32))
    a, b = _check_fmt(fmt, *ops)
    return _frozen(a, b, a.astype(np.float64) @ b.astype(np.float64).T)


@functools.lru_cache(maxsize=None)
def old_uniform_case(shape, seed=0):
    """The operands GemmF32(fill="random", seed=0) draws: what the max-norm
    tests of test_gpu_basic.py run on."""
    M, N, K = shape
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, M * K).astype(np.float32).reshape(M, K)
    b = rng.uniform(-1, 1, N * K).astype(np.float32).reshape(N, K)
    return _frozen(a, b, a.astype(np.float64) @ b.astype(np.float64).T)


def old_f32_formula_passes(c, ref, K) -> bool:
    """test_gemm_f32_matches_fp64's comparison."""
    return bool(np.abs(c - ref).max() < 1e-4 * np.sqrt(K) * max(1.0, np.abs(ref).max()))


# --------------------------------------------------------------------------- comparisons

def accumulation_bound(a, b, unit):
    """K · unit · (|a| · |b|ᵀ), per element, float64.

    unit = 2^-24 (fp32): the fp32 matrix-core result is a k-ordered fma chain,
    one rounding to nearest per step; K such roundings bound the error of a
    dot product by K·u·Σ|a·b| with no higher-order term (Jeannerod and Rump,
    "Improved error bounds for inner products in floating-point arithmetic",
    2013).
    unit = 2^-23 (bf16): the products of two bf16 values are exact in fp32;
    what remains is at most K fp32 additions in some order, each off by at
    most one unit in the last place of a partial sum of magnitude <= Σ|a·b|
    (the adder inside the 32-deep instruction is not documented, so one that
    truncates is allowed for) — the argument and the constant of the fp8 tests."""
    K = np.shape(a)[1]
    return K * unit * (np.abs(np.asarray(a, np.float64)) @ np.abs(np.asarray(b, np.float64)).T)


def assert_exact(c, expected):
    """C is float32 and equals `expected` element for element (no tolerance;
    NaN equals nothing); reports the first mismatches."""
    assert c.dtype == np.float32, c.dtype
    assert c.shape == expected.shape, (c.shape, expected.shape)
    bad = np.argwhere(c.astype(np.float64) != expected)
    assert bad.size == 0, (f"{len(bad)} of {c.size} elements differ; first at {bad[:4].tolist()}: got "
                           f"{[float(c[tuple(i)]) for i in bad[:4]]}, expected "
                           f"{[float(expected[tuple(i)]) for i in bad[:4]]}")


def classify(c):
    return np.where(np.isnan(c), NAN, np.where(c == np.inf, POS_INF, np.where(c == -np.inf, NEG_INF, FINITE))).astype(np.int8)


def assert_nonfinite(c, want):
    """The comparison of the `nonfinite` case: every element in its class,
    the finite ones equal to the integer product."""
    cls, expected = want
    assert c.dtype == np.float32 and c.shape == cls.shape
    got = classify(c)
    bad = np.argwhere(got != cls)
    assert bad.size == 0, (f"{len(bad)} elements in the wrong class (0 finite, 1 +inf, 2 -inf, 3 nan); first at "
                           f"{bad[:4].tolist()}: got {[int(got[tuple(i)]) for i in bad[:4]]}, expected "
                           f"{[int(cls[tuple(i)]) for i in bad[:4]]}")
    fin = cls == FINITE
    wrong = np.argwhere(fin & (np.where(fin, c, 0).astype(np.float64) != expected))
    assert wrong.size == 0, (len(wrong), wrong[:4].tolist())


# --------------------------------------------------------------------------- emulators
# plain numpy, float32 values held in float64

def _f32(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return x.astype(np.float32).astype(np.float64)


def _dot(a, b):
    """a · bᵀ in float64.  Rows of `a` with a non-finite value go element by
    element (0·Inf = NaN, as IEEE has it), whatever the BLAS does with them."""
    assert np.isfinite(b).all()
    odd = ~np.isfinite(a).all(axis=1)
    if not odd.any():
        return a @ b.T
    out = np.where(odd[:, None], 0.0, a) @ b.T
    with np.errstate(invalid="ignore"):
        for m in np.flatnonzero(odd):
            out[m] = (a[m][None, :] * b).sum(axis=1)
    return out


def _ops64(a, b):
    with np.errstate(invalid="ignore"):  # widening the signalling NaN of `nonfinite` raises the flag
        return np.asarray(a, np.float64), np.asarray(b, np.float64)


def emu_chain_f32(a, b):
    """The fp32 matrix-core result: one k-ordered chain acc = fl(a_k·b_k + acc)
    (product exact in float64, one rounding to fp32 per step)."""
    a, b = _ops64(a, b)
    acc = np.zeros((a.shape[0], b.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(a.shape[1]):
            acc = _f32(acc + a[:, k, None] * b[None, :, k])
    return acc.astype(np.float32)


def emu_chunked(a, b, k0=0, k1=None, chunk=32, ktile=64, after_ktile=None):
    """The bf16 structure: the fp32 accumulator takes one 32-deep sum per
    instruction (summed wide, rounded once), K-tile after K-tile over
    [k0, k1).  `after_ktile` (mutants): applied to the accumulator after every
    K-tile."""
    a, b = _ops64(a, b)
    k1 = a.shape[1] if k1 is None else k1
    acc = np.zeros((a.shape[0], b.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(k0, k1, ktile):
            for c in range(t, min(t + ktile, k1), chunk):
                acc = _f32(acc + _dot(a[:, c:c + chunk], b[:, c:c + chunk]))
            if after_ktile is not None:
                acc = after_ktile(acc)
    return acc.astype(np.float32)


def emu_split_k(a, b, S, partial=None, **kw):
    """Split-K: S partial tiles in fp32 (the workspace W), the last arrival
    adds the others' to its own in fp32.  `partial` (mutants): applied to the
    partials the workspace holds."""
    K = np.shape(a)[1]
    assert (K // 64) % S == 0
    parts = [emu_chunked(a, b, s * K // S, (s + 1) * K // S, **kw).astype(np.float64) for s in range(S)]
    acc = parts[-1]
    with np.errstate(invalid="ignore"):
        for p in parts[:-1]:
            acc = _f32(acc + (p if partial is None else partial(p)))
    return acc.astype(np.float32)


def emu_handover(a, b, helper_ktiles, partial=None, **kw):
    """The uneven owner/helper split: the helper multiplies the first
    `helper_ktiles` K-tiles and hands its fp32 partial over, the owner adds it
    to its own."""
    K = np.shape(a)[1]
    cut = helper_ktiles * 64
    assert 0 < cut < K
    helper = emu_chunked(a, b, 0, cut, **kw).astype(np.float64)
    owner = emu_chunked(a, b, cut, K, **kw).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return _f32(owner + (helper if partial is None else partial(helper))).astype(np.float32)


def through_device_layout(c, BM, BN, geom, group_m=4, mutate=None):
    """Row-major C → the buffer a kernel writes (tile-major in the kernels'
    grouped tile order, fragment order inside a tile when `geom` is given,
    through ops.gemm.rows_to_tile) → row-major again through ops.gemm.untile,
    as GemmBf16.result() does.  `mutate` (mutants) acts on the flat buffer."""
    M, N = c.shape
    ntm, ntn = M // BM, N // BN
    tm, tn = gemm.tile_coords(np.arange(ntm * ntn), M, N, BM, BN, group_m)
    blocks = c.reshape(ntm, BM, ntn, BN).transpose(0, 2, 1, 3)[tm, tn]
    buf = blocks.reshape(ntm * ntn, BM * BN) if geom is None else gemm.rows_to_tile(blocks, geom)
    buf = np.ascontiguousarray(buf).reshape(-1).copy()
    if mutate is not None:
        buf = mutate(buf)
    return gemm.untile(buf, M, N, BM, BN, group_m, geom)


# --------------------------------------------------------------------------- the cases by name

EXACT_CASES = ("exact_integers", "wide_integers", "k_pairing", "range_large", "range_subnormal", "nonfinite")


def build(case, shape, fmt):
    """(a, b, want) of a named case; `want` is what check() compares with."""
    if case == "exact_integers":
        return exact_integers(shape, None, fmt)
    if case == "wide_integers":
        return wide_integers(shape, 0, fmt)
    if case == "k_pairing":
        return k_pairing(shape, fmt)
    if case in ("range_large", "range_subnormal"):
        return range_ends(shape, 5, fmt, case[len("range_"):])
    if case == "nonfinite":
        return nonfinite(shape, fmt)
    if case == "row_scaled_random":
        return row_scaled_random(shape, 3, fmt)
    raise ValueError(case)


def check(case, c, a, b, want, fmt):
    """The comparison of a named case: `==` for the exact ones, the derived
    bound for row_scaled_random (returns the worst err / bound)."""
    if case == "nonfinite":
        return assert_nonfinite(c, want)
    if case == "row_scaled_random":
        return check_within_bound(c, want, accumulation_bound(a, b, UNIT[fmt]), case)
    return assert_exact(c, want)
