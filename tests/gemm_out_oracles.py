"""Designed fp32 accumulator bits for the output epilogue of the MX GEMMs
(kernels/gemm8_out.h behind kernels/sgemm_mx_out.hip), and the operands that
make the GEMM itself produce them, in the manner of gemm8_oracles.py.

No GPU use: the CPU tier (test_gemm_out_oracles.py) checks the construction
and shows that the data rejects each named wrong epilogue; the GPU tier
(test_gpu_gemm_mx_out.py) runs the plain and the output-mode kernels on the
operands and compares bit for bit.

The accumulator cannot be set directly, but the GEMM can produce any chosen
fp32 bit pattern exactly.  The scaled matrix instructions align and cut only
the products of 8 neighbouring k; everything else is added exactly in fp32,
denormals included (measured: profiles/gemm8_specials.md).  So every target
value is written as  sign · Σ_j d_j · 2^(p_j)  with small integer digits d_j
(0..15 for e4m3 operands, 0..3 for e2m1 ones: exact codes of the format) over
non-overlapping windows of 4 (2) bits:

* piece j of column n has the private position k = j·N + n;
* Bt is one-hot there: Bt[n][j·N + n] = 1, everything else 0;
* A[m][j·N + n] = ±d_j of C[m][n];
* the exponent is in the two E8M0 bytes of that K-block: ea + eb = p_j.  The
  32 columns of an output block share the K-block (j·N + n) / 32, so they
  share p_j: the windows are chosen per (row, output block), greedily from the
  top set bit of its 32 values, until every set bit is covered.

Every group of 8 neighbouring k then holds at most one non-zero product per
element of C (of at most 4 bits, nothing to cut), the pieces of one element
lie N >= 128 apart, and every partial sum is a subset of the target's bits: an
fp32 value, whatever the order of the additions.

eb belongs to a row of Bt and is therefore the same for every row m, while
p_j spans [-149, 124], more than one byte's [-127, 127].  So the J slots have
fixed kinds: slot 0 has eb = 127, then come slots of eb = -22 (windows
down to 2^-149) and slots of eb = 0 (windows up to 2^124); a block's windows
are dealt to the slots whose range holds them.

Specials.  ±Inf: one piece of the format's largest element (448, 6) in slot 0
under byte 254 times byte 254.

NaN.  A GEMM cannot make a single element of C NaN.  A NaN operand (an e4m3
NaN code, a scale byte 0xFF) makes a whole row or column of C NaN through
0·NaN, and Inf − Inf does not happen: with +448·2^254 in one K-step and
−448·2^254 in a later one the kernels return +Inf, not NaN (MI355X,
2026-10-21, both formats, both tiles: every such site held 0x7F800000 and every
other element of the target was exact).  The instruction adds its products to
the accumulator before anything is rounded to fp32, so the second product is
a large finite number beside a true Inf; only the accumulator ever holds an
Inf.  So the single NaN elements of designed_rows() stay with the CPU tier,
and the target the GPU tier builds (gpu_target) has +0 in their places and
whole NaN columns instead (NAN_COLUMNS, byte 0xFF on one block of that row of
Bt): every row then has exactly one NaN in the finite designed block the
column crosses, in each of the four lanes that hold an MXFP4 block and in
both bytes of a wave's scale word.  Sign and payload of those NaNs are the
hardware's (0xFFC00000 in every probe so far), so NaN-ness is what is
compared.

−0 cannot be reached: every product of a zero digit is +0 (the digits are
integers, the one-hot element is +1) and a sum that starts at +0 never gives
−0 under round-to-nearest; designed_accumulators() holds +0 in its place and
the host model (test_gemm_mx_out_host.py) keeps covering −0.
"""
from __future__ import annotations

import functools

import numpy as np

from cekirdekler_amd.ops.gemm import unpack_fp4
from test_gemm_mx_out_host import designed_rows, relu

RADIX_BITS = {"mxfp8": 4, "mxfp4": 2}     # bits of a digit: 0..15 are exact in e4m3, 0..3 in e2m1
J_CAP = {"mxfp8": 16, "mxfp4": 32}        # pieces per element: K = J·N
K_TILE = {"mxfp8": 128, "mxfp4": 256}     # the classes' K_MULTIPLE
BIGGEST = {"mxfp8": 448, "mxfp4": 6}      # the element whose product under 254 + 254 overflows
EB_INF, EB_LOW, EB_MID = 127, -22, 0      # eb of the three kinds of slot
INF_SLOTS = 1
E8M0_NAN = 0xFF
HW_NAN = np.uint32(0xFFC00000)            # the NaN the scaled matrix instructions return
P_MIN = -149                              # 2^-149: fp32's last bit
NO_WINDOW = -1000
# (M, N) of the GPU tier per tile: two tile rows, one tile column
SHAPES = {"256x256pbx": (512, 256), "128x128": (256, 128)}
# NaN columns of the GPU tier's target: (block, lane of 8 columns) = (1, 0), (2, 3), (5, 1), (6, 2) and (0, 3),
# (2, 1).  Under place() every designed block also lies in a block that no NaN column crosses.
NAN_COLUMNS = {"256x256pbx": (37, 94, 172, 213), "128x128": (30, 76)}

_SIGN, _ABS, _INF = np.uint32(0x80000000), np.uint32(0x7FFFFFFF), np.uint32(0x7F800000)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _bf16_rows():
    """uint32 [32][128]: the rows aimed at the bf16 rounding, all positive.
    Rows 0-7 ties at bit 15 with an even and an odd kept mantissa (and the
    all-ones one, which carries into the exponent), each ± 1 ulp, at exponent
    fields from 1 to 253; 8-11 the same lows around 1.0 (0x3F7FFFFF carries to
    1.0); 12-15 the smallest and the largest denormal, ties among denormals,
    the smallest normal ± 1 ulp; 16-23 the edge of Inf (0x7F7F7FFF stays,
    0x7F7F8000 and above round to Inf); 24-31 seeded values over the whole
    exponent range with a third of the low halves forced onto a tie ± 1 ulp.
    Every block is filled up with seeded values of the neighbouring binades,
    so that it has an ordinary maximum; a block's cases start at column 8·b,
    so that they meet different lanes."""
    rng = np.random.default_rng(2027)
    u = np.zeros((32, 4, 32), np.uint32)
    lows = (0x7FFF, 0x8000, 0x8001)

    def fill(field):
        """32 seeded values with exponent fields field-3 .. field+1 (within 1 .. 254)."""
        f = np.clip(field + rng.integers(-3, 2, 32), 1, 254).astype(np.uint32)
        return (f << np.uint32(23)) | rng.integers(0, 1 << 23, 32).astype(np.uint32)

    def put(r, b, cases, field):
        row = fill(field)
        cases = np.asarray(cases, np.uint32)
        assert len(cases) <= 28
        row[(8 * b + np.arange(len(cases))) % 32] = cases
        u[r, b] = row

    for i, field in enumerate((1, 60, 100, 126, 127, 128, 200, 253)):
        for b in range(4):
            hms = (0, 1, 2 + 2 * b, 3 + 2 * b, 0x7E, 0x7F, 0x40, 0x55)
            put(i, b, [(field << 23) | (hm << 16) | lo for hm in hms for lo in lows], field)
    around_one = [0x3F7FFFFF, 0x3F7F8000, 0x3F7F7FFF, 0x3F7F8001, 0x3FFFFFFF, 0x3FFF8000, 0x3F800000, 0x3F808000,
                  0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F000001, 0x3EFFFFFF, 0x3F7E8000, 0x3F7D8000]
    for i in range(4):
        for b in range(4):
            put(8 + i, b, np.roll(around_one, i + b), 127)
    tiny = [0x00000001, 0x007FFFFF, 0x00800000, 0x00800001, 0x007FFFFE, 0x00008000, 0x00018000, 0x00007FFF,
            0x00008001, 0x00017FFF, 0x00018001, 0x007F8000, 0x007F7FFF, 0x00808000, 0x00818000, 0x00010000]
    for i in range(4):
        for b in range(4):
            put(12 + i, b, np.roll(tiny, i + b), 1 + (i + b) % 2)
    edge = [0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0x7F7F8001, 0x7F7E8000, 0x7F7EFFFF, 0x7F7E7FFF, 0x7F7F0000,
            0x7F000000, 0x7EFFFFFF, 0x7EFF8000]
    for i in range(8):
        for b in range(4):
            put(16 + i, b, np.roll(edge, i + b)[:3 + i + b], 254 - (i + b) % 3)
    for i in range(8):
        for b in range(4):
            row = fill(int(rng.integers(20, 236)))
            tie = rng.random(32) < 1 / 3
            row[tie] = (row[tie] & np.uint32(0xFFFF0000)) | rng.choice(lows, int(tie.sum())).astype(np.uint32)
            u[24 + i, b] = row
    return u.reshape(32, 128)


@functools.lru_cache(maxsize=None)
def designed_accumulators():
    """fp32 [128][128].  Rows 0..63: designed_rows() of the host tier with
    every −0 replaced by +0 (see the module docstring).  Rows 64..95:
    _bf16_rows(); rows 96..127 the same negated, for ReLU and the sign."""
    d = np.empty((128, 128), np.uint32)
    d[:64] = _bits(designed_rows())
    d[:64][d[:64] == _SIGN] = 0
    d[64:96] = _bf16_rows()
    d[96:] = d[64:96] | _SIGN
    assert not (d == _SIGN).any()
    out = d.view(np.float32)
    out.setflags(write=False)
    return out


def place(D, M, N):
    """D ([128][128] fp32) tiled over [M][N].  The copy in band b of 128 rows
    and column copy c has its rows rolled by 5b + 3c and its four 32-column
    blocks rotated by b + c, and is negated for odd c (zeros stay +0): every
    designed block is stored as the low and as the high byte of a wave's
    scale word, in different rows of a 16-row strip (both lane-to-row maps of
    the epilogue, q·4 + lane/16 and q·8 + lane/8), in different waves and
    under both signs."""
    D = np.ascontiguousarray(D, np.float32)
    assert D.shape == (128, 128) and M % 128 == 0 and N % 128 == 0
    out = np.empty((M, N), np.uint32)
    for b in range(M // 128):
        for c in range(N // 128):
            t = np.roll(np.roll(D, 5 * b + 3 * c, axis=0).reshape(128, 4, 32), b + c, axis=1).reshape(128, 128)
            u = _bits(t).copy()
            if c & 1:
                u[(u & _ABS) != 0] ^= _SIGN
            out[128 * b:128 * b + 128, 128 * c:128 * c + 128] = u
    return out.view(np.float32)


@functools.lru_cache(maxsize=None)
def placed_target(tile):
    """place(designed_accumulators(), M, N) at the GPU tier's shape of ``tile``, read-only."""
    t = place(designed_accumulators(), *SHAPES[tile])
    t.setflags(write=False)
    return t


def reachable(target, nan_columns):
    """``target`` as a GEMM can build it (module docstring): +0 at its NaN
    sites, then the whole columns ``nan_columns`` NaN."""
    u = _bits(target).copy()
    u[(u & _ABS) > _INF] = 0
    u[:, list(nan_columns)] = HW_NAN
    return u.view(np.float32)


@functools.lru_cache(maxsize=None)
def gpu_target(tile):
    """reachable(placed_target(tile), NAN_COLUMNS[tile]): what the GPU tier builds and converts, read-only."""
    t = reachable(placed_target(tile), NAN_COLUMNS[tile])
    t.setflags(write=False)
    return t


def classes(target):
    """(finite, inf, nan) masks of an fp32 array by its bits."""
    a = _bits(target) & _ABS
    return a < _INF, a == _INF, a > _INF


def assert_designed_cases_present(stored, target, out, act):
    """The designed cases as they must show in a stored output ``(Y, SY,
    packed)`` of ``target`` ([M][N] fp32), so that a comparison on this data
    cannot go vacuous.  bf16: an Inf that a finite value rounded to.  MXFP8:
    0x7E from saturation (a scaled value beyond 448, not an Inf), subnormal
    codes, a 0x7F in a block that has finite non-zero values beside it.
    MXFP4: byte 0xFF over a block with a single NaN and over blocks whose
    other codes are not all zero.  Without ReLU the signed cases occur under
    both signs; under ReLU no sign bit is stored outside the NaN sites."""
    M, N = target.shape
    t = relu(target) if act == "relu" else np.ascontiguousarray(target, np.float32)
    fin, _, nan = classes(t)
    neg = (_bits(t) & _SIGN) != 0
    signs = (False,) if act == "relu" else (False, True)
    Y = np.asarray(stored[0]).reshape(M, -1)
    blocks = lambda x: x.reshape(M, N // 32, 32)  # noqa: E731
    if out == "bfloat16":
        to_inf = fin & ((Y & 0x7FFF) == 0x7F80)
        for s in signs:
            assert (to_inf & (neg == s)).any(), ("no finite value rounded to Inf", s)
        sign = Y & 0x8000
    elif out == "mxfp8":
        e = np.asarray(stored[1]).reshape(M, N // 32).astype(np.int64) - 127
        scaled = np.abs(np.ldexp(np.where(fin, t, 0).astype(np.float64), -np.repeat(e, 32, axis=1)))
        sat = fin & ((Y & 0x7F) == 0x7E) & (scaled > 448)
        for s in signs:
            assert (sat & (neg == s)).any(), ("no saturated code", s)
        assert (fin & ((Y & 0x78) == 0) & ((Y & 7) != 0)).any(), "no e4m3 subnormal code"
        beside = np.repeat(blocks(fin & (t != 0)).any(axis=2), 32, axis=1)
        assert (nan & (Y == 0x7F) & beside).any(), "no 0x7F beside finite values"
        sign = Y & 0x80
    else:
        codes = unpack_fp4(Y)
        ff = np.asarray(stored[1]).reshape(M, N // 32) == 0xFF
        assert (ff & (blocks(nan).sum(axis=2) == 1)).any(), "no 0xFF over a block with a single NaN"
        assert (ff & (blocks((codes & 7) != 0).sum(axis=2) > 0)).any(), "no 0xFF over non-zero codes"
        sign = codes & 8
    if act == "relu":
        assert (sign[~nan] == 0).all(), "a sign bit under ReLU"
    else:
        assert (sign[~nan] != 0).any()


def _magnitudes(target):
    """|target| = mant · 2^e in integers ([M][N/32][32] int64 each); mant = 0
    at Inf and NaN sites."""
    u = _bits(target)
    field = ((u >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64)
    frac = (u & np.uint32(0x7FFFFF)).astype(np.int64)
    mant = np.where(field == 0, frac, frac | (1 << 23))
    mant = np.where(field == 255, 0, mant)
    e = np.where(field == 0, P_MIN, field - 150)
    M, N = target.shape
    return mant.reshape(M, N // 32, 32), e.reshape(M, N // 32, 32)


def windows(target, bits):
    """The greedy windows of every (row, output block): ``p`` [M][N/32][W]
    (NO_WINDOW where a block needs fewer than W) and the digits ``d``
    [M][N/32][W][32], 0 <= d < 2^bits, with  |target| = Σ_w d·2^p  at every
    finite site.  Each window starts at the top bit still uncovered among the
    block's 32 values and reaches ``bits`` bits down (not below 2^-149)."""
    rem, e = _magnitudes(target)
    ps, ds = [], []
    while rem.any():
        length = np.frexp(rem.astype(np.float64))[1]  # bit length: rem < 2^24
        top = np.where(rem > 0, e + length - 1, NO_WINDOW).max(axis=2)
        active = top > NO_WINDOW
        p = np.where(active, np.maximum(top - (bits - 1), P_MIN), NO_WINDOW)
        s = p[..., None] - e  # the window's lowest bit within mant
        d = np.where(s >= 0, rem >> np.clip(s, 0, 62), rem << np.clip(-s, 0, bits))
        d = np.where(active[..., None], d, 0)
        assert d.max() < (1 << bits)
        rem = np.where(active[..., None], np.where(s > 0, rem & ((1 << np.clip(s, 0, 62)) - 1), 0), rem)
        ps.append(p)
        ds.append(d)
    return np.stack(ps, axis=2), np.stack(ds, axis=2).astype(np.int16)


def slot_exponents(J, n_low):
    """eb of the J slots: INF_SLOTS of EB_INF, ``n_low`` of EB_LOW, the rest EB_MID."""
    eb = np.full(J, EB_MID, np.int64)
    eb[:INF_SLOTS] = EB_INF
    eb[INF_SLOTS:INF_SLOTS + n_low] = EB_LOW
    return eb


def _deal(p, need_inf, eb):
    """Slots for one block's windows ``p`` (descending): a list of slot
    indices, or None if they do not fit.  Windows that only one kind of slot
    holds go first."""
    free = [j for j in range(len(eb)) if j >= need_inf]
    fits = lambda j, pw: -127 <= pw - eb[j] <= 127  # noqa: E731
    order = sorted(range(len(p)), key=lambda w: sum(fits(j, p[w]) for j in free))
    got = [None] * len(p)
    for w in order:
        # a window takes an eb = 127 slot last: those are the scarce ones
        for j in sorted(free, key=lambda j: (eb[j] == EB_INF, j)):
            if fits(j, p[w]):
                got[w] = j
                free.remove(j)
                break
        else:
            return None
    return got


@functools.lru_cache(maxsize=None)
def decompose_tile(tile, fmt):
    """decompose(gpu_target(tile), fmt), once per (tile, format), read-only."""
    out = decompose(gpu_target(tile), fmt)
    for x in out[:4]:
        x.setflags(write=False)
    return out


def decompose(target, fmt):
    """Operands whose MX GEMM is ``target`` (fp32 [M][N]) bit for bit, NaN at
    its NaN sites, which must be whole columns: ``(a, b, ea, eb, J)`` with K =
    J·N, as _set_ints of test_gpu_gemm_mx_out.py takes them.  ``a`` [M][K] and
    ``b`` [N][K] are integers that are exact codes of ``fmt``, ``ea``
    [M][K/32] and ``eb`` [N][K/32] exponents in [-127, 127]; a NaN column n
    has eb = 128 (byte 0xFF) on its block n / 32 of slot 0 and no piece.  J is
    the largest number of pieces a block needs (its windows, plus one slot if
    it holds an Inf), raised until K is a whole number of K-tiles and every
    block's windows fit the slots' ranges; it must not exceed J_CAP.  No
    element is left out."""
    target = np.ascontiguousarray(target, np.float32)
    M, N = target.shape
    NB, bits, big = N // 32, RADIX_BITS[fmt], BIGGEST[fmt]
    assert not (_bits(target) == _SIGN).any(), "-0 cannot be reached"
    fin, inf, nan = classes(target)
    nan_columns = np.flatnonzero(nan.any(axis=0))
    assert nan[:, nan_columns].all(), "a GEMM makes whole columns NaN, not single elements"
    p, d = windows(target, bits)
    count = (p > NO_WINDOW).sum(axis=2)
    need_inf = inf.reshape(M, NB, 32).any(axis=2).astype(np.int64)
    n_low = int(((p > NO_WINDOW) & (p < EB_MID - 127)).sum(axis=2).max())  # windows only EB_LOW reaches
    J = int((count + need_inf).max())
    while True:
        while (J * N) % K_TILE[fmt]:
            J += 1
        assert J <= J_CAP[fmt], (fmt, J, "a designed value needs too many pieces: change the value, not the cap")
        slot_eb = slot_exponents(J, min(n_low, J - INF_SLOTS))
        deals = {}
        for m in range(M):
            for nb in range(NB):
                key = (tuple(p[m, nb, :count[m, nb]].tolist()), int(need_inf[m, nb]))
                if key not in deals:
                    deals[key] = _deal(key[0], key[1], slot_eb)
        if all(v is not None for v in deals.values()):
            break
        J += 1
    sign = np.where(_bits(target) & _SIGN, -1, 1).astype(np.int16).reshape(M, NB, 32)
    a = np.zeros((M, J, NB, 32), np.int16)
    ea = np.zeros((M, J, NB), np.int64)
    for m in range(M):
        for nb in range(NB):
            c = int(count[m, nb])
            for w, j in enumerate(deals[tuple(p[m, nb, :c].tolist()), int(need_inf[m, nb])]):
                a[m, j, nb] = sign[m, nb] * d[m, nb, w]
                ea[m, j, nb] = p[m, nb, w] - slot_eb[j]
            ea[m, :need_inf[m, nb], nb] = EB_INF
    a = a.reshape(M, J, N)
    a[:, 0][inf] = np.where(_bits(target)[inf] & _SIGN, -big, big)
    assert not a.transpose(0, 2, 1)[nan].any()
    b = np.zeros((N, J, N), np.int16)
    b[np.arange(N), :, np.arange(N)] = 1
    eb = np.broadcast_to(slot_eb[None, :, None], (N, J, NB)).copy()
    assert np.abs(ea).max() <= 127 and np.abs(eb).max() <= 127
    eb[nan_columns, 0, nan_columns // 32] = E8M0_NAN - 127
    return a.reshape(M, J * N), b.reshape(N, J * N), ea.reshape(M, J * NB), eb.reshape(N, J * NB), J
