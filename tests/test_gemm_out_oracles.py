"""CPU tier of gemm_out_oracles.py: the designed accumulator bits hold what
they claim, place() puts every designed block where it says, gpu_target()
differs from that only where a GEMM cannot follow, decompose() builds
operands whose exact sum is that target (codes, scale bytes, one-hot Bt, one
product per group of 8 k, partial sums, Inf pieces and NaN columns, the host
references), and both targets reject each named wrong epilogue: a numpy codec
with that one error stores something else than host_codec does.  Every
comparison is exact."""
import numpy as np
import pytest

import cekirdekler_amd as ck
import gemm_out_oracles as goo
from cekirdekler_amd.ops.gemm import (MX_OUTPUTS, GemmMxFp4, GemmMxFp8, from_fp4_e2m1_codes, from_fp8_e4m3_bits,
                                      pack_fp4, pack_mx_scales, to_fp4_e2m1_codes, to_fp8_e4m3_bits)
from cekirdekler_amd.ops.quantize import gemm_out_model
from gemm8_oracles import emu_gemm8
from test_gemm_mx_out_host import assert_same_output, designed_rows, host_codec

FORMATS = {"mxfp8": GemmMxFp8, "mxfp4": GemmMxFp4}
TILES = tuple(goo.SHAPES)
ACTS = (None, "relu")
SIGN, ABS, INF = np.uint32(0x80000000), np.uint32(0x7FFFFFFF), np.uint32(0x7F800000)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ------------------------------------------------------------------ 1: the data


def test_designed_accumulators_hold_what_they_claim():
    d = bits(goo.designed_accumulators())
    assert d.shape == (128, 128) and not (d == SIGN).any()
    rows = bits(designed_rows())
    np.testing.assert_array_equal(d[:64], np.where(rows == SIGN, 0, rows))
    assert (rows == SIGN).any()  # the replacement had something to do
    np.testing.assert_array_equal(d[96:], d[64:96] | SIGN)
    have = set(d[64:96].ravel().tolist())
    for u in (0x3F7FFFFF, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0x00000001, 0x007FFFFF, 0x00800000, 0x00800001):
        assert u in have and (u | 0x80000000) in set(d[96:].ravel().tolist()), hex(u)
    # ties at bit 15 with an even and an odd kept mantissa, each with both neighbours, in every block of rows 64..71
    t = d[64:72].reshape(8, 4, 32)
    for odd in (0, 1):
        tie = ((t & 0xFFFF) == 0x8000) & (((t >> 16) & 1) == odd)
        assert tie.any(axis=2).all()
        for ulp in (1, -1):
            assert np.isin(t[tie].astype(np.int64) + ulp, t).all()
    # what the bf16 rounding has to get right
    b = host_codec(d.view(np.float32), "bfloat16")[0]
    fin = (d & ABS) < INF
    assert (fin & ((b & 0x7FFF) == 0x7F80)).sum() >= 32                    # finite → Inf
    assert (fin & ((d & ABS) >= 0x7F7F0000) & ((b & 0x7FFF) == 0x7F7F)).sum() >= 16  # … and its neighbours that stay
    denormal = ((d & ABS) < 0x00800000) & ((d & ABS) != 0)
    assert (denormal & ((b & 0x7FFF) == 0x0080)).any()                     # denormal → smallest normal
    assert ((d == 0x3F7FFFFF) & (b == 0x3F80)).any()                       # carry into the exponent
    # every block of the new rows has an ordinary maximum: finite and non-zero
    assert (np.where(fin, d & ABS, 0)[64:].reshape(64, 4, 32).max(axis=2) >= 0x00800000).all()


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("out", MX_OUTPUTS)
def test_model_equals_the_host_codecs_on_the_new_rows(out, act):
    """test_gemm_mx_out_host.py's comparison on the whole designed matrix."""
    d = goo.designed_accumulators()
    assert_same_output(gemm_out_model(d, out, act), host_codec(d, out, act), out, (out, act))


@pytest.mark.parametrize("tile", TILES)
def test_place(tile):
    M, N = goo.SHAPES[tile]
    d = bits(goo.designed_accumulators())
    t = bits(goo.place(d.view(np.float32), M, N))
    assert t.shape == (M, N) and M != N and not (t == SIGN).any()
    r, q = np.arange(128), np.arange(4)
    parities, strip_rows, wave_cols = set(), set(), set()
    for b in range(M // 128):
        for c in range(N // 128):
            rows = 128 * b + (r + 5 * b + 3 * c) % 128
            blk = (q + b + c) % 4
            got = t[rows][:, 128 * c:128 * c + 128].reshape(128, 4, 32)[:, blk]
            want = d.reshape(128, 4, 32)
            if c & 1:
                want = np.where((want & ABS) != 0, want ^ SIGN, want)
            np.testing.assert_array_equal(got, want)
            parities.add(int(blk[0] & 1))       # designed block 0: low or high byte of the scale word
            strip_rows.add(int(rows[0] % 16))   # designed row 0: its row in the 16-row strip
            wave_cols.add(int((4 * c + blk[0]) // 2))
    assert parities == {0, 1} and len(strip_rows) >= 2
    assert len({s % 4 for s in strip_rows}) >= 2 and len({s % 8 for s in strip_rows}) >= 2
    if N > 128:  # column copies: another wave column, and both signs of every non-zero designed value
        assert len(wave_cols) >= 2
        assert np.isin(d[(d & ABS) != 0] ^ SIGN, t).all()
    assert np.isin(d, t).all()


@pytest.mark.parametrize("tile", TILES)
def test_gpu_target(tile):
    """What the GPU tier builds: the placed target with +0 at its single NaN
    elements and whole NaN columns instead, which leave every designed block
    whole somewhere and put a single NaN into finite blocks."""
    M, N = goo.SHAPES[tile]
    p, g = bits(goo.placed_target(tile)), bits(goo.gpu_target(tile))
    cols = np.array(goo.NAN_COLUMNS[tile])
    was_nan = (p & ABS) > INF
    keep = ~was_nan
    keep[:, cols] = False
    np.testing.assert_array_equal(g[keep], p[keep])
    assert (g[:, cols] == goo.HW_NAN).all()
    assert (np.delete(g, cols, axis=1)[np.delete(was_nan, cols, axis=1)] == 0).all()
    assert ((g & ABS) > INF).sum() == M * len(cols) and not (g == SIGN).any()
    # one column per block at the most; every designed (row, block) also lies, under either sign, in a block without one
    assert len(set((cols // 32).tolist())) == len(cols)
    d = bits(goo.designed_accumulators()).reshape(128, 4, 32)
    free = np.delete(np.arange(N // 32), cols // 32)
    whole = {blk.tobytes() for blk in g.reshape(M, N // 32, 32)[:, free].reshape(-1, 32)}
    for r in range(128):
        for q in range(4):
            if not ((d[r, q] & ABS) > INF).any():
                blk = d[r, q]
                assert blk.tobytes() in whole or np.where((blk & ABS) != 0, blk ^ SIGN, blk).tobytes() in whole, (r, q)
    # a single NaN beside finite non-zero values, in most rows
    nan = (g & ABS) > INF
    single = nan.reshape(M, N // 32, 32).sum(axis=2) == 1
    beside = (((g & ABS) < INF) & ((g & ABS) != 0)).reshape(M, N // 32, 32).any(axis=2)
    assert (single & beside).sum() > M * len(cols) * 3 // 4


def test_nan_columns_meet_every_lane_and_both_bytes():
    lanes = {(n % 32) // 8 for cols in goo.NAN_COLUMNS.values() for n in cols}
    assert lanes == {0, 1, 2, 3}
    assert {(n // 32) % 2 for n in goo.NAN_COLUMNS["256x256pbx"]} == {0, 1}
    assert {(n % 32) // 8 for n in goo.NAN_COLUMNS["256x256pbx"]} == {0, 1, 2, 3}


# ------------------------------------------------------------- 2: the operands


def _pieces(tile, fmt):
    """(a [M][J][N], exponent ea + eb of each piece [M][J][N], J)."""
    M, N = goo.SHAPES[tile]
    a, b, ea, eb, J = goo.decompose_tile(tile, fmt)
    NB = N // 32
    ea3 = np.repeat(ea.reshape(M, J, NB), 32, axis=2)
    eb3 = eb.reshape(N, J, NB)[np.arange(N), :, np.arange(N) // 32].T  # [J][N]: the byte over k = j·N + n
    return a.reshape(M, J, N).astype(np.float64), ea3 + eb3[None], J


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_decompose(fmt, tile):
    M, N = goo.SHAPES[tile]
    target = goo.gpu_target(tile)
    a, b, ea, eb, J = goo.decompose_tile(tile, fmt)
    K = J * N
    assert J <= goo.J_CAP[fmt] and K % FORMATS[fmt].K_MULTIPLE == 0
    assert a.shape == (M, K) and b.shape == (N, K) and ea.shape == (M, K // 32) and eb.shape == (N, K // 32)
    # exact codes of the format, scale bytes 0 .. 254
    for x in (a, b):
        x = x.astype(np.float32)
        back = (from_fp8_e4m3_bits(to_fp8_e4m3_bits(x)) if fmt == "mxfp8"
                else from_fp4_e2m1_codes(to_fp4_e2m1_codes(x)))
        np.testing.assert_array_equal(back, x)
    # … but for the one byte 0xFF of each NaN column
    cols = np.array(goo.NAN_COLUMNS[tile])
    nan_bytes = np.zeros(eb.shape, bool)
    nan_bytes[cols, cols // 32] = True
    assert ((127 + eb)[nan_bytes] == 0xFF).all()
    for e in (ea, eb[~nan_bytes]):
        assert 0 <= (127 + e).min() and (127 + e).max() <= 254
    # Bt is one-hot at k = j·N + n; so in a group of 8 neighbouring k at most one product of any (m, n) is non-zero
    k = np.arange(K)
    np.testing.assert_array_equal(b, (k[None, :] % N == np.arange(N)[:, None]).astype(b.dtype))
    assert ((b != 0).reshape(N, K // 8, 8).sum(axis=2) <= 1).all()
    # the exact sum of the pieces, in every order: each partial sum along j is an fp32 value, the last the target
    fin, inf, nan = goo.classes(target)
    dig, e, _ = _pieces(tile, fmt)
    np.testing.assert_array_equal(np.flatnonzero(nan.any(axis=0)), cols)
    assert nan[:, cols].all() and not dig[:, :, cols].any()  # a NaN column has no piece
    with np.errstate(over="ignore"):
        pieces = np.ldexp(dig, e)  # float64: exact, 448·2^254 included
    assert np.isfinite(pieces).all()
    fin3 = np.broadcast_to(fin[:, None, :], pieces.shape)
    part = np.cumsum(np.where(fin3, pieces, 0), axis=1)
    with np.errstate(over="ignore", under="ignore"):
        assert np.array_equal(part.astype(np.float32).astype(np.float64), part)
    # any subset of the pieces, not only the prefixes: the pieces of an element share no bit
    mags = np.where(fin3, np.abs(pieces), 0)
    top = np.where(mags != 0, np.frexp(mags)[1], -10000)  # mags < 2^top
    low = np.where(mags != 0, e, 10000)            # digits are integers: a piece is a multiple of 2^e
    order = np.argsort(-top, axis=1)
    top_s, low_s = np.take_along_axis(top, order, axis=1), np.take_along_axis(low, order, axis=1)
    nz = np.take_along_axis(mags, order, axis=1) != 0
    assert (~(nz[:, 1:] & nz[:, :-1]) | (top_s[:, 1:] <= low_s[:, :-1])).all()
    total = part[:, -1].astype(np.float32)
    np.testing.assert_array_equal(bits(total)[fin], bits(target)[fin])
    assert (np.abs(dig[fin3]) < (1 << goo.RADIX_BITS[fmt])).all()
    # Inf: one piece of the largest element under 254 · 254, by the sign
    big = goo.BIGGEST[fmt]
    neg = (bits(target) & SIGN) != 0
    assert (inf & neg).sum() >= 32 and (inf & ~neg).sum() >= 32
    for mask, piece in ((inf & ~neg, big), (inf & neg, -big)):
        at = dig.transpose(0, 2, 1)[mask]  # [sites][J]
        assert (at[:, 0] == piece).all() and (at[:, 1:] == 0).all()
        assert (e.transpose(0, 2, 1)[mask][:, 0] == 254).all()
    assert (ea.reshape(M, J, N // 32)[:, 0][inf.reshape(M, N // 32, 32).any(axis=2)] == 127).all()
    assert (eb.reshape(N, J, N // 32)[:, 0][~nan_bytes.reshape(N, J, N // 32)[:, 0]] == 127).all()


@pytest.fixture(scope="module")
def cpu_cr():
    cr = ck.ClNumberCruncher(ck.ClPlatforms.all().cpus(True), "__global__ void nop(float* x) {}")
    yield cr
    cr.dispose()


def _same_as_target(got64, target):
    """A float64 host product rounds to the target's bits, and is NaN exactly at its NaN sites."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        got = np.asarray(got64).astype(np.float32)
    nan = goo.classes(target)[2]
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(bits(got)[~nan], bits(target)[~nan])


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_reference_reproduces_the_target(cpu_cr, fmt, tile):
    """The classes' own reference() on the operands as the GPU tier sets them."""
    M, N = goo.SHAPES[tile]
    a, b, ea, eb, J = goo.decompose_tile(tile, fmt)
    g = FORMATS[fmt](M, N, J * N, cruncher=cpu_cr, tile=tile, fill="none")
    enc = (lambda x: pack_fp4(to_fp4_e2m1_codes(x))) if fmt == "mxfp4" else to_fp8_e4m3_bits
    g.A.array[:] = enc(a.astype(np.float32)).ravel()
    g.B.array[:] = enc(b.astype(np.float32)).ravel()
    g.SA.array[:] = (127 + ea).ravel()
    g.SB.array[:] = (127 + eb).ravel()
    with np.errstate(invalid="ignore"):
        ref = g.reference()
    _same_as_target(ref, goo.gpu_target(tile))


def test_emu_gemm8_reproduces_the_target():
    """gemm8_oracles' element-by-element emulator (e4m3 codes only), on one band of the smaller shape."""
    a, b, ea, eb, _ = goo.decompose_tile("128x128", "mxfp8")
    rows = slice(0, 128)
    c = emu_gemm8(to_fp8_e4m3_bits(a[rows].astype(np.float32)), to_fp8_e4m3_bits(b.astype(np.float32)),
                  (127 + ea[rows]).astype(np.uint8), (127 + eb).astype(np.uint8))
    _same_as_target(c, goo.gpu_target("128x128")[rows])


# -------------------------------------------- 3: the data rejects wrong epilogues


def _relu(c, wrong):
    u = bits(c)
    nan = (u & ABS) > INF
    pos = u.view(np.int32) > 0
    if wrong == "relu_max":  # max(x, 0) as the float instruction has it: NaN → 0
        keep = pos & ~nan
    elif wrong == "relu_keeps_negative_denormals":  # a float compare x < 0 under flushed denormals
        keep = pos | nan | (((u & SIGN) != 0) & ((u & INF) == 0) & ((u & ABS) != 0))
    else:
        keep = pos | nan
    return np.where(keep, u, np.uint32(0)).view(np.float32)


def _bf16(c, wrong):
    u = bits(c).astype(np.uint64)
    if wrong == "bf16_half_up":
        r = (u + 0x8000) >> 16
    else:
        r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    if wrong == "bf16_no_inf_carry":  # a finite value stays finite
        r = np.where(((r & 0x7FFF) == 0x7F80) & ((u & 0x7FFFFFFF) < 0x7F800000), r - 1, r)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def _e4m3(y, wrong):
    """Codes of float64 ``y`` (already scaled)."""
    y32 = y.astype(np.float32)
    if wrong == "truncate":
        a = np.abs(y)
        m, ex = np.frexp(np.where(np.isfinite(a), a, 1.0))
        cut = np.where(a >= 2.0 ** -6, np.ldexp(np.floor(m * 16) / 16, ex), np.floor(a * 512) / 512)
        y32 = np.where(np.isfinite(y), np.copysign(cut, y), y).astype(np.float32)
    codes = to_fp8_e4m3_bits(y32)
    sign = ((bits(y32) >> np.uint32(24)) & np.uint32(0x80)).astype(np.uint8)
    if wrong == "no_saturation_repair":  # what rounds past 448 keeps the instruction's all-ones code
        codes = np.where(np.abs(y32) > 464, np.uint8(0x7F) | sign, codes)
    if wrong == "nan_keeps_sign":
        codes = np.where(np.isnan(y32), np.uint8(0x7F) | sign, codes)
    return codes.astype(np.uint8)


def _e2m1(y, wrong):
    if wrong != "truncate":
        return to_fp4_e2m1_codes(y)
    a = np.abs(y)
    with np.errstate(invalid="ignore"):
        code = sum((a >= v).astype(np.uint8) for v in (0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0))
    return np.where(np.isnan(y), 0, code | (np.signbit(y).astype(np.uint8) << 3)).astype(np.uint8)


def variant_codec(c, out, act=None, wrong=None):
    """host_codec written out once more in numpy, with one named error
    (``wrong=None``: none, and then it must equal host_codec)."""
    c = np.ascontiguousarray(c, np.float32)
    if act == "relu":
        c = _relu(c, wrong)
    if out == "bfloat16":
        return _bf16(c, wrong), None, None
    M, N = c.shape
    emax = 8 if out == "mxfp8" else 2
    with np.errstate(invalid="ignore"):
        x = c.astype(np.float64).reshape(M, N // 32, 32)
    amax = np.where(np.isfinite(x), np.abs(x), 0.0)

    def shared(m):
        return np.clip(np.where(m > 0, np.frexp(m)[1].astype(np.int64) - 1 - emax, 0), -127, 127)

    if wrong == "maximum_over_16":  # the last step of the block maximum is missing: each half its own, the first stored
        halves = shared(amax.reshape(M, N // 32, 2, 16).max(axis=3))
        e_el, e_byte = np.repeat(halves, 16, axis=2), halves[..., 0]
    else:
        e_byte = shared(amax.max(axis=2))
        e_el = np.broadcast_to(e_byte[..., None], x.shape)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        y = np.ldexp(x, -e_el).reshape(M, N)
        if out == "mxfp8":
            codes, sy = _e4m3(y, wrong), e_byte + 127
        else:
            codes = pack_fp4(_e2m1(y, wrong))
            lane = x[..., :8] if wrong == "nan_byte_per_lane" else x  # the byte of the block's first lane only
            sy = np.where(np.isnan(lane).any(axis=2), 0xFF, e_byte + 127)
    sy = sy.astype(np.uint8)
    if wrong == "scale_bytes_swapped":  # the two bytes of a wave's scale word
        sy = sy.reshape(M, N // 64, 2)[:, :, ::-1].reshape(M, N // 32).copy()
    return codes, sy, pack_mx_scales(sy)


# (the error, the outputs it can show in, the activations)
WRONG = [("bf16_half_up", ("bfloat16",), ACTS),
         ("bf16_no_inf_carry", ("bfloat16",), ACTS),
         ("truncate", ("mxfp8", "mxfp4"), ACTS),
         ("no_saturation_repair", ("mxfp8",), ACTS),
         ("nan_keeps_sign", ("mxfp8",), ACTS),
         ("nan_byte_per_lane", ("mxfp4",), ACTS),
         ("relu_max", MX_OUTPUTS, ("relu",)),
         ("relu_keeps_negative_denormals", MX_OUTPUTS, ("relu",)),
         ("maximum_over_16", ("mxfp8", "mxfp4"), ACTS),
         ("scale_bytes_swapped", ("mxfp8", "mxfp4"), ACTS)]


def _differs(got, want, out):
    try:
        assert_same_output(got, want, out)
    except AssertionError:
        return True
    return False


TARGETS = {"placed": goo.placed_target, "gpu": goo.gpu_target}


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("out", MX_OUTPUTS)
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("which", sorted(TARGETS))
def test_honest_codec_and_designed_cases(which, tile, out, act):
    """The written-out codec without an error is host_codec, and host_codec
    of the target shows every case the GPU tier looks for."""
    t = TARGETS[which](tile)
    want = host_codec(t, out, act)
    assert_same_output(variant_codec(t, out, act), want, out, (tile, out, act))
    goo.assert_designed_cases_present(want, t, out, act)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("which", sorted(TARGETS))
@pytest.mark.parametrize("wrong,outs,acts", WRONG, ids=[w[0] for w in WRONG])
def test_wrong_epilogues_are_rejected(wrong, outs, acts, which, tile):
    """On the placed designed bits and on what the GPU tier builds of them."""
    t = TARGETS[which](tile)
    for out in outs:
        for act in acts:
            got = variant_codec(t, out, act, wrong)
            assert _differs(got, host_codec(t, out, act), out), (wrong, out, act, "not noticed")
