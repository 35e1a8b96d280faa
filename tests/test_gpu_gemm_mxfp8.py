"""GPU tier of the MXFP8 GEMM (kernels/sgemm_mxfp8.hip, GemmMxFp8): exact
data first (integers under mixed block scales, a probe of the lane ↔ (row,
k block) scale map, cancelling extreme scales, the ends of the e4m3 range
under non-unit scales), then random wide-range data against a derived bound,
then the multi-device, host-resident and streamed paths and a re-upload;
last the cases of gemm8_oracles.py (NaN codes, scale byte 0xFF, the ends of
the scale range, results in fp32's subnormal range, ragged tile groups) and
the single-instruction probe of the scaled MFMA."""
import numpy as np
import pytest

import cekirdekler_amd as ck
import gemm8_oracles as g8
import gemm_oracles as go
from cekirdekler_amd.ops.gemm import (MXFP8_TILES, GemmMxFp8, e8m0_to_f64, from_fp8_e4m3_bits, from_mxfp8,
                                      to_fp8_e4m3_bits, to_mxfp8)
from cekirdekler_amd.ops.library import library

pytestmark = pytest.mark.gpu

# K/128 = 1, 2, 3, 5: the ping-pong prologue stages two K-tiles ahead, the Bt
# ring has three buffers and the scales are prefetched one K-tile ahead
# (clamped at the end), so these are the counts at which the loop ends can go wrong
K_TAIL_SHAPES = [(256, 256, 128), (512, 256, 256), (256, 512, 384), (1024, 768, 640)]
SHAPES = {"256x256pbx": K_TAIL_SHAPES, "128x128": K_TAIL_SHAPES + [(128, 128, 128), (384, 128, 256)]}
TILE_SHAPES = [(t, s) for t in sorted(MXFP8_TILES) for s in SHAPES[t]]


@pytest.fixture(scope="module")
def cr():
    c = ck.ClNumberCruncher(ck.ClPlatforms.all().gpus()[0], "", prebuilt=library("sgemm_mxfp8"))
    yield c
    c.dispose()


def _set(g, a, b, ea, eb):
    """Operands from exactly representable element values (checked) and
    scale exponents (one per row and block of 32, or one for all)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    g.A.array[:] = to_fp8_e4m3_bits(a).ravel()
    g.B.array[:] = to_fp8_e4m3_bits(b).ravel()
    assert np.array_equal(from_fp8_e4m3_bits(g.A.array), a.ravel())
    assert np.array_equal(from_fp8_e4m3_bits(g.B.array), b.ravel())
    g.SA.array[:] = np.broadcast_to(127 + np.asarray(ea), (g.M, g.K // 32)).ravel()
    g.SB.array[:] = np.broadcast_to(127 + np.asarray(eb), (g.N, g.K // 32)).ravel()


def _scaled(x, e):
    """float64 [rows][K] elements times 2^e per block of 32 (exact)."""
    rows, K = x.shape
    e = np.broadcast_to(np.asarray(e), (rows, K // 32))
    return (np.asarray(x, np.float64).reshape(rows, K // 32, 32) * np.ldexp(1.0, e)[..., None]).reshape(rows, K)


_INT_CACHE = {}


def _int_case(shape):
    """Integers in [-4, 4], scale exponents in {-2 .. 2} per block,
    independently for A and B, and the float64 product, once per shape."""
    if shape not in _INT_CACHE:
        M, N, K = shape
        rng = np.random.default_rng(sum(shape))
        a = rng.integers(-4, 5, (M, K))
        b = rng.integers(-4, 5, (N, K))
        ea = rng.integers(-2, 3, (M, K // 32))
        eb = rng.integers(-2, 3, (N, K // 32))
        # in units of 2^-4 every product is an integer <= 4·4·2^(2+2+4) = 2^12
        # and every partial sum an integer below K · 2^12 < 2^24: exact in
        # fp32 in any summation order
        assert K * 2 ** 12 < 2 ** 24
        ref = _scaled(a, ea) @ _scaled(b, eb).T
        assert np.array_equal(np.rint(ref * 16), ref * 16) and np.abs(ref * 16).max() < 2 ** 24
        ref.setflags(write=False)
        _INT_CACHE[shape] = (a, b, ea, eb, ref)
    return _INT_CACHE[shape]


def _int_gemm(shape, **kw):
    a, b, ea, eb, ref = _int_case(shape)
    g = GemmMxFp8(*shape, fill="none", **kw)
    _set(g, a, b, ea, eb)
    return g, ref


def _assert_exact(c, ref):
    assert c.dtype == np.float32
    bad = np.argwhere(c.astype(np.float64) != ref)
    assert bad.size == 0, (len(bad), bad[:4].tolist(), [float(c[tuple(i)]) for i in bad[:4]],
                           [float(ref[tuple(i)]) for i in bad[:4]])


@pytest.mark.parametrize("tile,shape", TILE_SHAPES)
def test_exact_integers_with_scales(cr, tile, shape):
    """C equals the float64 product of the scaled integers bit for bit
    (_int_case has the argument)."""
    g, ref = _int_gemm(shape, cruncher=cr, tile=tile, group_m=2)
    g.C.array[:] = np.nan
    g.run(resident=True)
    _assert_exact(g.result(), ref)


# SA[m][b] = 127 + ((3m + cb) % 5 - 2).  c = 5 is the probe as it was specified:
# 5b % 5 = 0, so that SA does not depend on the block and a wrong k block of
# A's scale goes unseen (the host check below shows it).  c = 2 is the same
# probe with SA varying in the block as well; both run.
PROBE_SA_BLOCK_COEFF = [5, 2]


def _probe_case(c):
    M, N, K = 256, 512, 384
    m, n, k, blk = np.arange(M), np.arange(N), np.arange(K), np.arange(K // 32)
    pick = (37 * m + 11) % K
    a = np.zeros((M, K), np.float32)
    a[m, pick] = 1
    b = ((3 * n[:, None] + 5 * k[None, :]) % 17 - 8).astype(np.float32)
    ea = (3 * m[:, None] + c * blk[None, :]) % 5 - 2
    eb = (7 * n[:, None] + 2 * blk[None, :]) % 5 - 2
    return (M, N, K), pick, a, b, ea, eb


@pytest.mark.parametrize("coeff", PROBE_SA_BLOCK_COEFF)
def test_scale_mapping_probe_distinguishes_on_the_host(coeff):
    """The probe's expected C against what wrong scale maps would give, on
    the CPU: the unit-scale product, SA and SB swapped in role (each applied
    to the other operand's row index), the k block of either scale shifted by
    one, and the scale row shifted by 16 (one fragment).  Every one of them
    differs from the expected C in more than half the elements, but for the
    shifted block of A under coeff = 5, which changes nothing."""
    (M, N, K), pick, a, b, ea, eb = _probe_case(coeff)
    pb = pick // 32
    m = np.arange(M)
    bv = b[:, pick].T.astype(np.float64)  # [M][N]: the surviving element of Bt
    n = np.arange(N)

    def c_of(ea_at, eb_at):  # exponents [M] and [M][N]
        return bv * np.ldexp(1.0, ea_at[:, None] + eb_at)

    want = c_of(ea[m, pb], eb[:, pb].T)
    np.testing.assert_array_equal(want, _scaled(a, ea) @ _scaled(b, eb).T)
    wrong = {
        "unit scales": bv,
        "A block + 1": c_of(ea[m, (pb + 1) % (K // 32)], eb[:, pb].T),
        "B block + 1": c_of(ea[m, pb], eb[:, (pb + 1) % (K // 32)].T),
        "A row + 16": c_of(ea[(m + 16) % M, pb], eb[:, pb].T),
        "B row + 16": c_of(ea[m, pb], eb[(n + 16) % N][:, pb].T),
        "SA <-> SB": c_of(eb[m % N, pb], ea[n % M][:, pb].T),
    }
    for name, c in wrong.items():
        frac = float((c != want).mean())
        if coeff == 5 and name == "A block + 1":
            assert frac == 0.0  # the blind spot of the probe as specified
        else:
            assert frac > 0.5, (name, frac)


@pytest.mark.parametrize("coeff", PROBE_SA_BLOCK_COEFF)
@pytest.mark.parametrize("tile", sorted(MXFP8_TILES))
def test_scale_mapping_probe(cr, tile, coeff):
    """A picks one k per row, SA and SB vary with row and block, Bt is
    asymmetric in n and k: C[m][n] is the one surviving product
    Bt[n][k]·2^(ea[m][k/32] + eb[n][k/32]), k = (37m + 11) % K.  A wrong lane ↔
    (row, k block) map, a wrong op_sel, SA and SB swapped or the packing off
    by a fragment give another C (test_scale_mapping_probe_distinguishes_on_the_host)."""
    shape, pick, a, b, ea, eb = _probe_case(coeff)
    g = GemmMxFp8(*shape, cruncher=cr, tile=tile, fill="none")
    _set(g, a, b, ea, eb)
    g.C.array[:] = np.nan
    g.run(resident=True)
    want = _scaled(a, ea) @ _scaled(b, eb).T
    unit = b[:, pick].T.astype(np.float64)
    assert (want != unit).mean() > 0.5
    _assert_exact(g.result(), want)


@pytest.mark.parametrize("tile", sorted(MXFP8_TILES))
def test_cancelling_extreme_scales(cr, tile):
    """SA = 2^-60 with SB = 2^60 gives the unit-scale integer product exactly,
    SA = SB = 2^40 that product times 2^80: the exponents are applied as
    exponents and do not travel through a narrower format."""
    shape = (256, 256, 256)
    rng = np.random.default_rng(11)
    a = rng.integers(-8, 9, shape[::2])
    b = rng.integers(-8, 9, shape[1:])
    ref = (a @ b.T).astype(np.float64)
    assert np.abs(ref).max() < 2 ** 24 and np.abs(ref).max() > 0
    for ea, eb, factor in ((-60, 60, 1.0), (40, 40, 2.0 ** 80)):
        g = GemmMxFp8(*shape, cruncher=cr, tile=tile, fill="none")  # resident operands go up once per object
        _set(g, a, b, ea, eb)
        g.C.array[:] = np.nan
        g.run(resident=True)
        _assert_exact(g.result(), ref * factor)


@pytest.mark.parametrize("tile", sorted(MXFP8_TILES))
def test_range_ends_with_scales(cr, tile):
    """±448 and ±2^-9 elements (test_gpu_gemm_fp8.py::test_range_ends) under
    SA = 2^3 and SB = 2^-5: the signed count times mag² times 2^-2."""
    M = N = K = 256
    rng = np.random.default_rng(5)
    sa = rng.choice([-1.0, 1.0], (M, K))
    sb = rng.choice([-1.0, 1.0], (N, K))
    count = sa @ sb.T
    for mag in (448.0, 2.0 ** -9):
        g = GemmMxFp8(M, N, K, cruncher=cr, tile=tile, fill="none")
        _set(g, sa * mag, sb * mag, 3, -5)
        g.C.array[:] = np.nan
        g.run(resident=True)
        _assert_exact(g.result(), count * (mag * mag) * 2.0 ** -2)
    assert np.abs(count).max() > 0


@pytest.mark.parametrize("tile", sorted(MXFP8_TILES))
def test_random_wide_range_data_within_derived_bound(cr, tile):
    """|C - ref| <= K · 2^-23 · Σ_k |a_k·b_k| per element, a and b the
    dequantised operands (the derivation of
    test_gpu_gemm_fp8.py::test_random_data_within_derived_bound: exact
    products, K fp32 additions each off by at most one unit in the last place
    of a partial sum <= Σ|a·b|).  The power-of-two scales add no rounding
    while nothing leaves fp32's normal range: the elements are at least 2^-9
    under block scales of at least 2^-21, so every nonzero product is above
    2^-60 and the sums are below 2^24 · K.  The bound assumes the instruction
    aligns the four blocks' partial sums with at least 24 bits — across
    blocks it does, inside a group of 8 neighbouring k it keeps 14
    (test_probe_adjacent_k_sum_as_measured), so the derivation is not a
    guarantee for every data set; on these uniform draws the bound holds with
    the margin printed below.  Outside the
    normal range — results in fp32's subnormal range, exponent sums of ±254,
    overflow — test_scale_ends has the exact cases."""
    M, N, K = 1024, 512, 512
    seed = 3
    g = GemmMxFp8(M, N, K, cruncher=cr, tile=tile, fill="random", seed=seed)
    a = from_mxfp8(g.A.array.reshape(M, K), g.SA.array.reshape(M, K // 32)).astype(np.float64)
    b = from_mxfp8(g.B.array.reshape(N, K), g.SB.array.reshape(N, K // 32)).astype(np.float64)
    assert int(g.SA.array.min()) >= 127 - 21 and int(g.SB.array.min()) >= 127 - 21
    np.testing.assert_array_equal(a, _scaled(from_fp8_e4m3_bits(g.A.array).reshape(M, K),
                                             g.SA.array.reshape(M, K // 32).astype(np.int64) - 127))
    ref = a @ b.T
    np.testing.assert_array_equal(ref, g.reference())
    bound = K * 2.0 ** -23 * (np.abs(a) @ np.abs(b).T)
    g.run(resident=True)
    c = g.result().astype(np.float64)
    err = np.abs(c - ref)
    ratio = float((err / bound).max())
    rel = float(err.max() / np.abs(ref).max())
    # end to end: against the float64 product of the unquantised inputs (the
    # draws of fill="random" repeated), reported and not asserted
    rng = np.random.default_rng(seed)
    raw = []
    for rows in (M, N):
        x = rng.uniform(-1, 1, (rows, K // 32, 32))
        raw.append(np.ldexp(x, rng.integers(-12, 13, (rows, K // 32, 1))).astype(np.float32).reshape(rows, K))
    assert np.array_equal(to_mxfp8(raw[0])[0].ravel(), g.A.array) and np.array_equal(to_mxfp8(raw[1])[1].ravel(),
                                                                                       g.SB.array)
    full = raw[0].astype(np.float64) @ raw[1].astype(np.float64).T
    e2e = float(np.abs(c - full).max() / np.abs(full).max())
    e2e_rms = float(np.sqrt(((c - full) ** 2).mean() / (full ** 2).mean()))
    print(f"mxfp8 {tile} {M}x{N}x{K}: worst |C-ref|/bound = {ratio:.3e}, max|C-ref|/max|ref| = {rel:.3e}, "
          f"end to end vs unquantised fp64: max|C-full|/max|full| = {e2e:.3e}, rms = {e2e_rms:.3e}")
    assert ratio <= 1.0, f"worst |C-ref|/bound = {ratio:.3e}, max|C-ref|/max|ref| = {rel:.3e}"
    # verify_full / verify report max |C - ref| / max |ref| per tile: the same
    # bound, taken per tile
    per_tile = lambda x: x.reshape(M // g.BM, g.BM, N // g.BN, g.BN).max(axis=(1, 3))  # noqa: E731
    limit = float((per_tile(bound) / per_tile(np.abs(ref))).max())
    err_full, checked = g.verify_full(1)
    assert checked == g.tiles and err_full <= limit, (err_full, limit, checked)
    assert g.verify(1) <= limit


def test_two_logical_devices():
    g0 = ck.ClPlatforms.all().gpus()[0]
    c2 = ck.ClNumberCruncher(g0 + g0, "", prebuilt=library("sgemm_mxfp8"))
    g, ref = _int_gemm((1024, 1024, 256), cruncher=c2)
    for _ in range(4):
        g.C.array[:] = np.nan
        g.run(resident=False)
        r = c2.ranges(1)
        assert len(r) == 2 and sum(r) == g.global_range and all(x % g.L == 0 for x in r), r
        _assert_exact(g.result(download=False), ref)
    err, checked = g.verify_full(1, host=True)
    assert checked == g.tiles and err == 0.0, (err, checked)
    c2.dispose()


def test_host_resident_run(cr):
    g, ref = _int_gemm((1024, 512, 256), cruncher=cr)
    g.C.array[:] = np.nan
    g.run(resident=False)
    _assert_exact(g.result(download=False), ref)


@pytest.mark.parametrize("group_m", [2, 1])
def test_host_resident_streamed_blobs(cr, group_m):
    """Four blobs per device.  The 8 tiles are 4 / group_m tile groups (the
    blob unit: one A row panel each), so group_m = 1 runs the event pipeline
    and group_m = 2, with fewer groups than blobs, the plain path.  A goes up
    one row panel per blob; Bt and both scale arrays are full reads."""
    g, ref = _int_gemm((1024, 512, 256), cruncher=cr, group_m=group_m)
    assert g.can_stream()
    g.C.array[:] = np.nan
    g.run(resident=False, stream_blobs=4)
    assert cr.last_record()["pipelined"] == (group_m == 1)
    _assert_exact(g.result(download=False), ref)


def test_reupload_takes_new_scales(cr):
    """SA changed on the host between two host-resident calls: the second
    call's C is the new exact product (stale packed scales would give the old one)."""
    shape = (1024, 512, 256)
    a, b, ea, eb, ref = _int_case(shape)
    g, _ = _int_gemm(shape, cruncher=cr)
    g.run(resident=False)
    _assert_exact(g.result(download=False), ref)
    ea2 = (ea + 3) % 5 - 2
    assert (ea2 != ea).all()
    g.SA.array[:] = (127 + ea2).ravel()
    ref2 = _scaled(a, ea2) @ _scaled(b, eb).T
    assert (ref2 != ref).mean() > 0.5
    g.C.array[:] = np.nan
    g.run(resident=False)
    _assert_exact(g.result(download=False), ref2)
    assert e8m0_to_f64(g.SA.array).max() == 4.0


# --------------------------------------------------------------------------- non-finite values and the ends of the scale range
# (tests/gemm8_oracles.py has the cases and their arguments, test_gemm8_oracles.py
# what each of them rejects)

def _set_codes(g, case):
    """Operands from a gemm8_oracles case: codes and scale bytes as they are
    (NaN codes and 0xFF included)."""
    a, b, sa, sb, want = case
    g.A.array[:] = a.ravel()
    g.B.array[:] = b.ravel()
    g.SA.array[:] = sa.ravel()
    g.SB.array[:] = sb.ravel()
    return want


def _run_case(cr, tile, shape, case, **kw):
    g = GemmMxFp8(*shape, cruncher=cr, tile=tile, fill="none", **kw)  # resident operands go up once per object
    want = _set_codes(g, case)
    g.C.array[:] = 1.0  # a leftover NaN must not pass for a computed one
    g.run(resident=True)
    go.assert_nonfinite(g.result(), want)


@pytest.mark.parametrize("shape", g8.CLASS_SHAPES)
@pytest.mark.parametrize("tile", sorted(MXFP8_TILES))
def test_nonfinite(cr, tile, shape):
    """e4m3 NaN codes (0x7F under scale byte 0, 0xFF under byte 254, 0x7F in
    Bt) poison exactly their row or column of C, 0·NaN included, and a scale
    byte 0xFF over finite elements its whole row (OCP MX, e8m0_to_f64,
    reference()); every other element is the exact product."""
    _run_case(cr, tile, shape, g8.mx_nonfinite(shape))


@pytest.mark.parametrize("kind", g8.SCALE_END_KINDS[:3])
@pytest.mark.parametrize("shape", g8.CLASS_SHAPES)
@pytest.mark.parametrize("tile", sorted(MXFP8_TILES))
def test_scale_ends(cr, tile, shape, kind):
    """Scale bytes 254 and 0 cancel exactly (either way round); +448 under
    byte 254 gives ±Inf by the sign of Bt's row, 254 + 254 included, while
    every other row stays finite and exact (gemm8_oracles.mx_scale_ends)."""
    _run_case(cr, tile, shape, g8.mx_scale_ends(shape, kind))


@pytest.mark.parametrize("kind", g8.SCALE_END_KINDS[3:])
@pytest.mark.parametrize("shape", g8.UNDERFLOW_SHAPES)
@pytest.mark.parametrize("tile", sorted(MXFP8_TILES))
def test_scale_ends_underflow(cr, tile, shape, kind):
    """ea + eb = -140 on every block pair: all of C lies in fp32's subnormal
    range and is exact (nothing flushed, in the instruction or the kernel);
    SA = SB = 0: all of C is ±0 and nothing is NaN."""
    _run_case(cr, tile, shape, g8.mx_scale_ends(shape, kind))


@pytest.mark.parametrize("tile,shape,group_m", [(t, s, gm) for t in sorted(MXFP8_TILES) for s, gm in g8.ragged_groups(t)])
def test_ragged_last_tile_group(cr, tile, shape, group_m):
    """Three tile rows under group_m 2 and 4: the last tile group is shorter
    than group_m.  C is prefilled with NaN, so a tile written twice (another
    one never) shows."""
    g, ref = _int_gemm(shape, cruncher=cr, tile=tile, group_m=group_m)
    assert (g.M // g.BM) % group_m != 0
    g.C.array[:] = np.nan
    g.run(resident=True)
    _assert_exact(g.result(), ref)


def test_nonfinite_on_two_logical_devices():
    """The NaN rows' tiles are split between two devices (host-resident,
    like test_two_logical_devices): they stay exactly those rows."""
    g0 = ck.ClPlatforms.all().gpus()[0]
    c2 = ck.ClNumberCruncher(g0 + g0, "", prebuilt=library("sgemm_mxfp8"))
    g = GemmMxFp8(*g8.SPLIT_SHAPE, cruncher=c2, fill="none")
    want = _set_codes(g, g8.mx_nonfinite(g8.SPLIT_SHAPE))
    for _ in range(2):
        g.C.array[:] = 1.0
        g.run(resident=False)
        r = c2.ranges(1)
        assert len(r) == 2 and sum(r) == g.global_range and min(r) > 0, r
        go.assert_nonfinite(g.result(download=False), want)
    c2.dispose()


@pytest.fixture(scope="module")
def probe_answers():
    """One launch of gemm8_oracles.PROBE_SRC, one wave and one
    v_mfma_scale_f32_16x16x128_f8f6f4 per question: name → C [16][16]."""
    c = ck.ClNumberCruncher(ck.ClPlatforms.all().gpus()[0], g8.PROBE_SRC)
    assert c.error_code() == 0, c.error_message()
    names, a, b, sa, sb = g8.probe_buffers()
    arrays = [ck.ClArray(x.copy()) for x in (a, b, sa, sb)]
    for x in arrays:
        x.write = False
    out = ck.ClArray(np.full(256 * len(names), -7.0, np.float32))
    out.read = False
    out.elements_per_work_item = 4
    arrays[0].next_param(*arrays[1:], out).compute(c, 1, g8.PROBE_KERNEL, 64 * len(names), 64)
    got = out.array.reshape(len(names), 16, 16).copy()
    c.dispose()
    for i, n in enumerate(names):
        print(g8.probe_report(n, got[i]))
    return dict(zip(names, got))


def test_single_instruction_probe(probe_answers):
    """What the instruction itself does, apart from the GEMM kernels, with an
    element NaN, a scale byte 0xFF, exponent sums of +254, 0 and -254 and
    results in fp32's subnormal range: the IEEE / OCP answer in every case
    (the fixture prints the raw values, profiles/gemm8_specials.md keeps them)."""
    assert set(g8.PROBE_IEEE) < set(probe_answers)
    for n in g8.PROBE_IEEE:
        go.assert_nonfinite(probe_answers[n], g8.probe_problems()[n][4])


def test_probe_adjacent_k_sum_as_measured(probe_answers):
    """Two products at neighbouring k, 2^16 and 2^(14-i-j): the instruction
    keeps 14 bits below the larger one's top and drops the rest
    (gemm8_oracles.adjacent_k_as_measured; GemmFp8's docstring and docs/API.md
    state it).  The derived bounds of the random-data tests hold on their
    data, not on data with more than 14 bits between neighbouring products."""
    go.assert_exact(probe_answers["adjacent_k"], g8.adjacent_k_as_measured())


@pytest.mark.xfail(strict=True, reason="the matrix core sums 8 neighbouring products in 14 bits (profiles/gemm8_specials.md)")
def test_probe_adjacent_k_sum_is_exact(probe_answers):
    """The IEEE twin of test_probe_adjacent_k_sum_as_measured: fails on an
    MI355X today; a hardware or compiler change that makes it pass is noticed."""
    go.assert_nonfinite(probe_answers["adjacent_k"], g8.probe_problems()["adjacent_k"][4])


@pytest.mark.parametrize("sa,sb", [(127, 127), (254, 0), (97, 160)])
@pytest.mark.parametrize("tile", sorted(MXFP8_TILES))
def test_wide_groups_as_measured(cr, tile, sa, sb):
    """test_gpu_gemm_fp8.py::test_wide_groups_as_measured under uniform
    scales: ±448 among small integers are summed by the measured 14-bit rule
    (gemm8_oracles.emu_group_sums), and the scales, cancelling or not, only
    multiply the result by their power of two."""
    shape = g8.CLASS_SHAPES[1]
    a, b, want, exact = g8.wide_groups(shape)
    g = GemmMxFp8(*shape, cruncher=cr, tile=tile, fill="none")
    g.A.array[:] = a.ravel()
    g.B.array[:] = b.ravel()
    g.SA.array[:] = sa
    g.SB.array[:] = sb
    g.C.array[:] = np.nan
    g.run(resident=True)
    _assert_exact(g.result(), want * 2.0 ** (sa + sb - 254))
