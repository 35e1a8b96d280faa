"""GPU tier of the MXFP4 GEMM (kernels/sgemm_mxfp4.hip, GemmMxFp4): the
single-instruction probe of the e2m1 scaled MFMA first (which k a nibble
supplies, which scale byte meets which data, 0xFF, the ends of the scale
range, subnormal results, sums of neighbouring products), then exact data
(all 15 values under mixed block scales, the scale-mapping probe, cancelling
extreme scales, the ends of the e2m1 range, scale byte 0xFF), random
wide-range data against a derived bound, and the multi-device, host-resident
and streamed paths, a re-upload and the ragged last tile group.
gemm4_oracles.py has the cases and their arguments."""
import numpy as np
import pytest

import cekirdekler_amd as ck
import gemm4_oracles as g4
import gemm8_oracles as g8
import gemm_oracles as go
from cekirdekler_amd.ops.gemm import (MXFP4_TILES, GemmMxFp4, e8m0_to_f64, from_fp4_e2m1_codes, from_mxfp4, to_mxfp4,
                                      unpack_fp4)
from cekirdekler_amd.ops.library import library

pytestmark = pytest.mark.gpu

TILES = sorted(MXFP4_TILES)
TILE_SHAPES = [(t, s) for t in TILES for s in g4.SHAPES[t]]


@pytest.fixture(scope="module")
def cr():
    c = ck.ClNumberCruncher(ck.ClPlatforms.all().gpus()[0], "", prebuilt=library("sgemm_mxfp4"))
    yield c
    c.dispose()


# --------------------------------------------------------------------------- the single-instruction probe

@pytest.fixture(scope="module")
def probe_answers():
    """One launch of gemm4_oracles.PROBE_SRC, one wave and one e2m1
    v_mfma_scale_f32_16x16x128_f8f6f4 per question: name → C [16][16]."""
    c = ck.ClNumberCruncher(ck.ClPlatforms.all().gpus()[0], g4.PROBE_SRC)
    assert c.error_code() == 0, c.error_message()
    names, *bufs = g4.probe_buffers()
    arrays = [ck.ClArray(x.copy()) for x in bufs]
    for x in arrays:
        x.write = False
    out = ck.ClArray(np.full(256 * len(names), -7.0, np.float32))
    out.read = False
    out.elements_per_work_item = 4
    arrays[0].next_param(*arrays[1:], out).compute(c, 1, g4.PROBE_KERNEL, 64 * len(names), 64)
    got = out.array.reshape(len(names), 16, 16).copy()
    c.dispose()
    for i, n in enumerate(names):
        print(g4.probe_report(n, got[i]))
    return dict(zip(names, got))


def test_probe_k_map_as_measured(probe_answers):
    """Question 1.  Measured on an MI355X: position k of either operand under
    the natural loader (lane 16·(k/32) + row, byte (k % 32)/2, low nibble for
    even k) meets position k of the other, for all 128 k — a lane's 16 bytes
    are k in [32q, 32q + 32) in natural order, low nibble first, and registers
    4 … 7 of the operand are ignored (the probe fills them with 6.0)."""
    for operand in "ab":
        km = g4.measured_k_map(probe_answers, operand)
        print(f"probe4 k map of {operand}:", km.tolist())
        np.testing.assert_array_equal(km, np.arange(128))


def test_probe_scale_map_as_measured(probe_answers):
    """Question 2.  Measured on an MI355X: the scale byte of lane l applies to
    row l % 16 and MX block l / 16 of the instruction's 128 k (the lane's own
    16 bytes), and op_sel = b picks bits 8b … 8b+7 of the scale register, for
    A and for Bt independently."""
    for operand in "ab":
        for o in range(4):
            row, block, want_block = g4.measured_scale_map(probe_answers, operand, o)
            print(f"probe4 scale map of {operand}, op_sel {o}: rows {row.tolist()} blocks {block.tolist()}")
            np.testing.assert_array_equal(row, np.arange(16))
            np.testing.assert_array_equal(block, want_block)
            name = f"scale_map_{operand}{o}"
            go.assert_nonfinite(probe_answers[name], g4.probe_problems()[name]["want"])


def test_single_instruction_probe(probe_answers):
    """Questions 3 to 5 and the dense baseline: a scale byte 0xFF makes its
    block NaN, zeros included; exponent sums of +254, 0 and -254 give ±Inf,
    the exact product and ±0; results in fp32's subnormal range are exact —
    the IEEE / OCP answer in every case."""
    for n in g4.PROBE_IEEE:
        go.assert_nonfinite(probe_answers[n], g4.probe_problems()[n]["want"])


def test_probe_adjacent_sums_as_measured(probe_answers):
    """Question 6, as measured on an MI355X (profiles/gemm_mxfp4.md has the
    raw values): both sums are the correctly rounded fp32 result.  Inside a
    block two e2m1 products differ by at most 144× ("adjacent_k": 36 beside
    0.25 … 3); across a block boundary 2^16 at k = 31 beside 2^(14-i-j) at
    k = 32 keeps all 24 bits (2^16 + 2^-7 is returned, 2^-8 ties to even).
    The e4m3 path's 14-bit cut inside a group of 8 neighbouring k
    (test_gpu_gemm_mxfp8.py) is not reachable with e2m1 data, so the exact
    tests here needed no narrowing."""
    for n in ("adjacent_k", "adjacent_blocks"):
        go.assert_nonfinite(probe_answers[n], g4.probe_problems()[n]["want"])


# --------------------------------------------------------------------------- exact data

def _int_gemm(shape, **kw):
    a, b, ea, eb, ref = g4.int_case(shape)
    g = GemmMxFp4(*shape, fill="none", **kw)
    g4.set_operands(g, a, b, ea, eb)
    return g, ref


def _run_exact(g, want):
    g.C.array[:] = np.nan
    g.run(resident=True)
    go.assert_exact(g.result(), want)


@pytest.mark.parametrize("tile,shape", TILE_SHAPES)
def test_exact_integers_with_scales(cr, tile, shape):
    """C equals the float64 product of the scaled e2m1 values bit for bit
    (gemm4_oracles.int_case has the argument and asserts its arithmetic)."""
    g, ref = _int_gemm(shape, cruncher=cr, tile=tile, group_m=2)
    assert shape[2] * 2304 < 2 ** 24 and np.abs(ref * 16).max() < 2 ** 24
    _run_exact(g, ref)


@pytest.mark.parametrize("coeff", g4.PROBE_SA_BLOCK_COEFF)
@pytest.mark.parametrize("tile", TILES)
def test_scale_mapping_probe(cr, tile, coeff):
    """A picks one k per row, SA and SB vary with row and block, Bt is
    asymmetric in n and k: C[m][n] is the one surviving product.  A wrong lane
    ↔ (row, k block) map, a wrong op_sel, swapped nibbles or exchanged steps
    give another C (test_mxfp4_host.py::test_scale_mapping_probe_distinguishes_on_the_host)."""
    shape, pick, a, b, ea, eb = g4.probe_case(coeff)
    want, wrong = g4.probe_expected_and_wrong(coeff)
    g = GemmMxFp4(*shape, cruncher=cr, tile=tile, fill="none")
    g4.set_operands(g, a, b, ea, eb)
    assert (want != wrong["unit scales"]).mean() > 0.5
    _run_exact(g, want)


@pytest.mark.parametrize("tile", TILES)
def test_cancelling_extreme_scales(cr, tile):
    """SA = 2^-60 with SB = 2^60 gives the unit-scale product exactly, SA = SB
    = 2^40 that product times 2^80: the exponents are applied as exponents."""
    shape = (256, 256, 256)
    a, b, _, _, _ = g4.int_case(shape)
    ref = a.astype(np.float64) @ b.astype(np.float64).T
    assert np.abs(ref).max() > 0
    for ea, eb, factor in ((-60, 60, 1.0), (40, 40, 2.0 ** 80)):
        g = GemmMxFp4(*shape, cruncher=cr, tile=tile, fill="none")  # resident operands go up once per object
        g4.set_operands(g, a, b, ea, eb)
        _run_exact(g, ref * factor)


@pytest.mark.parametrize("tile", TILES)
def test_range_ends_with_scales(cr, tile):
    """±6 and ±0.5 everywhere under SA = 2^3 and SB = 2^-5: the signed count
    times mag² times 2^-2."""
    M = N = K = 256
    rng = np.random.default_rng(5)
    sa = rng.choice([-1.0, 1.0], (M, K))
    sb = rng.choice([-1.0, 1.0], (N, K))
    count = sa @ sb.T
    assert np.abs(count).max() > 0
    for mag in (6.0, 0.5):
        g = GemmMxFp4(M, N, K, cruncher=cr, tile=tile, fill="none")
        g4.set_operands(g, sa * mag, sb * mag, 3, -5)
        _run_exact(g, count * (mag * mag) * 2.0 ** -2)


@pytest.mark.parametrize("operand", ["A", "B"])
@pytest.mark.parametrize("tile", TILES)
def test_scale_byte_ff_poisons_its_row_or_column(cr, tile, operand):
    """One scale byte 0xFF in A (row 177, a block of the second K-tile), then
    in Bt (row 150, first K-tile): exactly that row (column) of C is NaN, zero
    elements included, and every other element the exact product."""
    shape = (256, 256, 512)
    g, ref = _int_gemm(shape, cruncher=cr, tile=tile)
    row = 177 if operand == "A" else 150
    arr, rows, blk = (g.SA, g.M, 9) if operand == "A" else (g.SB, g.N, 2)
    arr.array.reshape(rows, -1)[row, blk] = 0xFF
    cls = np.zeros(ref.shape, np.int8)
    if operand == "A":
        cls[row] = go.NAN
    else:
        cls[:, row] = go.NAN
    assert np.isnan(g.reference()).sum() == 256
    g.C.array[:] = 1.0  # a leftover NaN must not pass for a computed one
    g.run(resident=True)
    go.assert_nonfinite(g.result(), (cls, np.where(cls == go.FINITE, ref, 0.0)))


# --------------------------------------------------------------------------- random data

@pytest.mark.parametrize("tile", TILES)
def test_random_wide_range_data_within_derived_bound(cr, tile):
    """|C - ref| <= K · 2^-23 · Σ_k |a_k·b_k| per element, a and b the
    dequantised operands (test_gpu_gemm_mxfp8.py's bound and caveats: exact
    products, K fp32 additions each off by at most one unit in the last place
    of a partial sum <= Σ|a·b|; the power-of-two scales add no rounding while
    nothing leaves fp32's normal range: elements of at least 2^-1 under block
    scales of at least 2^-15 give products above 2^-32).  It is a bound for
    these uniform draws, not a guarantee for every data set."""
    M, N, K = g4.RANDOM_SHAPE
    seed = 3
    g = GemmMxFp4(M, N, K, cruncher=cr, tile=tile, fill="random", seed=seed)
    a = from_mxfp4(g.A.array.reshape(M, K // 2), g.SA.array.reshape(M, K // 32)).astype(np.float64)
    b = from_mxfp4(g.B.array.reshape(N, K // 2), g.SB.array.reshape(N, K // 32)).astype(np.float64)
    assert int(g.SA.array.min()) >= 127 - 15 and int(g.SB.array.min()) >= 127 - 15 and int(g.SA.array.max()) < 0xFF
    np.testing.assert_array_equal(a, g4.scaled(from_fp4_e2m1_codes(unpack_fp4(g.A.array)).reshape(M, K),
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
    assert np.array_equal(to_mxfp4(raw[0])[0].ravel(), g.A.array) and np.array_equal(to_mxfp4(raw[1])[1].ravel(),
                                                                                       g.SB.array)
    full = raw[0].astype(np.float64) @ raw[1].astype(np.float64).T
    e2e = float(np.abs(c - full).max() / np.abs(full).max())
    e2e_rms = float(np.sqrt(((c - full) ** 2).mean() / (full ** 2).mean()))
    print(f"mxfp4 {tile} {M}x{N}x{K}: worst |C-ref|/bound = {ratio:.3e}, max|C-ref|/max|ref| = {rel:.3e}, "
          f"end to end vs unquantised fp64: max|C-full|/max|full| = {e2e:.3e}, rms = {e2e_rms:.3e}")
    assert ratio <= 1.0, f"worst |C-ref|/bound = {ratio:.3e}, max|C-ref|/max|ref| = {rel:.3e}"
    # verify_full / verify report max |C - ref| / max |ref| per tile: the same bound, taken per tile
    per_tile = lambda x: x.reshape(M // g.BM, g.BM, N // g.BN, g.BN).max(axis=(1, 3))  # noqa: E731
    limit = float((per_tile(bound) / per_tile(np.abs(ref))).max())
    err_full, checked = g.verify_full(1)
    assert checked == g.tiles and err_full <= limit, (err_full, limit, checked)
    assert g.verify(1) <= limit


# --------------------------------------------------------------------------- paths

@pytest.mark.parametrize("resident", [False, True])
def test_two_logical_devices(resident):
    g0 = ck.ClPlatforms.all().gpus()[0]
    c2 = ck.ClNumberCruncher(g0 + g0, "", prebuilt=library("sgemm_mxfp4"))
    g, ref = _int_gemm(g4.TWO_DEVICE_SHAPE, cruncher=c2)
    for _ in range(3):
        g.C.array[:] = np.nan
        g.run(resident=resident)
        r = c2.ranges(1)
        assert len(r) == 2 and sum(r) == g.global_range and all(x % g.L == 0 for x in r), r
        go.assert_exact(g.result(download=resident), ref)
    err, checked = g.verify_full(1, host=not resident)
    assert checked == g.tiles and err == 0.0, (err, checked)
    c2.dispose()


def test_host_resident_run(cr):
    g, ref = _int_gemm(g4.HOST_SHAPE, cruncher=cr)
    g.C.array[:] = np.nan
    g.run(resident=False)
    go.assert_exact(g.result(download=False), ref)
    err, checked = g.verify_full(1, host=True)
    assert checked == g.tiles and err == 0.0, (err, checked)


@pytest.mark.parametrize("group_m", [2, 1])
def test_host_resident_streamed_blobs(cr, group_m):
    """Four blobs per device.  The 8 tiles are 4 / group_m tile groups (the
    blob unit: one A row panel of K/2 bytes per row each), so group_m = 1 runs
    the event pipeline and group_m = 2, with fewer groups than blobs, the
    plain path.  A goes up one row panel per blob; Bt and both scale arrays
    are full reads."""
    g, ref = _int_gemm(g4.HOST_SHAPE, cruncher=cr, group_m=group_m)
    assert g.can_stream()
    g.C.array[:] = np.nan
    g.run(resident=False, stream_blobs=4)
    assert cr.last_record()["pipelined"] == (group_m == 1)
    assert g.A.elements_per_work_item * (g.N // g.BN) * g.L == g.BM * g.K // 2
    go.assert_exact(g.result(download=False), ref)
    err, checked = g.verify_full(1, host=True)
    assert checked == g.tiles and err == 0.0, (err, checked)


def test_reupload_takes_new_scales(cr):
    """SA changed on the host between two host-resident calls: the second
    call's C is the new exact product (stale packed scales would give the old one)."""
    shape = g4.HOST_SHAPE
    a, b, ea, eb, ref = g4.int_case(shape)
    g, _ = _int_gemm(shape, cruncher=cr)
    g.run(resident=False)
    go.assert_exact(g.result(download=False), ref)
    ea2 = (ea + 2) % 3 - 1
    assert (ea2 != ea).all()
    g.SA.array[:] = (127 + ea2).ravel()
    ref2 = g4.scaled(a, ea2) @ g4.scaled(b, eb).T
    assert (ref2 != ref).mean() > 0.5
    g.C.array[:] = np.nan
    g.run(resident=False)
    go.assert_exact(g.result(download=False), ref2)
    assert e8m0_to_f64(g.SA.array).max() == 2.0
    err, checked = g.verify_full(1, host=True)
    assert checked == g.tiles and err == 0.0, (err, checked)


@pytest.mark.parametrize("tile,shape,group_m", [(t, s[:2] + (256,), gm) for t in TILES for s, gm in g8.ragged_groups(t)])
def test_ragged_last_tile_group(cr, tile, shape, group_m):
    """gemm8_oracles' ragged shapes at K = 256: three tile rows under group_m
    2 and 4, the last tile group shorter than group_m.  C is prefilled with NaN, so a tile written twice (another
    one never) shows."""
    g, ref = _int_gemm(shape, cruncher=cr, tile=tile, group_m=group_m)
    assert (g.M // g.BM) % group_m != 0
    _run_exact(g, ref)
    err, checked = g.verify_full(1)
    assert checked == g.tiles and err == 0.0, (err, checked)
