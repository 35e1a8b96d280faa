"""GPU tier of the mixed MXFP8 × MXFP4 GEMM (kernels/sgemm_mxf8f4.hip,
GemmMxFp8Fp4): the single-instruction probe of the scaled MFMA with an e4m3 A
against an e2m1 Bt first (which k a byte or nibble supplies, which scale byte
meets which data, 0xFF, the e4m3 NaN codes, the ends of the scale range,
subnormal results, sums of neighbouring products), then exact data (small
integers against all 15 e2m1 values under mixed block scales, the
scale-mapping probe, cancelling extreme scales, scale byte 0xFF, a NaN code,
ragged tile groups), random wide-range data against a derived bound, the
multi-device, host-resident and streamed paths and a re-upload, operands
quantised on the device, and the output modes with a two-layer chain.
gemm84_oracles.py has the cases and their arguments."""
import numpy as np
import pytest

import cekirdekler_amd as ck
import gemm84_oracles as g84
import gemm_oracles as go
from cekirdekler_amd.ops.gemm import (MX_OUTPUTS, MXF8F4_TILES, GemmMxFp8Fp4, e8m0_to_f64, from_fp4_e2m1_codes,
                                      from_fp8_e4m3_bits, from_mxfp4, from_mxfp8, to_mxfp4, to_mxfp8, unpack_fp4)
from cekirdekler_amd.ops.library import library
from test_gemm_mx_out_host import assert_same_output, host_codec

pytestmark = pytest.mark.gpu

TILES = sorted(MXF8F4_TILES)
TILE_SHAPES = [(t, s) for t in TILES for s in g84.SHAPES[t]]
LIBS = ("sgemm_mxf8f4", "sgemm_mxf8f4_out", "mx_quantize", "mx4_quantize")


@pytest.fixture(scope="module")
def cr():
    c = ck.ClNumberCruncher(ck.ClPlatforms.all().gpus()[0], "", prebuilt=library(*LIBS))
    yield c
    c.dispose()


# --------------------------------------------------------------------------- the single-instruction probe

@pytest.fixture(scope="module")
def probe_answers():
    """One launch of gemm84_oracles.PROBE_SRC, one wave and one mixed
    v_mfma_scale_f32_16x16x128_f8f6f4 per question: name → C [16][16]."""
    c = ck.ClNumberCruncher(ck.ClPlatforms.all().gpus()[0], g84.PROBE_SRC)
    assert c.error_code() == 0, c.error_message()
    names, *bufs = g84.probe_buffers()
    arrays = [ck.ClArray(x.copy()) for x in bufs]
    for x in arrays:
        x.write = False
    out = ck.ClArray(np.full(256 * len(names), -7.0, np.float32))
    out.read = False
    out.elements_per_work_item = 4
    arrays[0].next_param(*arrays[1:], out).compute(c, 1, g84.PROBE_KERNEL, 64 * len(names), 64)
    got = out.array.reshape(len(names), 16, 16).copy()
    c.dispose()
    for i, n in enumerate(names):
        print(g84.probe_report(n, got[i]))
    return dict(zip(names, got))


def test_probe_k_map_as_measured(probe_answers):
    """Question 1.  Measured on an MI355X: each operand keeps the map of its
    own format.  A (e4m3): lane l, q = l / 16, supplies k in [16q, 16q + 16) in
    registers 0 … 3 and k in [64 + 16q, 64 + 16q + 16) in registers 4 … 7.  Bt
    (e2m1): k in [32q, 32q + 32) in natural order, low nibble first, registers
    4 … 7 ignored (the probe fills them with 6.0).  Under those loaders
    position k of either operand meets position k of the other, for all 128 k."""
    for operand in "ab":
        km = g84.measured_k_map(probe_answers, operand)
        print(f"probe84 k map of {operand}:", km.tolist())
        np.testing.assert_array_equal(km, np.arange(128))


def test_probe_scale_map_as_measured(probe_answers):
    """Question 2.  Measured on an MI355X: for A and for Bt alike the scale
    byte of lane l applies to row l % 16 and MX block l / 16 of the
    instruction's 128 k, and op_sel = b picks bits 8b … 8b+7 of the scale
    register, independently per operand."""
    for operand in "ab":
        for o in range(4):
            row, block, want_block = g84.measured_scale_map(probe_answers, operand, o)
            print(f"probe84 scale map of {operand}, op_sel {o}: rows {row.tolist()} blocks {block.tolist()}")
            np.testing.assert_array_equal(row, np.arange(16))
            np.testing.assert_array_equal(block, want_block)
            name = f"scale_map_{operand}{o}"
            go.assert_nonfinite(probe_answers[name], g84.probe_problems()[name]["want"])


def test_probe_special_values_as_measured(probe_answers):
    """Question 3 and the dense baseline: a scale byte 0xFF makes its block
    NaN, zeros included; an e4m3 NaN code in A makes its row of C NaN, 0·NaN
    included; exponent sums of +254, 0 and -254 give ±Inf, the exact product
    and ±0; results in fp32's subnormal range are exact — the IEEE / OCP
    answer in every case."""
    for n in g84.PROBE_IEEE:
        go.assert_nonfinite(probe_answers[n], g84.probe_problems()[n]["want"])


def test_probe_adjacent_sums_as_measured(probe_answers):
    """Question 4, as measured on an MI355X (profiles/gemm_mxf8f4.md has the
    raw values).  Inside a group of 8 neighbouring k the mixed form does what
    the pure e4m3 form does: 2^10 beside 2^(9-i-j%4) keeps the smaller product
    while it lies within 14 bits from the larger one's top and drops it whole
    below (gemm84_oracles.adjacent_k_as_measured).  Across a block boundary
    (2^16 at k = 31 beside 2^(14-i-j) at k = 32) the sum is the correctly
    rounded fp32 result."""
    go.assert_exact(probe_answers["adjacent_k"], g84.adjacent_k_as_measured())
    go.assert_nonfinite(probe_answers["adjacent_blocks"], g84.probe_problems()["adjacent_blocks"]["want"])


# --------------------------------------------------------------------------- exact data

def _int_gemm(shape, **kw):
    a, b, ea, eb, ref = g84.int_case(shape)
    g = GemmMxFp8Fp4(*shape, fill="none", **kw)
    g84.set_operands(g, a, b, ea, eb)
    return g, ref


def _run_exact(g, want):
    g.C.array[:] = np.nan
    g.run(resident=True)
    go.assert_exact(g.result(), want)


@pytest.mark.parametrize("tile,shape", TILE_SHAPES)
def test_exact_integers_with_scales(cr, tile, shape):
    """C equals the float64 product of the scaled values bit for bit
    (gemm84_oracles.int_case has the argument and asserts its arithmetic)."""
    g, ref = _int_gemm(shape, cruncher=cr, tile=tile, group_m=2)
    assert shape[2] * 1536 < 2 ** 24 and np.abs(ref * 8).max() < 2 ** 24
    _run_exact(g, ref)


@pytest.mark.parametrize("coeff", g84.PROBE_SA_BLOCK_COEFF)
@pytest.mark.parametrize("tile", TILES)
def test_scale_mapping_probe(cr, tile, coeff):
    """A picks one k per row, SA and SB vary with row and block, Bt is
    asymmetric in n and k: C[m][n] is the one surviving product.  A wrong k
    order of A, exchanged steps, swapped nibbles, SA stepped by the K-tile or
    a wrong op_sel give another C
    (test_mxf8f4_host.py::test_scale_mapping_probe_distinguishes_on_the_host)."""
    shape, pick, a, b, ea, eb = g84.probe_case(coeff)
    want, wrong = g84.probe_expected_and_wrong(coeff)
    g = GemmMxFp8Fp4(*shape, cruncher=cr, tile=tile, fill="none")
    g84.set_operands(g, a, b, ea, eb)
    assert (want != wrong["unit scales"]).mean() > 0.5
    _run_exact(g, want)


@pytest.mark.parametrize("tile", TILES)
def test_cancelling_extreme_scales(cr, tile):
    """SA = 2^-60 with SB = 2^60 gives the unit-scale product exactly, SA = SB
    = 2^40 that product times 2^80: the exponents are applied as exponents."""
    shape = (256, 256, 256)
    a, b, _, _, _ = g84.int_case(shape)
    ref = a.astype(np.float64) @ b.astype(np.float64).T
    assert np.abs(ref).max() > 0
    for ea, eb, factor in ((-60, 60, 1.0), (40, 40, 2.0 ** 80)):
        g = GemmMxFp8Fp4(*shape, cruncher=cr, tile=tile, fill="none")  # resident operands go up once per object
        g84.set_operands(g, a, b, ea, eb)
        _run_exact(g, ref * factor)


@pytest.mark.parametrize("operand", ["A", "B"])
@pytest.mark.parametrize("tile", TILES)
def test_scale_byte_ff_poisons_its_row_or_column(cr, tile, operand):
    """One scale byte 0xFF in SA (row 177, a block of the second K-tile), then
    in SB (row 150, first K-tile): exactly that row (column) of C is NaN, zero
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


@pytest.mark.parametrize("code", [0x7F, 0xFF])
@pytest.mark.parametrize("tile", TILES)
def test_e4m3_nan_code_poisons_its_row(cr, tile, code):
    """One e4m3 NaN code in A (row 93, k = 340: the second K-tile, the high
    half of a lane's bytes): exactly that row of C is NaN, 0·NaN included, and
    every other element the exact product."""
    shape = (256, 256, 512)
    g, ref = _int_gemm(shape, cruncher=cr, tile=tile)
    b = g84.int_case(shape)[1]
    assert (b[:, 340] == 0).any()
    g.A.array.reshape(g.M, g.K)[93, 340] = code
    cls = np.zeros(ref.shape, np.int8)
    cls[93] = go.NAN
    assert np.isnan(g.reference()).sum() == 256
    g.C.array[:] = 1.0
    g.run(resident=True)
    go.assert_nonfinite(g.result(), (cls, np.where(cls == go.FINITE, ref, 0.0)))


@pytest.mark.parametrize("tile,shape,group_m", [(t, s, gm) for t in TILES for s, gm in g84.RAGGED])
def test_ragged_last_tile_group(cr, tile, shape, group_m):
    """Three tile rows under group_m 2 and 4: the last tile group is shorter
    than group_m.  C is prefilled with NaN, so a tile written twice (another
    one never) shows."""
    g, ref = _int_gemm(shape, cruncher=cr, tile=tile, group_m=group_m)
    assert g.M // g.BM == 3 and (g.M // g.BM) % group_m != 0
    _run_exact(g, ref)
    err, checked = g.verify_full(1)
    assert checked == g.tiles and err == 0.0, (err, checked)


# --------------------------------------------------------------------------- random data

@pytest.mark.parametrize("tile", TILES)
def test_random_wide_range_data_within_derived_bound(cr, tile):
    """|C - ref| <= K · 2^-23 · Σ_k |a_k·b_k| per element, a and b the
    dequantised operands (test_gpu_gemm_mxfp8.py's bound and caveats: exact
    products, K fp32 additions each off by at most one unit in the last place
    of a partial sum <= Σ|a·b|; the power-of-two scales add no rounding while
    nothing leaves fp32's normal range: A's elements are at least 2^-9 under
    block scales of at least 2^-21, Bt's at least 2^-1 under scales of at
    least 2^-15, so every nonzero product is above 2^-46).  The probe shows the
    mixed form summing as the pure e4m3 form does (14 bits inside a group of 8
    neighbouring k, full width across blocks), so the bound and its caveat are
    that test's: it holds for these uniform draws, not for every data set."""
    M, N, K = g84.RANDOM_SHAPE
    seed = 3
    g = GemmMxFp8Fp4(M, N, K, cruncher=cr, tile=tile, fill="random", seed=seed)
    a = from_mxfp8(g.A.array.reshape(M, K), g.SA.array.reshape(M, K // 32)).astype(np.float64)
    b = from_mxfp4(g.B.array.reshape(N, K // 2), g.SB.array.reshape(N, K // 32)).astype(np.float64)
    assert int(g.SA.array.min()) >= 127 - 21 and int(g.SB.array.min()) >= 127 - 15
    assert int(g.SA.array.max()) < 0xFF and int(g.SB.array.max()) < 0xFF
    np.testing.assert_array_equal(a, g84.scaled(from_fp8_e4m3_bits(g.A.array).reshape(M, K),
                                                g.SA.array.reshape(M, K // 32).astype(np.int64) - 127))
    np.testing.assert_array_equal(b, g84.scaled(from_fp4_e2m1_codes(unpack_fp4(g.B.array)).reshape(N, K),
                                                g.SB.array.reshape(N, K // 32).astype(np.int64) - 127))
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
    assert np.array_equal(to_mxfp8(raw[0])[0].ravel(), g.A.array) and np.array_equal(to_mxfp4(raw[1])[1].ravel(),
                                                                                       g.SB.array)
    full = raw[0].astype(np.float64) @ raw[1].astype(np.float64).T
    e2e = float(np.abs(c - full).max() / np.abs(full).max())
    e2e_rms = float(np.sqrt(((c - full) ** 2).mean() / (full ** 2).mean()))
    print(f"mxf8f4 {tile} {M}x{N}x{K}: worst |C-ref|/bound = {ratio:.3e}, max|C-ref|/max|ref| = {rel:.3e}, "
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
    c2 = ck.ClNumberCruncher(g0 + g0, "", prebuilt=library("sgemm_mxf8f4"))
    g, ref = _int_gemm(g84.TWO_DEVICE_SHAPE, cruncher=c2)
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
    g, ref = _int_gemm(g84.HOST_SHAPE, cruncher=cr)
    g.C.array[:] = np.nan
    g.run(resident=False)
    go.assert_exact(g.result(download=False), ref)
    err, checked = g.verify_full(1, host=True)
    assert checked == g.tiles and err == 0.0, (err, checked)


@pytest.mark.parametrize("group_m", [2, 1])
def test_host_resident_streamed_blobs(cr, group_m):
    """Four blobs per device.  The 8 tiles are 4 / group_m tile groups (the
    blob unit: one A row panel of K bytes per row each), so group_m = 1 runs
    the event pipeline and group_m = 2, with fewer groups than blobs, the
    plain path.  A goes up one row panel per blob; Bt and both scale arrays
    are full reads."""
    g, ref = _int_gemm(g84.HOST_SHAPE, cruncher=cr, group_m=group_m)
    assert g.can_stream() and g.tiles == 8
    g.C.array[:] = np.nan
    g.run(resident=False, stream_blobs=4)
    assert cr.last_record()["pipelined"] == (group_m == 1)
    assert g.A.elements_per_work_item * (g.N // g.BN) * g.L == g.BM * g.K
    go.assert_exact(g.result(download=False), ref)
    err, checked = g.verify_full(1, host=True)
    assert checked == g.tiles and err == 0.0, (err, checked)


def test_reupload_takes_new_scales(cr):
    """SA changed on the host between two host-resident calls: the second
    call's C is the new exact product (stale packed scales would give the old one)."""
    shape = g84.HOST_SHAPE
    a, b, ea, eb, ref = g84.int_case(shape)
    g, _ = _int_gemm(shape, cruncher=cr)
    g.run(resident=False)
    go.assert_exact(g.result(download=False), ref)
    ea2 = (ea + 2) % 3 - 1
    assert (ea2 != ea).all()
    g.SA.array[:] = (127 + ea2).ravel()
    ref2 = g84.scaled(a, ea2) @ g84.scaled(b, eb).T
    assert (ref2 != ref).mean() > 0.5
    g.C.array[:] = np.nan
    g.run(resident=False)
    go.assert_exact(g.result(download=False), ref2)
    assert e8m0_to_f64(g.SA.array).max() == 2.0


# --------------------------------------------------------------------------- operands made on the device

def _same_bits(got, want):
    assert got.dtype == want.dtype == np.float32 and not np.isnan(want).any()
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (len(bad), bad[:4].tolist())


@pytest.mark.parametrize("tile", TILES)
def test_device_quantised_operands_equal_the_host_codec(cr, tile):
    """quantize("A") (MXFP8) and quantize("B") (MXFP4) on fp32 input: C is bit
    for bit that of a run on the host codecs' operands, and the synced codes
    and scales are the host codecs'."""
    M, N, K = 256, 512, 512
    rng = np.random.default_rng(8)
    xs = [np.ldexp(rng.uniform(-1, 1, (rows, K // 32, 32)), rng.integers(-12, 13, (rows, K // 32, 1)))
          .astype(np.float32).reshape(rows, K) for rows in (M, N)]
    host = GemmMxFp8Fp4(M, N, K, cruncher=cr, tile=tile, fill="none")
    for arr, sc, (codes, scales) in ((host.A, host.SA, to_mxfp8(xs[0])), (host.B, host.SB, to_mxfp4(xs[1]))):
        arr.array[:] = codes.ravel()
        sc.array[:] = scales.ravel()
    host.C.array[:] = np.nan
    host.run()
    want = host.result()
    dev = GemmMxFp8Fp4(M, N, K, cruncher=cr, tile=tile, fill="none")
    dev.quantize("A", xs[0])
    dev.quantize("B", xs[1])
    assert dev._stale == {"A", "B"}
    dev.C.array[:] = np.nan
    dev.run()
    assert cr.last_record()["h2d_bytes"] <= dev.dims.nbytes, cr.last_record()  # at most the dims array
    _same_bits(dev.result(), want)
    dev.sync_operands()
    for d, h in ((dev.A, host.A), (dev.SA, host.SA), (dev.B, host.B), (dev.SB, host.SB)):
        np.testing.assert_array_equal(d.array, h.array)


# --------------------------------------------------------------------------- output modes

SENTINEL = {"bfloat16": 0xAAAA, "mxfp8": 0xAA, "mxfp4": 0xAA}
_PLAIN = {}


def _plain_c(cr, tile):
    """The plain kernel's C on the class's default fill at OUT_SHAPE, once per tile."""
    if tile not in _PLAIN:
        g = GemmMxFp8Fp4(*g84.OUT_SHAPE, cruncher=cr, tile=tile)
        g.C.array[:] = np.nan
        g.run()
        c = g.result()
        assert np.isfinite(c).all() and np.ptp(np.frexp(np.abs(c[c != 0]))[1]) > 20 and (c < 0).mean() > 0.3
        c.setflags(write=False)
        _PLAIN[tile] = c
    return _PLAIN[tile]


def _run_out(g):
    """One resident call with the outputs pre-filled on host and device, so
    that an unwritten byte shows; (Y, SY, packed) as stored, from device 0."""
    arrays = [g.Y] + ([g.SY, g.Yp] if g.SY is not None else [])
    for a in arrays:
        a.array[:] = SENTINEL[g.out] if a is g.Y else (0xAA if a is g.SY else 0xAAAAAAAA)
        g.cr.upload(a, 0)
    g.run()
    for a in arrays:
        a.array[:] = 0x55
        g.cr.download(a, 0)
    return tuple(a.array.copy() for a in arrays) + (None,) * (3 - len(arrays))


@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("out", MX_OUTPUTS)
@pytest.mark.parametrize("tile", TILES)
def test_output_equals_the_codec_of_the_plain_c(cr, tile, out, act):
    """Y, SY and Yp are bit for bit the host codec applied to the plain
    kernel's C of the same operands (the class's default fill, block factors
    2^-12 … 2^12)."""
    c = _plain_c(cr, tile)
    g = GemmMxFp8Fp4(*g84.OUT_SHAPE, cruncher=cr, tile=tile, out=out, act=act)
    assert_same_output(_run_out(g), host_codec(c, out, act), out, (tile, out, act))


@pytest.mark.parametrize("tile", TILES)
def test_two_layer_chain_equals_the_host_model(cr, tile):
    """Layer 1 with out="mxfp8", act="relu"; layer 2 takes its resident output
    as A.  What layer 2 multiplied is the host codec of layer 1's plain C, and
    its C is bit for bit that of a fresh GEMM fed those codes by upload."""
    M, N1, K1 = g84.OUT_SHAPE
    g1 = GemmMxFp8Fp4(M, N1, K1, cruncher=cr, tile=tile, out="mxfp8", act="relu")
    g2 = GemmMxFp8Fp4(M, 256, N1, cruncher=cr, tile=tile, seed=3)
    g2.take_operand("A", g1)
    g1.run()
    g2.C.array[:] = np.nan
    g2.run()
    rec = cr.last_record()
    assert rec["h2d_bytes"] == g2.dims.nbytes + g2.B.nbytes + g2._SBp.nbytes, rec
    c2 = g2.result()
    g2.sync_operands()
    want = host_codec(_plain_c(cr, tile), "mxfp8", "relu")
    np.testing.assert_array_equal(g2.A.array, want[0].ravel())
    np.testing.assert_array_equal(g2.SA.array, want[1].ravel())
    g3 = GemmMxFp8Fp4(M, 256, N1, cruncher=cr, tile=tile, fill="none")
    for dst, src in ((g3.A, g2.A), (g3.SA, g2.SA), (g3.B, g2.B), (g3.SB, g2.SB)):
        dst.array[:] = src.array
    g3.C.array[:] = np.nan
    g3.run()
    _same_bits(c2, g3.result())
    # and the host model of the whole chain: the float64 product of the dequantised operands.  Layer 2's A is
    # MXFP8 data of a wide range inside a block (e4m3 spans 2^-9 … 448 under one scale), so the measured cut of
    # the e4m3 path applies: in a group of 8 neighbouring k every product is cut to a multiple of 2^(E-13), E
    # the exponent of the group's largest product p_max >= 2^E; that is less than 2^(E-13) <= 2^-13·|p_max| per
    # product and 8·2^-13·|p_max| <= 2^-10·Σ_group|p| per group, on top of the K fp32 additions' K·2^-23·Σ|a·b|
    a2 = from_mxfp8(want[0], want[1]).astype(np.float64)
    b2 = g2._operand("B")
    ref = a2 @ b2.T
    np.testing.assert_array_equal(ref, g2.reference())
    bound = (N1 * 2.0 ** -23 + 2.0 ** -10) * (np.abs(a2) @ np.abs(b2).T)
    err = np.abs(c2.astype(np.float64) - ref)
    print(f"mxf8f4 chain {tile}: worst |C2-ref|/bound = {float((err[bound > 0] / bound[bound > 0]).max()):.3e}")
    assert (err <= bound).all()
