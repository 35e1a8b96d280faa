"""GPU tier of the MX GEMMs' output modes (kernels/sgemm_mx_out.hip): bf16,
MXFP8 and MXFP4 outputs of both operand formats and both tile structures,
with and without ReLU.  Every comparison is exact: against the host codec of
a float64-exact product (integers under mixed block scales), against the host
codec of the plain kernel's C (wide-range data, NaN / Inf / zero rows), through
a chain of two layers that shares the resident output as the next operand,
on two and three logical devices with every replica whole, and against the
host codec of designed fp32 accumulator bits that the GEMM itself is made to
produce (gemm_out_oracles.py: ties, saturation, subnormals, denormals, single
Inf elements and NaN columns; −0 and a NaN element on its own cannot be
reached that way and stay with the host tier).

Shapes: at least two tiles each way, M ≠ N (a transposed or mis-pitched store
shows), K = 256 (one K-tile of MXFP4, two of MXFP8), one ragged tile group.
The designed bits take two tile rows of one tile column at K = J·N, J the
pieces per element (14 for MXFP8 operands, 27 or 28 for MXFP4 ones)."""
import numpy as np
import pytest

import cekirdekler_amd as ck
import gemm_out_oracles as goo
from cekirdekler_amd.ops.gemm import (MX_OUTPUTS, GemmMxFp4, GemmMxFp8, pack_fp4, to_fp4_e2m1_codes,
                                      to_fp8_e4m3_bits, unpack_fp4)
from cekirdekler_amd.ops.library import library
from cekirdekler_amd.ops.quantize import mxfp8_reference
from test_gemm_mx_out_host import assert_same_output, bf16_is_nan, host_codec

pytestmark = pytest.mark.gpu

FORMATS = {"mxfp8": GemmMxFp8, "mxfp4": GemmMxFp4}
LIBS = ("sgemm_mxfp8", "sgemm_mxfp4", "mx_quantize", "mx4_quantize", "sgemm_mx_out")
# (tile, (M, N, K), group_m): (512, 768) has one group of two tile rows under
# group_m = 4, (768, 512) a ragged second group under group_m = 2
CASES = [("256x256pbx", (512, 768, 256), 4), ("256x256pbx", (768, 512, 256), 2), ("128x128", (256, 384, 256), 4)]
ACTS = (None, "relu")
SENTINEL = {"bfloat16": 0xAAAA, "mxfp8": 0xAA, "mxfp4": 0xAA}


@pytest.fixture(scope="module")
def cr():
    c = ck.ClNumberCruncher(ck.ClPlatforms.all().gpus()[0], "", prebuilt=library(*LIBS))
    yield c
    c.dispose()


def _run_out(g, resident=True):
    """One call with the outputs pre-filled on host and device, so that an
    unwritten byte shows; returns (Y, SY, packed) as stored, from device 0."""
    arrays = [g.Y] + ([g.SY, g.Yp] if g.SY is not None else [])
    for a in arrays:
        a.array[:] = SENTINEL[g.out] if a is g.Y else (0xAA if a is g.SY else 0xAAAAAAAA)
        g.cr.upload(a, 0)
    g.run(resident=resident)
    return _stored(g, download=resident)


def _stored(g, download=True, dev=0):
    arrays = [g.Y] + ([g.SY, g.Yp] if g.SY is not None else [])
    if download:
        for a in arrays:
            a.array[:] = 0x55
            g.cr.download(a, dev)
    return tuple(a.array.copy() for a in arrays) + (None,) * (3 - len(arrays))


def _plain_c(cls, shape, tile, group_m, cr, fill=None):
    """The plain kernel's C (fp32 row-major) on the operands ``fill`` sets."""
    g = cls(*shape, cruncher=cr, tile=tile, group_m=group_m)
    if fill is not None:
        fill(g)
    g.C.array[:] = np.nan
    g.run()
    return g.result()


# ----------------------------------------------- 1: independent of the plain kernel

_INT_CACHE = {}


def _scaled(x, e):
    """float64 [rows][K] elements times 2^e per block of 32 (exact)."""
    rows, K = x.shape
    return (np.asarray(x, np.float64).reshape(rows, K // 32, 32) * np.ldexp(1.0, e)[..., None]).reshape(rows, K)


def _int_case(shape):
    """Integers in [-4, 4] (exact in e4m3 and in e2m1), scale exponents in
    {-2 .. 2} per block, independently for A and B, and the float64 product,
    once per shape.  In units of 2^-4 every product is an integer of at most
    4·4·2^(2+2+4) = 2^12 and every partial sum an integer below K·2^12 < 2^24:
    exact in fp32 in any summation order, so C is known exactly.  The products
    of 8 neighbouring k lie within one block pair and differ by at most 2^4,
    far inside the bits the scaled instruction keeps."""
    if shape not in _INT_CACHE:
        M, N, K = shape
        rng = np.random.default_rng(sum(shape))
        a, b = rng.integers(-4, 5, (M, K)), rng.integers(-4, 5, (N, K))
        ea, eb = rng.integers(-2, 3, (M, K // 32)), rng.integers(-2, 3, (N, K // 32))
        assert K * 2 ** 12 < 2 ** 24
        ref = _scaled(a, ea) @ _scaled(b, eb).T
        assert np.array_equal(np.rint(ref * 16), ref * 16) and np.abs(ref * 16).max() < 2 ** 24
        assert (ref < 0).mean() > 0.3 and (ref > 0).mean() > 0.3  # ReLU has something to do
        c32 = ref.astype(np.float32)
        assert np.array_equal(c32.astype(np.float64), ref)
        for x in (a, b, ea, eb, c32):
            x.setflags(write=False)
        _INT_CACHE[shape] = (a, b, ea, eb, c32)
    return _INT_CACHE[shape]


def _set_ints(g, a, b, ea, eb):
    enc = (lambda x: pack_fp4(to_fp4_e2m1_codes(x))) if g.FORMAT == "mxfp4" else to_fp8_e4m3_bits
    g.A.array[:] = enc(np.asarray(a, np.float32)).ravel()
    g.B.array[:] = enc(np.asarray(b, np.float32)).ravel()
    g.SA.array[:] = (127 + ea).ravel()
    g.SB.array[:] = (127 + eb).ravel()


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("out", MX_OUTPUTS)
@pytest.mark.parametrize("tile,shape,group_m", CASES)
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_exact_product_through_every_output(cr, fmt, tile, shape, group_m, out, act):
    a, b, ea, eb, c32 = _int_case(shape)
    g = FORMATS[fmt](*shape, cruncher=cr, tile=tile, group_m=group_m, fill="none", out=out, act=act)
    _set_ints(g, a, b, ea, eb)
    got = _run_out(g)
    assert_same_output(got, host_codec(c32, out, act), out, (fmt, tile, shape, out, act))
    # result() is the decoded output
    if out == "bfloat16":
        want = host_codec(c32, out, act)[0]
        np.testing.assert_array_equal(g.result().view(np.uint32) >> 16, want.astype(np.uint32))


# ------------------------------------------ 2: against the plain kernel, wide range

_PLAIN = {}


def _plain_default(cr, fmt, tile, shape, group_m):
    key = (fmt, tile, shape, group_m)
    if key not in _PLAIN:
        c = _plain_c(FORMATS[fmt], shape, tile, group_m, cr)
        assert np.isfinite(c).all() and np.ptp(np.frexp(np.abs(c[c != 0]))[1]) > 20  # a wide range of binades
        c.setflags(write=False)
        _PLAIN[key] = c
    return _PLAIN[key]


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("out", MX_OUTPUTS)
@pytest.mark.parametrize("tile,shape,group_m", CASES)
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_equals_the_codec_of_the_plain_c(cr, fmt, tile, shape, group_m, out, act):
    """The classes' default fill (block factors 2^-12 .. 2^12): the same
    operands through the plain tile and through the output mode."""
    c = _plain_default(cr, fmt, tile, shape, group_m)
    g = FORMATS[fmt](*shape, cruncher=cr, tile=tile, group_m=group_m, out=out, act=act)
    assert_same_output(_run_out(g), host_codec(c, out, act), out, (fmt, tile, shape, out, act))


# ------------------------------------------------------------------- 3: specials


def _specials(g):
    """One A row under scale byte 0xFF (a NaN row of C); one A block and one
    B block at byte 254, each with the format's largest element in one place
    and zeros elsewhere, so that a single product per element of C overflows
    (±Inf by the other operand's sign, no Inf − Inf); one zero A row."""
    kb, per = g.K // 32, 32 // g.PER_ITEM  # bytes of a block
    big = 0x7E if g.FORMAT == "mxfp8" else 0x07  # 448, or 6 in the low nibble
    for arr, sc, rows, r in ((g.A, g.SA, g.M, g.BM + 37), (g.B, g.SB, g.N, g.BN + 70)):
        sc.array.reshape(rows, kb)[r, 1] = 254
        arr.array.reshape(rows, -1)[r, per:2 * per] = 0
        arr.array.reshape(rows, -1)[r, per + 3] = big
    g.SA.array.reshape(g.M, kb)[5] = 0xFF
    g.A.array.reshape(g.M, -1)[g.M - 3] = 0


@pytest.mark.parametrize("out", MX_OUTPUTS)
@pytest.mark.parametrize("tile,shape,group_m", [CASES[0], CASES[2]])
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_specials(cr, fmt, tile, shape, group_m, out):
    cls = FORMATS[fmt]
    key = ("specials", fmt, tile, shape)
    if key not in _PLAIN:
        c = _plain_c(cls, shape, tile, group_m, cr, fill=_specials)
        c.setflags(write=False)
        _PLAIN[key] = c
    c = _PLAIN[key]
    BM, BN = cls.TILE_TABLE[tile][:2]
    assert np.isnan(c[5]).all() and (c[BM + 37] == np.inf).any() and (c[BM + 37] == -np.inf).any()
    assert np.isinf(np.delete(c[:, BN + 70], 5)).any()
    assert (c[shape[0] - 3].view(np.uint32) << 1 == 0).all() and (c[np.isfinite(c)] < 0).any()
    for act in ACTS:
        g = cls(*shape, cruncher=cr, tile=tile, group_m=group_m, out=out, act=act)
        _specials(g)
        got = _run_out(g)
        assert_same_output(got, host_codec(c, out, act), out, (fmt, tile, out, act))
        Y, SY = got[0].reshape(shape[0], -1), None if got[1] is None else got[1].reshape(shape[0], -1)
        if out == "bfloat16":
            assert bf16_is_nan(Y[5]).all()
            assert (Y[shape[0] - 3] & 0x7FFF == 0).all()
        elif out == "mxfp8":
            assert (Y[5] == 0x7F).all() and (SY[5] == 127).all() and (SY[shape[0] - 3] == 127).all()
        else:  # e2m1 has no NaN: code 0 under the block byte 0xFF
            assert (SY[5] == 0xFF).all() and (Y[5] == 0).all() and (unpack_fp4(Y[5]) == 0).all()
            assert (SY[shape[0] - 3] == 127).all() and (Y[shape[0] - 3] & 0x77 == 0).all()
        if act == "relu" and out != "bfloat16":  # negatives went to +0: no sign bit survives outside NaN rows
            sign = 0x80 if out == "mxfp8" else 0x88
            assert (np.delete(Y, 5, axis=0) & sign == 0).all()


# --------------------------------------------------------------------- 4: chain


def _chain(cr, first_fmt, out, second_fmt):
    g1 = FORMATS[first_fmt](512, 512, 256, cruncher=cr, out=out, act="relu")
    g2 = FORMATS[second_fmt](512, 256, 512, cruncher=cr, seed=3)
    return g1, g2


def _fresh_plain(cr, g2):
    """A plain GEMM of g2's class fed g2's (synced) codes and scales by upload."""
    g3 = type(g2)(g2.M, g2.N, g2.K, cruncher=cr, fill="none")
    for dst, src in ((g3.A, g2.A), (g3.SA, g2.SA), (g3.B, g2.B), (g3.SB, g2.SB)):
        dst.array[:] = src.array
    g3.C.array[:] = np.nan
    g3.run()
    return g3.result()


def _same_bits(got, want):
    assert got.dtype == want.dtype == np.float32 and not np.isnan(want).any()
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (len(bad), bad[:4].tolist())


@pytest.mark.parametrize("first_fmt,out,second_fmt", [("mxfp4", "mxfp8", "mxfp8"), ("mxfp8", "mxfp4", "mxfp4")])
def test_chain_shares_the_resident_output(cr, first_fmt, out, second_fmt):
    g1, g2 = _chain(cr, first_fmt, out, second_fmt)
    g2.take_operand("A", g1)
    g1.run()
    g2.C.array[:] = np.nan
    g2.run()
    rec = cr.last_record()
    # dims and B (its codes and packed scales) go up; nothing of A does
    assert rec["h2d_bytes"] == g2.dims.nbytes + g2.B.nbytes + g2._SBp.nbytes, rec
    assert g2._stale == {"A"}
    c2 = g2.result()
    with pytest.raises(ValueError, match=r"sync_operands\(\)"):
        g2.run(resident=False)
    g2.sync_operands()
    # what g2 multiplied is the codec of g1's plain C
    plain = FORMATS[first_fmt](512, 512, 256, cruncher=cr)
    plain.run()
    want = host_codec(plain.result(), out, "relu")
    np.testing.assert_array_equal(g2.A.array, want[0].ravel())
    np.testing.assert_array_equal(g2.SA.array, want[1].ravel())
    _same_bits(c2, _fresh_plain(cr, g2))
    # a second round: g1 again, g2 again without any upload but dims
    g1.run()
    assert g2._stale == {"A"}
    g2.run()
    assert cr.last_record()["h2d_bytes"] <= g2.dims.nbytes, cr.last_record()
    _same_bits(g2.result(), c2)


def test_chain_through_the_bf16_output(cr):
    """The path for a user kernel between the layers: Y is a resident bf16
    ClArray, which quantize() takes where it lies."""
    g1, g2 = _chain(cr, "mxfp4", "bfloat16", "mxfp8")
    g1.run()
    assert g1.Y.is_bf16 and g1.Y.read is False
    g2.quantize("A", g1.Y)
    g2.C.array[:] = np.nan
    g2.run()
    assert cr.last_record()["h2d_bytes"] == g2.dims.nbytes + g2.B.nbytes + g2._SBp.nbytes, cr.last_record()
    c2 = g2.result()
    g1.result()  # downloads Y
    codes, scales = mxfp8_reference(g1.Y.array.reshape(512, 512))
    g2.sync_operands()
    np.testing.assert_array_equal(g2.A.array, codes.ravel())
    np.testing.assert_array_equal(g2.SA.array, scales.ravel())
    _same_bits(c2, _fresh_plain(cr, g2))


# ------------------------------------------------------ 5: several logical devices

MULTI_SHAPE, MULTI_TILE = (1024, 512, 256), "256x256pbx"


@pytest.mark.parametrize("ndev,fmt,out", [(2, "mxfp8", "mxfp4"), (3, "mxfp4", "mxfp8"), (2, "mxfp4", "bfloat16"),
                                          (3, "mxfp8", "mxfp8")])
def test_logical_devices_hold_whole_outputs(cr, ndev, fmt, out):
    want = host_codec(_plain_default(cr, fmt, MULTI_TILE, MULTI_SHAPE, 1), out, "relu")
    g0 = ck.ClPlatforms.all().gpus()[0]
    devs = g0
    for _ in range(ndev - 1):
        devs = devs + g0
    c = ck.ClNumberCruncher(devs, "", prebuilt=library(*LIBS))
    try:
        c.set_time_scale(ndev - 1, 1.7)  # moves the split after the first call
        g = FORMATS[fmt](*MULTI_SHAPE, cruncher=c, tile=MULTI_TILE, group_m=1, out=out, act="relu")
        unit = g._group_work_items()
        arrays = [g.Y] + ([g.SY, g.Yp] if g.SY is not None else [])
        for it in range(3):
            g.run()
            assert len(g.records) == (1 if out == "bfloat16" else 2)
            r = g.records[0]["ranges"]
            assert len(r) == ndev and sum(r) == g.global_range and all(v % unit == 0 for v in r), r
            for rec in g.records:
                assert rec["d2h_bytes"] == 0, rec
            for d in range(ndev):  # every replica is whole
                assert_same_output(_stored(g, dev=d), want, out, (it, d))
        # one host-resident call downloads exactly the slices
        for a in arrays:
            a.array[:] = 0x55
        g.run(resident=False)
        assert g.records[0]["d2h_bytes"] == g.Y.nbytes + (g.SY.nbytes if g.SY is not None else 0), g.records[0]
        if g.Yp is not None:
            assert g.records[1]["d2h_bytes"] == g.Yp.nbytes, g.records[1]
        assert_same_output(_stored(g, download=False), want, out, "host-resident")
    finally:
        c.dispose()


# ------------------------------------------ 6: designed fp32 accumulator bits

_DESIGNED = {}


def _designed_shape(fmt, tile):
    M, N = goo.SHAPES[tile]
    return M, N, goo.decompose_tile(tile, fmt)[4] * N


def _set_designed(g, fmt, tile):
    """The operands of gemm_out_oracles.decompose_tile through _set_ints,
    encoded once per (format, tile)."""
    key = ("operands", fmt, tile)
    arrays = (g.A, g.B, g.SA, g.SB)
    if key not in _DESIGNED:
        _set_ints(g, *goo.decompose_tile(tile, fmt)[:4])
        _DESIGNED[key] = tuple(x.array.copy() for x in arrays)
    for dst, src in zip(arrays, _DESIGNED[key]):
        dst.array[:] = src


@pytest.mark.parametrize("tile", sorted(goo.SHAPES))
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_plain_kernel_builds_the_designed_accumulators(cr, fmt, tile):
    """The plain MX GEMM on accumulators that span fp32's whole range: every
    finite and Inf element of gemm_out_oracles.gpu_target bit for bit, NaN
    exactly in its NaN columns.  What the output-mode cases below convert is
    therefore the designed bits."""
    target = goo.gpu_target(tile)
    c = _plain_c(FORMATS[fmt], _designed_shape(fmt, tile), tile, 4, cr, fill=lambda g: _set_designed(g, fmt, tile))
    fin, inf, nan = goo.classes(target)
    got_nan = goo.classes(c)[2]
    bad = np.argwhere((got_nan != nan) | (~nan & (c.view(np.uint32) != target.view(np.uint32))))
    assert bad.size == 0, (fmt, tile, len(bad), [(int(m), int(n), hex(int(target.view(np.uint32)[m, n])),
                                                  hex(int(c.view(np.uint32)[m, n]))) for m, n in bad[:6]])
    # the NaN the epilogue is handed carries a sign bit: the e4m3 NaN code has a sign to drop
    assert (c.view(np.uint32)[nan] >> 31).any()
    assert nan.sum() >= 2 * target.shape[0] and inf.sum() >= 32 and (np.abs(target[fin]) < 2.0 ** -126).sum() > 100


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("out", MX_OUTPUTS)
@pytest.mark.parametrize("tile", sorted(goo.SHAPES))
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_designed_accumulators_through_every_output(cr, fmt, tile, out, act):
    """gemm8_out.h on designed bits: rounding ties ± 1 ulp of bf16, e4m3 and
    e2m1, the carry to Inf, saturation, subnormal codes and fp32 denormals,
    a single Inf or NaN element in a finite block (the NaN of a NaN column;
    the two tiles' columns meet all four lanes of an MXFP4 block), negatives, denormals and
    NaN under ReLU; every designed block in both bytes of a wave's scale
    word (gemm_out_oracles.place)."""
    target = goo.gpu_target(tile)
    g = FORMATS[fmt](*_designed_shape(fmt, tile), cruncher=cr, tile=tile, group_m=4, fill="none", out=out, act=act)
    _set_designed(g, fmt, tile)
    got = _run_out(g)
    assert_same_output(got, host_codec(target, out, act), out, (fmt, tile, out, act))
    goo.assert_designed_cases_present(got, target, out, act)
