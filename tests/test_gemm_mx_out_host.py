"""CPU tier of the MX GEMMs' output modes (kernels/sgemm_mx_out.hip,
GemmMxFp8 / GemmMxFp4 with ``out=`` and ``act=``): the executable model of
the epilogue against the float64 codecs on designed rows, the constructor
matrix (kernel, arity, arrays, flags, refusals, take_operand's checks), the
unchanged ``out=None`` objects, and the contiguity of a device's slice of Y
and SY under a split in whole tile groups.  Every comparison is exact."""
import numpy as np
import pytest

import cekirdekler_amd as ck
from cekirdekler_amd.ops.gemm import (MX_OUT_KERNELS, MX_OUTPUTS, MXFP4_TILES, MXFP8_TILES, GemmFp8, GemmMxFp4,
                                      GemmMxFp8, pack_mx_scales, tile_coords, to_bf16_bits, to_mxfp4, to_mxfp8)
from cekirdekler_amd.cruncher import ClComputeError
from cekirdekler_amd.ops.library import ARITY, LIBRARY
from cekirdekler_amd.ops.quantize import gemm_out_model, mxfp4_reference, mxfp8_reference, relu_model

FORMATS = {"mxfp8": GemmMxFp8, "mxfp4": GemmMxFp4}
TILES = ("256x256pbx", "128x128")
ACTS = (None, "relu")


def relu(c):
    """ReLU as the issue defines it: x > 0 → x, NaN → NaN, everything else → +0."""
    c = np.asarray(c, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(c > 0, c, np.where(np.isnan(c), c, np.float32(0))).astype(np.float32)


def host_codec(c, out, act=None):
    """What an output-mode kernel must store for the fp32 ``[M][N]`` values
    ``c`` of the plain kernel, through the float64 host codecs: ``(Y, SY,
    packed)``; bf16 has no SY and no packed array."""
    c = np.ascontiguousarray(c, np.float32)
    if act == "relu":
        c = relu(c)
    with np.errstate(invalid="ignore", over="ignore"):
        if out == "bfloat16":
            return to_bf16_bits(c).reshape(c.shape), None, None
        codes, scales = (mxfp8_reference if out == "mxfp8" else mxfp4_reference)(c)
    return codes, scales, pack_mx_scales(scales)


def bf16_is_nan(b):
    return (np.asarray(b, np.uint16) & 0x7FFF) > 0x7F80


def assert_same_output(got, want, out, what=""):
    """(Y, SY, packed) bit for bit; bf16: NaN-ness compared as such, every other value by its bits."""
    for name, g, w in zip(("Y", "SY", "packed"), got, want):
        if w is None:
            assert g is None, (what, name)
            continue
        g, w = np.asarray(g).ravel(), np.asarray(w).ravel()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        if out == "bfloat16":
            gn, wn = bf16_is_nan(g), bf16_is_nan(w)
            bad = np.flatnonzero((gn != wn) | (~wn & (g != w)))
        else:
            bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, name, len(bad), bad[:4].tolist(), [hex(int(v)) for v in g[bad[:4]]],
                               [hex(int(v)) for v in w[bad[:4]]])


# ----------------------------------------------------------------- 1: the model


def designed_rows():
    """fp32 [64][128] (so that the scales pack): per 32-column block one
    designed case, the rest seeded wide-range values.
    Rows 0-7 e4m3 ties and values around them under a block maximum of 256·…;
    rows 8-15 the same for e2m1; 16-23 values that round past 448 / past 6;
    24-31 results in the formats' subnormal ranges; 32-39 all-zero blocks of
    both signs; 40-47 ±Inf; 48-55 NaN of both signs and payloads; 56-63 −0
    among negatives and denormals."""
    rng = np.random.default_rng(2026)
    x = np.ldexp(rng.uniform(-1, 1, (64, 4, 32)), rng.integers(-20, 21, (64, 4, 1))).astype(np.float32)
    f = np.float32
    # e4m3 ties: maximum 256 (scale 2^0 after the −8), neighbours at 3-bit mantissa ties ± 1 ulp
    ties8 = np.array([1.0625, 1.1875, 17.0, 19.0, 0.0009765625 * 1.5, 2.0 ** -10, 2.0 ** -9 * 0.5, 3.25], f)
    for r in range(8):
        x[r, :, 0] = 256.0
        for k, t in enumerate(ties8):
            for s, ulp in enumerate((0, 1, -1)):
                x[r, :, 1 + 3 * k + s] = (np.array([t], f).view(np.int32) + np.int32(ulp)).view(f) * f((-1) ** r)
    # e2m1 ties: maximum 4 (scale 2^0), ties 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5
    ties4 = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 0.125], f)
    for r in range(8, 16):
        x[r, :, 0] = 4.0
        for k, t in enumerate(ties4):
            for s, ulp in enumerate((0, 1, -1)):
                x[r, :, 1 + 3 * k + s] = (np.array([t], f).view(np.int32) + np.int32(ulp)).view(f) * f((-1) ** r)
        x[r, :, 25:] = 0.0
    # past 448 and past 6: the block maximum 1.9999·2^r becomes 511.9 under the e4m3 scale and 7.99 under
    # the e2m1 one, both beyond the largest value plus half a step
    for r in range(16, 24):
        x[r] = np.ldexp(rng.uniform(-1, 1, (4, 32)), r - 20).astype(f)
        x[r, :, 0] = np.ldexp(f(1.9999), r)
        x[r, :, 1] = -np.ldexp(f(1.87), r)  # e4m3: 478.7 rounds to 480 > 448
        x[r, :, 2] = np.ldexp(f(1.76), r)   # e4m3: 450.6 rounds to 448
    # subnormal results: tiny beside a large maximum, and fp32 denormals alone
    for r in range(24, 32):
        x[r, :2] = np.ldexp(rng.uniform(-1, 1, (2, 32)), -16 - r).astype(f)
        x[r, :2, 0] = 1.0
        x[r, 2:] = (rng.integers(1, 1 << 23, (2, 32)).astype(np.uint32)).view(f)
    x[32:36] = 0.0
    x[36:40] = -0.0
    x[38, :, 5] = 0.0
    for r in range(40, 48):
        x[r, :, r - 40] = np.inf if r & 1 else -np.inf
    x[46] = np.inf
    x[47, :, :] = -np.inf
    nan_bits = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF], np.uint32)
    for r in range(48, 56):
        x[r, :, (3 * r) % 32] = nan_bits[r % 6].view(f)
    x.reshape(64, 128)[54] = nan_bits[2].view(f)
    x[55, 1] = nan_bits[1].view(f)
    for r in range(56, 64):
        x[r] = -np.abs(x[r])
        x[r, :, 3] = -0.0
        x[r, :, 4] = np.uint32(0x80000001).view(f)
        x[r, :, 5] = np.uint32(0x00000001).view(f)
    return x.reshape(64, 128)


def test_designed_rows_hold_what_they_claim():
    x = designed_rows()
    with np.errstate(invalid="ignore"):  # signalling NaN patterns in a float64 cast
        c8, s8 = to_mxfp8(x)
        c4, s4 = to_mxfp4(x)
    assert ((c8[16:24] & 0x7F) == 0x7E).sum() >= 16 and (s8[32:40] == 127).all() and (c8[36:38] == 0x80).all()
    assert ((c8[24:32] & 0x78) == 0).sum() > 100  # e4m3 subnormal or zero codes
    assert (c8[48:56] == 0x7F).sum() >= 32 and (s4[54] == 0xFF).all() and (s4[48:56] == 0xFF).sum() >= 32
    assert np.isinf(x[40:48]).sum() >= 32 and (c8[46] == 0x7E).all() and (c8[47] == 0xFE).all()
    assert (np.signbit(x[56:]) | (x[56:] > 0)).all()
    assert (relu(x[56:]).view(np.uint32)[:, [3, 4]] == 0).all() and (relu(x[56:])[:, 5] > 0).all()


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("out", MX_OUTPUTS)
def test_model_equals_the_host_codecs(out, act):
    """gemm_out_model (integer ReLU, integer bf16 rounding, the quantise
    kernels' models) against the float64 codecs behind a numpy ReLU."""
    x = designed_rows()
    got = gemm_out_model(x, out, act)
    c = relu(x) if act else x
    if out == "bfloat16":
        want = (to_bf16_bits(c).reshape(c.shape), None, None)
    else:
        with np.errstate(invalid="ignore"):
            codes, scales = (to_mxfp8 if out == "mxfp8" else to_mxfp4)(c)
        want = (codes, scales, pack_mx_scales(scales))
    assert_same_output(got, want, out, (out, act))
    assert_same_output(host_codec(x, out, act), want, out)
    if out == "bfloat16":  # a NaN stays a NaN, nothing else becomes one
        np.testing.assert_array_equal(bf16_is_nan(got[0]), np.isnan(c))


def test_relu_of_the_specials():
    f = np.float32
    x = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 1e-45, -1e-45], f)
    np.testing.assert_array_equal(relu_model(x).view(np.uint32),
                                  np.array([0, 0, 1.0, 0, np.inf, 0, 1e-45, 0], f).view(np.uint32))
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001], np.uint32)
    np.testing.assert_array_equal(relu_model(nans.view(f)).view(np.uint32), nans)  # NaN → NaN, sign and payload kept
    np.testing.assert_array_equal(relu_model(x).view(np.uint32), relu(x).view(np.uint32))
    with pytest.raises(ValueError):
        gemm_out_model(np.zeros((64, 128), f), "mxfp8", "gelu")
    with pytest.raises(ValueError):
        gemm_out_model(np.zeros((64, 128), f), "float16")


# ------------------------------------------------------------ 2: constructor matrix


@pytest.fixture(scope="module")
def cpu_cr():
    cr = ck.ClNumberCruncher(ck.ClPlatforms.all().cpus(True), "__global__ void nop(float* x) {}")
    yield cr
    cr.dispose()


@pytest.fixture(scope="module")
def cpu_cr2():
    cpu = ck.ClPlatforms.all().cpus(True)
    cr = ck.ClNumberCruncher(cpu + cpu, "__global__ void nop(float* x) {}")
    assert cr.number_of_devices == 2
    yield cr
    cr.dispose()


def test_tables():
    assert set(MX_OUT_KERNELS) == {(f, t, o) for f, tiles in (("mxfp8", MXFP8_TILES), ("mxfp4", MXFP4_TILES))
                                   for t in tiles for o in MX_OUTPUTS}
    assert sorted(MX_OUT_KERNELS.values()) == sorted(LIBRARY["sgemm_mx_out"]) and len(LIBRARY["sgemm_mx_out"]) == 12
    for lib in ("sgemm_mxfp8", "sgemm_mxfp4"):  # the plain tables took no new names
        assert len(LIBRARY[lib]) == 2 and not set(LIBRARY[lib]) & set(LIBRARY["sgemm_mx_out"])


@pytest.mark.parametrize("out", MX_OUTPUTS)
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_constructor_matrix(cpu_cr, fmt, tile, out):
    cls = FORMATS[fmt]
    BM, BN, L, plain = cls.TILE_TABLE[tile]
    M, N, K = 3 * BM, 2 * BN, 256
    g = cls(M, N, K, cruncher=cpu_cr, tile=tile, fill="none", group_m=2, out=out, act="relu")
    assert g.kernel == plain + "_" + ("bf16" if out == "bfloat16" else out) == MX_OUT_KERNELS[fmt, tile, out]
    assert g.kernel in LIBRARY["sgemm_mx_out"] and "sgemm_mx_out" in g.LIBS and g.LIBS[:-1] == cls.LIBS
    assert len(g._params()) + 1 == ARITY[g.kernel] == (6 if out == "bfloat16" else 7)
    assert g.dims.array.tolist() == [M, N, K, 2, 1, 1, 0, 0]  # dims[5]: ReLU
    assert g.C is None and g.global_range == g.tiles * L
    n = M * N
    if out == "bfloat16":
        assert g.Y.is_bf16 and g.Y.N == n and g.SY is None and g.Yp is None
    elif out == "mxfp8":
        assert g.Y.is_fp8 and g.Y.N == n
    else:
        assert g.Y.is_fp4 and g.Y.N == n // 2
    outs = [g.Y] if out == "bfloat16" else [g.Y, g.SY]
    assert g._params()[:4] == (g.A, g.B, g._SAp, g._SBp) and list(g._params()[4:]) == outs
    if out != "bfloat16":
        assert g.SY.N == n // 32 and g.SY.array.dtype == np.uint8
        assert g.Yp.N == n // 128 and g.Yp.array.dtype == np.uint32
        assert g.SY.elements_per_work_item * L == BM * BN // 32
    # a tile's share per work item: the whole range covers the array exactly
    assert g.Y.elements_per_work_item * L * g.Y.array.itemsize * (2 if out == "mxfp4" else 1) == (
        BM * BN * (2 if out == "bfloat16" else 1))
    for a in outs:
        assert a.read is False and a.elements_per_work_item * g.global_range == a.N
    for resident in (True, False):
        g._output_flags(resident)
        for a in outs:
            assert (a.read, a.write, a.partial_read, a.gather_resident) == (False, not resident, False, False)
    assert cls(M, N, K, cruncher=cpu_cr, tile=tile, fill="none", out=out).dims.array[5] == 0
    # refusals in an output mode
    with pytest.raises(ValueError, match="stream_blobs"):
        g.run(resident=False, stream_blobs=2)
    for shell in (g.run_shells, g.run_host_shells, g.verify_shells, g.verify_shells_full):
        with pytest.raises(ValueError, match="shell"):
            shell()
    with pytest.raises(ClComputeError, match="sgemm_mx_out"):
        g.run()  # this cruncher has no library kernels: a missing kernel is an error


def test_refused_arguments(cpu_cr, cpu_cr2):
    for cls in FORMATS.values():
        with pytest.raises(ValueError, match="act needs an output mode"):
            cls(256, 256, 256, cruncher=cpu_cr, fill="none", act="relu")
        with pytest.raises(ValueError, match="out must be"):
            cls(256, 256, 256, cruncher=cpu_cr, fill="none", out="float16")
        with pytest.raises(ValueError, match="act must be"):
            cls(256, 256, 256, cruncher=cpu_cr, fill="none", out="mxfp8", act="gelu")
        with pytest.raises(TypeError):
            GemmFp8(256, 256, 256, cruncher=cpu_cr, fill="none", out="mxfp8")
        # several devices: whole tile groups only
        with pytest.raises(ValueError, match="whole tile groups"):
            cls(768, 512, 256, cruncher=cpu_cr2, fill="none", group_m=2, out="mxfp8")
        g = cls(1024, 512, 256, cruncher=cpu_cr2, fill="none", group_m=2, out="mxfp8")
        assert g.granularity() == g._group_work_items() == 2 * 2 * 512
        g._output_flags(True)
        assert g.Y.gather_resident and g.SY.gather_resident and not g.Y.write
        # one device takes a ragged last group
        cls(768, 512, 256, cruncher=cpu_cr, fill="none", group_m=2, out="mxfp8")
        # without an output mode the split is as it was, ragged groups included
        plain = cls(768, 512, 256, cruncher=cpu_cr2, fill="none", group_m=2)
        assert plain.granularity() == plain.L


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_take_operand_checks(cpu_cr, cpu_cr2, fmt):
    cls, other = FORMATS[fmt], FORMATS["mxfp4" if fmt == "mxfp8" else "mxfp8"]
    prod = other(512, 512, 256, cruncher=cpu_cr, fill="none", out=fmt, act="relu")
    g = cls(512, 256, 512, cruncher=cpu_cr, fill="none")
    a_before = g.A
    with pytest.raises(ValueError, match="'A' or 'B'"):
        g.take_operand("C", prod)
    for bad_out in (None, "bfloat16", "mxfp4" if fmt == "mxfp8" else "mxfp8"):
        with pytest.raises(ValueError, match="format mismatch"):
            g.take_operand("A", other(512, 512, 256, cruncher=cpu_cr, fill="none", out=bad_out))
    with pytest.raises(ValueError, match="rows mismatch"):
        g.take_operand("A", other(256, 512, 256, cruncher=cpu_cr, fill="none", out=fmt))
    with pytest.raises(ValueError, match="rows mismatch"):
        g.take_operand("B", prod)  # B has N = 256 rows
    with pytest.raises(ValueError, match="K mismatch"):
        g.take_operand("A", other(512, 256, 256, cruncher=cpu_cr, fill="none", out=fmt))
    with pytest.raises(ValueError, match="cruncher mismatch"):
        g.take_operand("A", other(512, 512, 256, cruncher=cpu_cr2, fill="none", group_m=2, out=fmt))
    assert g.A is a_before and not g._stale
    g.take_operand("A", prod)
    assert g.A is prod.Y and g.SA is prod.SY and g._SAp is prod.Yp and g._stale == {"A"}
    assert g._params() == (g.A, g.B, g._SAp, g._SBp, g.C) and g.A.N == 512 * 512 // cls.PER_ITEM
    # resident: nothing of A goes up; a host-resident call is refused while the host arrays are behind
    assert g._inputs(True) == (g.dims, g.B, g._SBp)
    with pytest.raises(ValueError, match=r"sync_operands\(\)"):
        g.run(resident=False)
    gb = cls(256, 512, 512, cruncher=cpu_cr, fill="none")
    gb.take_operand("B", prod)
    assert gb.B is prod.Y and gb.SB is prod.SY and gb._SBp is prod.Yp and gb._stale == {"B"}


# -------------------------------------------------------- 3: out=None is unchanged


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_plain_objects_are_unchanged(cpu_cr, fmt, tile):
    cls = FORMATS[fmt]
    BM, BN, L, kname = cls.TILE_TABLE[tile]
    g = cls(2 * BM, 2 * BN, 256, cruncher=cpu_cr, tile=tile, fill="none")
    assert g.out is None and g.act is None and g.kernel == kname and kname in LIBRARY["sgemm_" + fmt]
    assert "LIBS" not in vars(g) and g.LIBS is cls.LIBS and "sgemm_mx_out" not in cls.LIBS
    assert GemmMxFp8.LIBS == ("sgemm_mxfp8", "mx_quantize")
    assert GemmMxFp4.LIBS == ("sgemm_mxfp4", "mx4_quantize", "mx_quantize")
    assert g._params() == (g.A, g.B, g._SAp, g._SBp, g.C) and len(g._params()) + 1 == ARITY[kname] == 6
    assert g.C.N == g.M * g.N and g.C.read is False and g.C.elements_per_work_item == BM * BN // L
    assert g.dims.array.tolist() == [g.M, g.N, 256, 4, 1, 0, 0, 0]
    assert not hasattr(g, "Y")
    g._output_flags(True)
    assert g.C.write is False
    g._output_flags(False)
    assert g.C.write is True
    with pytest.raises(NotImplementedError):
        g.run_shells()


# --------------------------------------------- 4: a device's slice under a split


@pytest.mark.parametrize("ranges", [(1, 3), (3, 1), (1, 2, 1), (2, 0, 2), (1, 1, 2)])
@pytest.mark.parametrize("out", MX_OUTPUTS)
@pytest.mark.parametrize("tile,group_m", [("256x256pbx", 1), ("256x256pbx", 2), ("128x128", 2)])
def test_slices_are_contiguous_row_blocks(cpu_cr, tile, group_m, out, ranges):
    """Ranges in whole tile groups (2 and 3 devices, uneven): the elements a
    device's tiles cover in the row-major Y and SY are exactly
    [reference · e, (reference + range) · e), e the array's
    elements_per_work_item, and the devices' slices tile the arrays."""
    BM, BN, L, _ = MXFP8_TILES[tile]
    groups = sum(ranges)
    M, N = groups * group_m * BM, 3 * BN
    g = GemmMxFp8(M, N, 256, cruncher=cpu_cr, tile=tile, fill="none", group_m=group_m, out=out)
    unit = g._group_work_items()
    assert unit * groups == g.global_range
    arrays = [(g.Y, g.Y.N // M)] + ([(g.SY, N // 32)] if g.SY is not None else [])
    for arr, pitch in arrays:  # pitch: storage items per row
        e = arr.elements_per_work_item
        covered = np.zeros(arr.N, np.int32)
        ref = 0
        for r in ranges:
            lo, n = ref * unit, r * unit
            tm, tn = tile_coords(np.arange(lo // L, (lo + n) // L), M, N, BM, BN, group_m)
            mine = np.zeros((M, pitch), bool)
            bw = BN * pitch // N
            for a, b in zip(np.asarray(tm).tolist(), np.asarray(tn).tolist()):
                assert not mine[a * BM:(a + 1) * BM, b * bw:(b + 1) * bw].any()
                mine[a * BM:(a + 1) * BM, b * bw:(b + 1) * bw] = True
            idx = np.flatnonzero(mine.ravel())
            want = np.arange(lo * e, (lo + n) * e)
            np.testing.assert_array_equal(idx, want)
            covered[idx] += 1
            ref += r
        assert (covered == 1).all()
