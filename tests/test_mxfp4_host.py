"""MXFP4 on the host (no GPU): the e2m1 codec and the nibble packing, the OCP
MX rule of to_mxfp4 against a slow per-block transcription, the fp4x2 arrays,
the library entry, the GemmMxFp4 op object and its references, and the host
twin of the GPU tier's scale-mapping probe."""
import math

import numpy as np
import pytest

import cekirdekler_amd as ck
import gemm4_oracles as g4
from cekirdekler_amd.ops.gemm import (MXFP4_TILE_WAVES, MXFP4_TILES, MXFP8_TILES, GemmMxFp4, GemmMxFp8, decode_operand,
                                      e8m0_to_f64, from_fp4_e2m1_codes, from_mxfp4, pack_fp4, pack_mx_scales,
                                      rows_to_tile, tile_coords, to_fp4_e2m1_codes, to_mxfp4, unpack_fp4,
                                      unpack_mx_scales)

E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


# ------------------------------------------------------------------- codec


def test_all_16_codes_round_trip():
    codes = np.arange(16, dtype=np.uint8)
    v = from_fp4_e2m1_codes(codes)
    assert v.dtype == np.float32
    np.testing.assert_array_equal(v[:8], E2M1)
    np.testing.assert_array_equal(v[8:], [-x for x in E2M1])
    assert np.signbit(v[8]) and v[8] == 0  # -0 kept
    back = to_fp4_e2m1_codes(v)
    assert back.dtype == np.uint8
    np.testing.assert_array_equal(back, codes)
    # bit layout s e e m: value = (-1)^s · (e ? (1 + m/2) · 2^(e-1) : m/2)
    for c in range(16):
        s, e, m = c >> 3, (c >> 1) & 3, c & 1
        want = (m / 2 if e == 0 else (1 + m / 2) * 2.0 ** (e - 1)) * (-1) ** s
        assert float(v[c]) == want
    with pytest.raises(ValueError):
        from_fp4_e2m1_codes(np.array([16], np.uint8))


def test_rounds_to_nearest_even_at_every_midpoint():
    mids = {0.25: 0.0, 0.75: 1.0, 1.25: 1.0, 1.75: 2.0, 2.5: 2.0, 3.5: 4.0, 5.0: 4.0}
    assert sorted(mids) == [(a + b) / 2 for a, b in zip(E2M1, E2M1[1:])]  # every midpoint
    for dtype in (np.float32, np.float64):
        for x, want in mids.items():
            for sign in (1.0, -1.0):
                got = from_fp4_e2m1_codes(to_fp4_e2m1_codes(np.array([sign * x], dtype)))
                assert float(got[0]) == sign * want, (x, sign, got)
            # just off the midpoint: to the nearer neighbour
            lo, hi = max(v for v in E2M1 if v < x), min(v for v in E2M1 if v > x)
            below, above = np.nextafter(dtype(x), dtype(0)), np.nextafter(dtype(x), dtype(10))
            assert float(from_fp4_e2m1_codes(to_fp4_e2m1_codes(np.array([below], dtype)))[0]) == lo
            assert float(from_fp4_e2m1_codes(to_fp4_e2m1_codes(np.array([above], dtype)))[0]) == hi


def test_nearest_value_on_a_fine_grid():
    x = np.linspace(-7, 7, 28001).astype(np.float32)
    got = from_fp4_e2m1_codes(to_fp4_e2m1_codes(x)).astype(np.float64)
    grid = np.array(sorted(set(E2M1) | {-v for v in E2M1}))
    nearest = np.abs(x.astype(np.float64)[:, None] - grid[None, :]).min(axis=1)
    np.testing.assert_array_equal(np.abs(got - x), nearest)
    assert (np.sign(got) * np.sign(x) >= 0).all()


def test_saturation_and_nan():
    x = np.array([6.0, 6.5, 7.99, 8.0, 1e30, np.inf, -6.5, -1e30, -np.inf], np.float32)
    np.testing.assert_array_equal(from_fp4_e2m1_codes(to_fp4_e2m1_codes(x)), [6, 6, 6, 6, 6, 6, -6, -6, -6])
    np.testing.assert_array_equal(to_fp4_e2m1_codes(np.array([np.nan, -np.nan], np.float32)), [0, 0])
    assert to_fp4_e2m1_codes(np.array([-0.0, -0.1], np.float32)).tolist() == [8, 8]


def test_pack_unpack_and_nibble_order():
    rng = np.random.default_rng(0)
    codes = rng.integers(0, 16, (5, 7, 64)).astype(np.uint8)
    p = pack_fp4(codes)
    assert p.dtype == np.uint8 and p.shape == (5, 7, 32)
    np.testing.assert_array_equal(unpack_fp4(p), codes)
    np.testing.assert_array_equal(pack_fp4(unpack_fp4(p)), p)
    # element 2i in bits 0-3 of byte i, element 2i + 1 in bits 4-7
    assert pack_fp4(np.array([0x3, 0xA, 0xF, 0x0], np.uint8)).tolist() == [0xA3, 0x0F]
    assert unpack_fp4(np.array([0x21], np.uint8)).tolist() == [1, 2]
    every = np.arange(256, dtype=np.uint8)
    np.testing.assert_array_equal(pack_fp4(unpack_fp4(every)), every)
    with pytest.raises(ValueError):
        pack_fp4(np.zeros(3, np.uint8))
    with pytest.raises(ValueError):
        pack_fp4(np.array([16, 0], np.uint8))


# ------------------------------------------------------------------- to_mxfp4


def _slow_e2m1(v):
    """One float → code: the nearest of the 8 magnitudes, ties to the even
    code, saturating; NaN → 0."""
    if math.isnan(v):
        return 0
    s = 8 if math.copysign(1.0, v) < 0 else 0
    a = abs(v)
    if a >= 6:
        return s | 7
    best = min(range(8), key=lambda c: (abs(E2M1[c] - a), c & 1))
    return s | best


def _slow_mxfp4(x):
    """The rule of the issue, block by block in Python floats (float32 input
    is exact in them, and so is the scaling by a power of two)."""
    rows, K = x.shape
    codes = np.zeros((rows, K), np.uint8)
    scales = np.zeros((rows, K // 32), np.uint8)
    for r in range(rows):
        for blk in range(K // 32):
            vals = [float(v) for v in x[r, 32 * blk:32 * blk + 32]]
            finite = [abs(v) for v in vals if math.isfinite(v) and v != 0]
            e = 0
            if finite:
                e = math.frexp(max(finite))[1] - 1 - 2
                e = max(-127, min(127, e))
            scales[r, blk] = 0xFF if any(math.isnan(v) for v in vals) else e + 127
            for i, v in enumerate(vals):
                if math.isinf(v):
                    codes[r, 32 * blk + i] = 15 if v < 0 else 7
                else:
                    codes[r, 32 * blk + i] = _slow_e2m1(math.ldexp(v, -e))
    return codes, scales


def _mx_data():
    """float32 [48][128] reaching: the lower clamp of the scale (fp32
    subnormals), all-zero blocks, ±inf, a NaN block, a block of nothing but
    inf, scaled maxima in (6, 8), exact midpoints and plain random blocks."""
    rng = np.random.default_rng(7)
    x = (rng.uniform(-1, 1, (48, 4, 32)) * np.ldexp(1.0, rng.integers(-40, 41, (48, 4, 1)))).astype(np.float32)
    x[0, 0] = 0.0
    x[0, 1, 3] = -0.0
    x[0, 1, :3] = 0.0
    # e = floor(log2(6 · 2^-128)) - 2 = -128 clamps to -127: the elements are v/2, v in {0, 1, 2, 3, 4, 6}
    x[1, 0] = np.float32(2.0 ** -128) * rng.choice([0, 1, 2, 3, 4, 6, -1, -2, -3, -4, -6], 32)
    x[1, 0, 0] = np.float32(2.0 ** -128) * 6
    x[1, 1] = np.float32(2.0 ** -126) * rng.uniform(-1, 1, 32)
    x[2, 0, 5], x[2, 0, 6] = np.inf, -np.inf
    x[2, 1] = np.inf
    x[3, 2, 9] = np.nan                                            # the NaN block
    x[3, 3, 0] = np.inf
    for r, top in enumerate((6.5, 7.0, 7.75, 7.99), start=4):       # scaled maxima in (6, 8)
        x[r, 0] = rng.uniform(-4, 4, 32)
        x[r, 0, r] = top * 2.0 ** (r - 5)
    x[8, 0] = np.tile([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 4.0], 4) * np.float32(2.0 ** 9)  # midpoints under e = 9
    x[9, 0] = -x[8, 0]
    return x.reshape(48, 128)


def test_to_mxfp4_matches_the_slow_transcription():
    x = _mx_data()
    packed, scales = to_mxfp4(x)
    assert packed.dtype == np.uint8 and scales.dtype == np.uint8
    assert packed.shape == (48, 64) and scales.shape == (48, 4)
    want_codes, want_scales = _slow_mxfp4(x)
    np.testing.assert_array_equal(scales, want_scales)
    np.testing.assert_array_equal(unpack_fp4(packed), want_codes)
    # what the data reaches
    assert scales[1, 0] == 0 and scales[0, 0] == 127 and scales[2, 1] == 127
    assert (scales == 0xFF).sum() == 1 and scales[3, 2] == 0xFF
    codes = unpack_fp4(packed)
    assert (codes[0, :32] == 0).all() and codes[0, 35] == 8
    assert codes[2, 5] == 7 and codes[2, 6] == 15 and (codes[2, 32:64] == 7).all()
    assert codes[3, 64 + 9] == 0  # the NaN element's code
    assert all((codes[r, :32] & 7).max() == 7 for r in range(4, 8))  # (6, 8) saturates to 6
    dq = from_mxfp4(packed, scales)
    assert dq.dtype == np.float32 and dq.shape == x.shape
    nan = np.isnan(dq)
    assert nan[3, 64:96].all() and nan.sum() == 32  # the whole block, and only that block
    np.testing.assert_array_equal(dq[1, :32], x[1, :32])  # subnormals under the clamped scale: exact
    assert dq[2, 5] == 6 * 2.0 ** (int(scales[2, 0]) - 127)
    # the upper clamp is reachable from float64 input only
    big = np.full((1, 32), 2.0 ** 200, np.float64)
    p, s = to_mxfp4(big)
    assert s[0, 0] == 254 and (unpack_fp4(p) == 7).all()
    p, s = to_mxfp4(np.full((1, 32), 2.0 ** 129, np.float64))
    assert s[0, 0] == 254 and (unpack_fp4(p) == 6).all()  # e = 127 exactly: 2^129 · 2^-127 = 4
    with pytest.raises(ValueError):
        to_mxfp4(np.zeros((2, 48), np.float32))


def test_to_mxfp4_is_idempotent_through_from_mxfp4():
    x = _mx_data()
    x = x[~np.isnan(x).any(axis=1)]  # a NaN block comes back all NaN: nothing to repeat
    p1, s1 = to_mxfp4(x)
    dq = from_mxfp4(p1, s1)
    p2, s2 = to_mxfp4(dq)
    np.testing.assert_array_equal(from_mxfp4(p2, s2).view(np.uint32), dq.view(np.uint32))
    # where a block's maximum survives in e2m1's top binade the bits repeat too
    top = (unpack_fp4(p1).reshape(-1, 4, 32) & 7).max(axis=-1) >= 6
    np.testing.assert_array_equal(s2[top], s1[top])
    np.testing.assert_array_equal(p2.reshape(-1, 4, 16)[top], p1.reshape(-1, 4, 16)[top])
    assert top.mean() > 0.5
    rng = np.random.default_rng(9)
    y = (rng.standard_normal((64, 256)) * np.ldexp(1.0, rng.integers(-20, 21, (64, 1)))).astype(np.float32)
    p1, s1 = to_mxfp4(y)
    dq = from_mxfp4(p1, s1)
    np.testing.assert_array_equal(from_mxfp4(*to_mxfp4(dq)), dq)
    # |y - dq| <= max(|y| / 4, X / 4): half a step of 1 mantissa bit, the saturation of (6, 8), the subnormal step
    X = np.repeat(e8m0_to_f64(s1), 32, axis=-1)
    assert (np.abs(y - dq.astype(np.float64)) <= np.maximum(np.abs(y.astype(np.float64)) / 4, X / 4)).all()


# ------------------------------------------------------------------- arrays


def test_fp4_clarray_flags_and_decode_operand():
    for name in ("float4_e2m1fn_x2", "fp4x2", "e2m1x2", "FP4X2"):
        a = ck.ClArray(48, name)
        assert a.is_fp4 and not a.is_fp8 and not a.is_bf16 and a.N == 48 and a.array.dtype == np.uint8
        assert a.dtype_name == "float4_e2m1fn_x2"
    plain = ck.ClArray(48, name, fast=False)
    assert plain.is_fp4 and plain.N == 48 and not plain.fast_arr
    assert not ck.ClArray(8, "fp8").is_fp4 and not ck.ClArray(8, np.uint8).is_fp4 and ck.ClArray(8, "fp8").is_fp8
    f = ck.ClFp4x2Array(16)
    assert f.is_fp4 and not f.is_fp8 and f.array.dtype == np.uint8 and len(f) == 16
    assert ck.ClArray(f).is_fp4 and ck.ClArray(ck.ClArray(f)).is_fp4
    wrapped = ck.ClArray(np.arange(6, dtype=np.uint8), "fp4x2")
    assert wrapped.is_fp4 and wrapped.N == 6
    # the flag survives a storage switch and a resize
    wrapped.fast_arr = True
    assert wrapped.is_fp4 and wrapped.fast_arr and wrapped.array.tolist() == [0, 1, 2, 3, 4, 5]
    wrapped.N = 10
    assert wrapped.is_fp4 and wrapped.N == 10
    # decode_operand: two elements per byte, low nibble first
    a = ck.ClArray(np.array([0x21, 0xF7, 0x08], np.uint8), "fp4x2")
    np.testing.assert_array_equal(decode_operand(a), [0.5, 1.0, 6.0, -6.0, -0.0, 0.0])
    assert np.signbit(decode_operand(a)[4])
    # torch round trip: the packed dtype where torch has it, plain bytes otherwise
    import torch

    t = a.as_torch()
    t4 = getattr(torch, "float4_e2m1fn_x2", None)
    assert t.dtype == (t4 if t4 is not None else torch.uint8)
    back = ck.ClArray(t)
    assert back.is_fp4 == (t4 is not None) and back.array.tolist() == a.array.tolist()
    if t4 is not None:
        assert ck.ClArray(4, t4).is_fp4


# ------------------------------------------------------------------ library


def test_mxfp4_library_entry():
    from cekirdekler_amd.ops.library import ARITY, LIBRARY, code_object

    names = ["cek_sgemm_mxfp4_128x128", "cek_sgemm_mxfp4_256x256pbx"]
    assert sorted(LIBRARY["sgemm_mxfp4"]) == names == sorted(v[3] for v in MXFP4_TILES.values())
    assert all(ARITY[k] == 6 for k in names)
    assert sorted(MXFP4_TILE_WAVES) == sorted(MXFP4_TILES) and MXFP4_TILE_WAVES == {k: (2, 4, 8, 4) if k != "128x128"
                                                                                  else (2, 2, 4, 4) for k in MXFP4_TILES}
    blob = open(code_object("sgemm_mxfp4"), "rb").read()
    for k in names:
        assert k.encode() + b"\0" in blob, k
    assert sorted(LIBRARY["sgemm_mxfp8"]) == sorted(v[3] for v in MXFP8_TILES.values())  # as it was


# --------------------------------------------------------------- op objects


@pytest.fixture(scope="module")
def cpu_cr():
    cr = ck.ClNumberCruncher(ck.ClPlatforms.all().cpus(True), "__global__ void nop(float* x) {}")
    yield cr
    cr.dispose()


@pytest.mark.parametrize("tile", sorted(MXFP4_TILES))
def test_mxfp4_objects(cpu_cr, tile):
    M, N, K = 512, 256, 512
    g = GemmMxFp4(M, N, K, cruncher=cpu_cr, tile=tile)
    assert g.global_range == g.tiles * g.L and g.split_k == 1 and not g.exchange and not g.row_major_c
    assert g.A.is_fp4 and g.B.is_fp4 and g.A.N == M * K // 2 and g.B.N == N * K // 2
    assert g.SA.array.dtype == np.uint8 and g.SA.N == M * K // 32 and g.SB.N == N * K // 32
    assert g._SAp.N == M * K // 128 and g._SBp.N == N * K // 128
    assert g.kernel == MXFP4_TILES[tile][3] and g.C.elements_per_work_item * g.L == g.BM * g.BN
    assert GemmMxFp4.__init__.__defaults__[1] == "256x256pbx"
    assert g.flops == 2.0 * M * N * K  # K in elements
    for call in (lambda: g.run_shells(2), lambda: g.run_host_shells(2), lambda: g.verify_shells(2),
                 lambda: g.verify_shells_full(2)):
        with pytest.raises(NotImplementedError, match="GemmMxFp4"):
            call()
    with pytest.raises(NotImplementedError, match="separate, later change"):
        g.quantize("A", np.zeros((M, K), np.float32))
    # the default data is the MXFP8 draw through to_mxfp4: block factors 2^-12 .. 2^12
    sa = g.SA.array.astype(np.int64) - 127
    assert sa.min() < -12 and sa.max() > 5 and len(np.unique(sa)) > 20 and (g.SA.array != 0xFF).all()
    a = from_mxfp4(g.A.array.reshape(M, K // 2), g.SA.array.reshape(M, K // 32)).astype(np.float64)
    b = from_mxfp4(g.B.array.reshape(N, K // 2), g.SB.array.reshape(N, K // 32)).astype(np.float64)
    assert 2.0 ** 11 < np.abs(a).max() <= 2.0 ** 12
    np.testing.assert_array_equal(g._operand("A"), a)
    np.testing.assert_array_equal(g.reference(), a @ b.T)
    np.testing.assert_array_equal(g.reference(slice(3, 9)), (a @ b.T)[3:9])
    np.testing.assert_array_equal(g._operand_t("B", "cpu").numpy(), b)
    # the same seed draws the same numbers as GemmMxFp8
    rng = np.random.default_rng(0)
    x = np.ldexp(rng.uniform(-1, 1, (M, K // 32, 32)), rng.integers(-12, 13, (M, K // 32, 1))).astype(np.float32)
    np.testing.assert_array_equal(to_mxfp4(x.reshape(M, K))[0].ravel(), g.A.array)


@pytest.mark.parametrize("tile", sorted(MXFP4_TILES))
def test_constructor_refusals(cpu_cr, tile):
    BM, BN = MXFP4_TILES[tile][:2]
    for shape in ((BM, BN, 128), (BM, BN, 384), (BM, BN, 0), (BM + 64, BN, 256), (BM, BN - 16, 256), (0, BN, 256),
                  (BM, -BN, 256), (BM, BN, -256)):
        with pytest.raises(ValueError):
            GemmMxFp4(*shape, cruncher=cpu_cr, tile=tile)
    GemmMxFp4(BM, BN, 256, cruncher=cpu_cr, tile=tile, fill="none")
    with pytest.raises(KeyError):
        GemmMxFp4(256, 256, 256, cruncher=cpu_cr, tile="256x256pb")


def test_rows_are_counted_in_bytes(cpu_cr):
    """can_stream and the streamed A panel count K/2 bytes per row; the MXFP8
    object of the same shape counts K (the hook's default)."""
    M, N, K = 1024, 512, 512
    g = GemmMxFp4(M, N, K, cruncher=cpu_cr, fill="none", group_m=1)
    g8 = GemmMxFp8(M, N, K, cruncher=cpu_cr, fill="none", group_m=1)
    assert g._row_items() == K // 2 and g8._row_items() == K
    assert g.can_stream() and g8.can_stream()
    # a panel of BM rows is BM·K/2 bytes: with N/BN·L = 1024 work items per tile row, 64 bytes each
    assert (g.BM * g._row_items()) // ((N // g.BN) * g.L) == 64
    # K/2 bytes per row do not divide among the work items of this many tile columns, K bytes do
    wide = GemmMxFp4(256, 256 * 3, 256, cruncher=cpu_cr, fill="none", group_m=1)
    assert not wide.can_stream()


def _plant(g, ref):
    tm, tn = tile_coords(np.arange(g.tiles), g.M, g.N, g.BM, g.BN, g.group_m)
    tiles = np.stack([ref[r * g.BM:(r + 1) * g.BM, c * g.BN:(c + 1) * g.BN].astype(np.float32)
                      for r, c in zip(tm, tn)])
    g.C.array[:] = rows_to_tile(tiles, g.geom).ravel()


@pytest.mark.parametrize("tile", sorted(MXFP4_TILES))
def test_mxfp4_result_and_verify_full_include_the_scales(tile):
    """C planted as the fragment-ordered exact product (gemm4_oracles.int_case:
    exact in fp32): result() returns it, verify_full and verify are 0, and one
    perturbed element is found."""
    cpu = ck.ClPlatforms.all().cpus(True)
    cr = ck.ClNumberCruncher(cpu + cpu, "__global__ void nop(float* x) {}")
    shape = (512, 768, 256)
    a, b, ea, eb, ref = g4.int_case(shape)
    g = GemmMxFp4(*shape, cruncher=cr, tile=tile, fill="none")
    g4.set_operands(g, a, b, ea, eb)
    np.testing.assert_array_equal(g.reference(), ref)
    unit = a.astype(np.float64) @ b.astype(np.float64).T
    assert (ref != unit).mean() > 0.5  # the scales are in the reference
    half = g.tiles // 2 * g.L
    cr.cores.set_state(1, [half, g.tiles * g.L - half], [[0.0, 0.0] for _ in range(10)], [1.0, 1.0])
    _plant(g, ref)
    np.testing.assert_array_equal(g.result(download=False).astype(np.float64), ref)
    err, checked = g.verify_full(1, host=True, device="cpu")
    assert checked == g.tiles and err == 0.0, (err, checked)
    assert g.verify(1, host=True) == 0.0
    g.C.array[g.C.N - 7] += 0.5 * float(np.abs(ref).max())  # one element of the last tile
    err, _ = g.verify_full(1, host=True, device="cpu")
    assert err > 1e-4
    cr.dispose()


def test_packed_scales_follow_the_public_ones(cpu_cr):
    """pack_mx_scales unchanged, a K-tile of 256 k being two of its 128-k
    steps: K = 512 gives [4][M/64][64] dwords."""
    g = GemmMxFp4(256, 256, 512, cruncher=cpu_cr, tile="128x128")
    for upload in (True, True):
        g.SA.array[:] = np.arange(g.SA.N) % 251
        arrays = g._inputs(upload)
        assert len(arrays) == 5 and len(g._params()) == 5 and g._params()[-1] is g.C
        np.testing.assert_array_equal(unpack_mx_scales(arrays[3].array.reshape(4, 4, 64)), g.SA.array.reshape(256, 16))
        np.testing.assert_array_equal(unpack_mx_scales(arrays[4].array.reshape(4, 4, 64)), g.SB.array.reshape(256, 16))
        np.testing.assert_array_equal(arrays[3].array.reshape(4, 4, 64), pack_mx_scales(g.SA.array.reshape(256, 16)))


# ------------------------------------------------- the scale-mapping probe


@pytest.mark.parametrize("coeff", g4.PROBE_SA_BLOCK_COEFF + sorted(g4.PROBE_BLIND_COEFF))
def test_scale_mapping_probe_distinguishes_on_the_host(coeff):
    """The probe's expected C against what wrong maps would give, on the CPU
    (gemm4_oracles.probe_expected_and_wrong lists them: the MXFP8 probe's and
    those particular to fp4 — swapped nibbles, exchanged 128-k steps).  Under
    the coefficients the GPU tier runs every one of them differs from the
    expected C in more than half the elements; c = 5 and c = 3 are shown to
    have the blind spots gemm4_oracles.PROBE_BLIND_COEFF names, and are not run."""
    want, wrong = g4.probe_expected_and_wrong(coeff)
    assert len(wrong) == 11
    blind = g4.PROBE_BLIND_COEFF.get(coeff, ())
    assert (coeff in g4.PROBE_SA_BLOCK_COEFF) == (not blind)
    for name, c in wrong.items():
        frac = float((c != want).mean())
        if name in blind:
            assert frac < 0.5, (name, frac)
        else:
            assert frac > 0.5, (name, frac)


def test_single_instruction_probe_problems_are_well_formed():
    """The probe's buffers (no GPU): 30 problems, every expectation an fp32
    value, and the read-back helpers return the expected maps when fed the
    expected answers."""
    names, a, b, sa, sb, sel = g4.probe_buffers()
    n = len(names)
    assert a.shape == b.shape == (n * 1024,) and sa.shape == sb.shape == (n * 256,) and sel.shape == (n,)
    assert set(g4.PROBE_IEEE) < set(names) and sel.min() >= 0 and sel.max() < 16
    answers = {k: np.where(p["want"][0] == 0, p["want"][1], np.nan).astype(np.float32)
               for k, p in g4.probe_problems().items()}
    for operand in "ab":
        np.testing.assert_array_equal(g4.measured_k_map(answers, operand), np.arange(128))
        for o in range(4):
            row, block, want_block = g4.measured_scale_map(answers, operand, o)
            np.testing.assert_array_equal(row, np.arange(16))
            np.testing.assert_array_equal(block, want_block)
            assert sorted(set(want_block.tolist())) == [0, 1, 2, 3]
