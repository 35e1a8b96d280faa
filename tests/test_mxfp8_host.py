"""MXFP8 on the host (no GPU): the OCP MX codec (exact round trips, the
derived error bound, edge cases), the packed scale layout of
kernels/sgemm_mxfp8.hip, the library entry and the GemmMxFp8 op object."""
import numpy as np
import pytest

import cekirdekler_amd as ck
from cekirdekler_amd.ops.gemm import (FP8_TILES, MXFP8_TILE_WAVES, MXFP8_TILES, GemmMxFp8, e8m0_to_f64,
                                      from_fp8_e4m3_bits, from_mxfp8, pack_mx_scales, rows_to_tile, tile_coords,
                                      to_fp8_e4m3_bits, to_mxfp8, unpack_mx_scales)

CODES = np.arange(256, dtype=np.uint8)
FINITE = CODES[(CODES & 0x7F) != 0x7F]  # the 254 non-NaN codes


# ------------------------------------------------------------------- codec


def test_exact_round_trip_and_scale_byte():
    """Blocks c · 2^e, c finite e4m3 values with at least one |c| >= 256 (so the
    block maximum lies in e4m3's top binade and the shared exponent is e):
    the scale byte is e + 127 and decoding gives x back bit for bit."""
    rng = np.random.default_rng(0)
    rows, nb = 64, 12
    codes = rng.choice(FINITE, (rows, nb, 32))
    top = CODES[(CODES & 0x7F) >= 0x78][:-1]  # |c| in 256 .. 448 (0x78 .. 0x7E), both signs
    top = top[(top & 0x7F) != 0x7F]
    assert np.abs(from_fp8_e4m3_bits(top)).min() == 256 and np.abs(from_fp8_e4m3_bits(top)).max() == 448
    codes[..., 0] = rng.choice(top, (rows, nb))
    codes = rng.permuted(codes, axis=-1)
    e = rng.integers(-100, 101, (rows, nb))
    e[0, :4] = [-100, 100, 0, -1]
    x64 = np.ldexp(from_fp8_e4m3_bits(codes).astype(np.float64), e[..., None])
    x = x64.astype(np.float32).reshape(rows, nb * 32)
    assert np.array_equal(x.astype(np.float64), x64.reshape(rows, -1))  # exact in fp32
    got_codes, scales = to_mxfp8(x)
    assert got_codes.dtype == np.uint8 and scales.dtype == np.uint8
    assert got_codes.shape == (rows, nb * 32) and scales.shape == (rows, nb)
    np.testing.assert_array_equal(scales.astype(np.int64), e + 127)
    back = from_mxfp8(got_codes, scales)
    assert back.dtype == np.float32
    np.testing.assert_array_equal(back.view(np.uint32), x.view(np.uint32))  # signed zeros too


def test_error_bound_on_random_data():
    """|x − dq| <= max(|x| / 8, X · 2^-10), X the block's scale: the scaled
    value x / X is below 512; in e4m3's normal range [2^-6, 448] rounding to
    3 mantissa bits is off by at most 2^-4 relative, below 2^-6 by half a
    subnormal step (2^-10 · X absolute), and a value in (448, 512) that
    saturates to 448 loses less than 64 / 512 = 1/8 of itself."""
    rng = np.random.default_rng(1)
    rows, nb = 256, 16
    mag = np.ldexp(1.0, rng.integers(-30, 31, (rows, nb, 1)))
    x = (rng.uniform(-1, 1, (rows, nb, 32)) * mag).astype(np.float32)
    x[0, 0] = 0.0
    x[1, 1, ::2] = 0.0
    x[2, 2, 0] = np.float32(2.0 ** 30 * 0.99999)  # scaled value just under 512: saturates
    x = x.reshape(rows, nb * 32)
    codes, scales = to_mxfp8(x)
    dq = from_mxfp8(codes, scales).astype(np.float64)
    X = np.repeat(e8m0_to_f64(scales), 32, axis=-1)
    err = np.abs(x.astype(np.float64) - dq)
    bound = np.maximum(np.abs(x.astype(np.float64)) / 8, X * 2.0 ** -10)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"mxfp8 codec: worst |x - dq| / bound = {worst:.4f}")
    assert (err <= bound).all(), worst
    assert worst > 0.5  # the bound is not slack by more than a factor two
    assert (np.abs(from_fp8_e4m3_bits(codes)) == 448).any()  # a saturated element is among the data


def test_edge_cases():
    z = np.zeros((3, 64), np.float32)
    z[1, 5] = -0.0
    codes, scales = to_mxfp8(z)
    assert (scales == 127).all() and ((codes & 0x7F) == 0).all() and codes[1, 5] == 0x80

    x = np.ones((1, 96), np.float32)
    x[0, 3] = np.nan          # block 0: NaN beside ones
    x[0, 32:64] = np.nan      # block 1: nothing finite
    x[0, 70] = np.inf         # block 2: inf beside ones
    x[0, 71] = -np.inf
    codes, scales = to_mxfp8(x)
    # 1.0: floor(log2) = 0, e = -8, elements 256 = code 0x78
    np.testing.assert_array_equal(scales, [[119, 127, 119]])
    assert codes[0, 3] == 0x7F and (np.delete(codes[0, :32], 3) == 0x78).all()
    assert (codes[0, 32:64] == 0x7F).all()
    assert codes[0, 70] == 0x7E and codes[0, 71] == 0xFE and codes[0, 64] == 0x78
    assert np.isnan(from_mxfp8(codes, scales)[0, 3]) and from_mxfp8(codes, scales)[0, 70] == 448 * 2.0 ** -8

    # the clamp at e = -127: fp32 subnormals (floor(log2) - 8 < -127)
    tiny = np.full((1, 32), 2.0 ** -130, np.float32)
    codes, scales = to_mxfp8(tiny)
    # e = -138 clamps to -127: the elements are 2^-130 · 2^127 = 2^-3 (code 0x20), not 256
    assert scales[0, 0] == 0 and (codes == 0x20).all()
    np.testing.assert_array_equal(from_mxfp8(codes, scales), tiny)
    # the clamp at e = +127: reachable from float64 input only
    big = np.full((1, 32), 2.0 ** 200, np.float64)
    codes, scales = to_mxfp8(big)
    assert scales[0, 0] == 254 and (codes == 0x7E).all()
    # no input produces the E8M0 NaN byte
    rng = np.random.default_rng(2)
    with np.errstate(over="ignore"):
        wild = rng.standard_normal((64, 128)).astype(np.float32) * np.float32(1e38)
    wild[::3, ::5] = np.inf
    wild[::7, ::2] = np.nan
    assert (to_mxfp8(wild)[1] != 0xFF).all()
    assert np.isnan(e8m0_to_f64(np.array([0xFF], np.uint8))[0]) and e8m0_to_f64(np.array([0, 127, 254], np.uint8)).tolist() == [
        2.0 ** -127, 1.0, 2.0 ** 127]
    with pytest.raises(ValueError):
        to_mxfp8(np.zeros((2, 48), np.float32))


# ----------------------------------------------------------------- packing


def test_pack_unpack_round_trip():
    rng = np.random.default_rng(3)
    for R, nb in ((64, 4), (128, 8), (256, 12), (512, 20)):
        s = rng.integers(0, 255, (R, nb), dtype=np.uint8)
        p = pack_mx_scales(s)
        assert p.dtype == np.uint32 and p.shape == (nb // 4, R // 64, 64)
        np.testing.assert_array_equal(unpack_mx_scales(p), s)
    with pytest.raises(ValueError):
        pack_mx_scales(np.zeros((32, 4), np.uint8))


def test_pack_places_one_byte_by_the_kernel_header_formula():
    """kernels/sgemm_mxfp8.hip: byte i of dword (kt·R/64 + g)·64 + l is
    s[g·64 + i·16 + l % 16][kt·4 + l // 16]."""
    R, nb = 256, 12
    row, blk = 64 * 2 + 16 * 3 + 9, 4 * 1 + 2  # g = 2, i = 3, l % 16 = 9; kt = 1, l // 16 = 2
    s = np.zeros((R, nb), np.uint8)
    s[row, blk] = 0xAB
    p = pack_mx_scales(s).ravel()
    g, i, fr, kt, fq = 2, 3, 9, 1, 2
    lane = fq * 16 + fr
    index = (kt * (R // 64) + g) * 64 + lane
    assert index == 425
    assert int(p[index]) == 0xAB << (8 * i) == 0xAB000000
    assert np.count_nonzero(p) == 1


# ------------------------------------------------------------------ library


def test_mxfp8_library_entry():
    from cekirdekler_amd.ops.library import ARITY, LIBRARY, code_object

    names = ["cek_sgemm_mxfp8_128x128", "cek_sgemm_mxfp8_256x256pbx"]
    assert sorted(LIBRARY["sgemm_mxfp8"]) == names == sorted(v[3] for v in MXFP8_TILES.values())
    assert all(ARITY[k] == 6 for k in names)
    assert sorted(MXFP8_TILE_WAVES) == sorted(MXFP8_TILES)
    blob = open(code_object("sgemm_mxfp8"), "rb").read()
    for k in names:
        assert k.encode() + b"\0" in blob, k
    # the unit-scale library is as it was
    fp8 = ["cek_sgemm_fp8_128x128", "cek_sgemm_fp8_256x256pb", "cek_sgemm_fp8_256x256pbx"]
    assert sorted(LIBRARY["sgemm_fp8"]) == fp8 == sorted(v[3] for v in FP8_TILES.values())
    assert all(ARITY[k] == 4 for k in fp8)


# --------------------------------------------------------------- op objects


@pytest.fixture(scope="module")
def cpu_cr():
    cr = ck.ClNumberCruncher(ck.ClPlatforms.all().cpus(True), "__global__ void nop(float* x) {}")
    yield cr
    cr.dispose()


@pytest.mark.parametrize("tile", sorted(MXFP8_TILES))
def test_mxfp8_objects(cpu_cr, tile):
    M, N, K = 512, 256, 256
    g = GemmMxFp8(M, N, K, cruncher=cpu_cr, tile=tile)
    assert g.global_range == g.tiles * g.L and g.split_k == 1 and not g.exchange and not g.row_major_c
    assert g.A.is_fp8 and g.B.is_fp8 and g.A.N == M * K and g.B.N == N * K
    assert g.SA.array.dtype == np.uint8 and g.SA.N == M * K // 32 and g.SB.N == N * K // 32
    assert g.kernel == MXFP8_TILES[tile][3] and g.C.elements_per_work_item * g.L == g.BM * g.BN
    assert GemmMxFp8.__init__.__defaults__[1] == "256x256pbx"
    with pytest.raises(ValueError):
        GemmMxFp8(512, 512, 192, cruncher=cpu_cr, tile=tile)
    for call in (lambda: g.run_shells(2), lambda: g.run_host_shells(2), lambda: g.verify_shells(2),
                 lambda: g.verify_shells_full(2)):
        with pytest.raises(NotImplementedError):
            call()
    # the default data exercises the scales: block factors 2^-12 .. 2^12
    sa = g.SA.array.astype(np.int64) - 127
    assert sa.min() < -15 and sa.max() > -1 and len(np.unique(sa)) > 20
    a = from_mxfp8(g.A.array.reshape(M, K), g.SA.array.reshape(M, K // 32)).astype(np.float64)
    b = from_mxfp8(g.B.array.reshape(N, K), g.SB.array.reshape(N, K // 32)).astype(np.float64)
    assert 2.0 ** 11 < np.abs(a).max() <= 2.0 ** 12
    np.testing.assert_array_equal(g.reference(), a @ b.T)
    np.testing.assert_array_equal(g.reference(slice(3, 9)), (a @ b.T)[3:9])


def _plant(g, ref):
    tm, tn = tile_coords(np.arange(g.tiles), g.M, g.N, g.BM, g.BN, g.group_m)
    tiles = np.stack([ref[r * g.BM:(r + 1) * g.BM, c * g.BN:(c + 1) * g.BN].astype(np.float32)
                      for r, c in zip(tm, tn)])
    g.C.array[:] = rows_to_tile(tiles, g.geom).ravel()


@pytest.mark.parametrize("tile", sorted(MXFP8_TILES))
def test_mxfp8_result_and_verify_full_include_the_scales(tile):
    """C planted as the fragment-ordered exact product (integers times
    power-of-two scales: exact in fp32): result() returns it, verify_full and
    verify are 0, and one perturbed element is found."""
    cpu = ck.ClPlatforms.all().cpus(True)
    cr = ck.ClNumberCruncher(cpu + cpu, "__global__ void nop(float* x) {}")
    M, N, K = 512, 768, 256
    g = GemmMxFp8(M, N, K, cruncher=cr, tile=tile, fill="none")
    rng = np.random.default_rng(4)
    g.A.array[:] = to_fp8_e4m3_bits(rng.integers(-4, 5, M * K).astype(np.float32))
    g.B.array[:] = to_fp8_e4m3_bits(rng.integers(-4, 5, N * K).astype(np.float32))
    g.SA.array[:] = 127 + rng.integers(-2, 3, g.SA.N)
    g.SB.array[:] = 127 + rng.integers(-2, 3, g.SB.N)
    ref = g.reference()
    unit = (from_fp8_e4m3_bits(g.A.array).reshape(M, K).astype(np.float64)
            @ from_fp8_e4m3_bits(g.B.array).reshape(N, K).astype(np.float64).T)
    assert (ref != unit).mean() > 0.5  # the scales are in the reference
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
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
    g = GemmMxFp8(256, 256, 128, cruncher=cpu_cr, tile="128x128")
    for upload in (True, True):
        g.SA.array[:] = np.arange(g.SA.N) % 251
        arrays = g._inputs(upload)
        assert len(arrays) == 5 and len(g._params()) == 5 and g._params()[-1] is g.C
        np.testing.assert_array_equal(unpack_mx_scales(arrays[3].array.reshape(1, 4, 64)), g.SA.array.reshape(256, 4))
        np.testing.assert_array_equal(unpack_mx_scales(arrays[4].array.reshape(1, 4, 64)), g.SB.array.reshape(256, 4))
