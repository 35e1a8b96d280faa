"""fp8 e4m3fn on the host (no GPU): the numpy codec against torch, fp8
arrays, the auxiliary-function codec on the CPU device, the GemmFp8 op
objects and the kernel library entry."""
import numpy as np
import pytest
import torch

import cekirdekler_amd as ck
from cekirdekler_amd.ops.gemm import (FP8_TILES, GemmFp8, from_fp8_e4m3_bits, rows_to_tile, tile_coords,
                                      to_fp8_e4m3_bits)

CODES = np.arange(256, dtype=np.uint8)
FINITE = CODES[(CODES & 0x7F) != 0x7F]  # the 254 non-NaN codes


def _torch_decode(codes):
    return torch.from_numpy(np.ascontiguousarray(codes)).view(torch.float8_e4m3fn).float().numpy()


def _midpoints():
    """Every midpoint between neighbouring code values (the rounding ties), both signs."""
    pos = np.sort(_torch_decode(CODES[:0x7F]).astype(np.float64))  # 0 .. 448
    mid = ((pos[:-1] + pos[1:]) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (pos[:-1] + pos[1:]) / 2)  # exact in fp32
    return np.concatenate([mid, -mid])


# ------------------------------------------------------------------- codec


def test_decode_matches_torch_on_all_256_codes():
    want = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy()
    got = from_fp8_e4m3_bits(CODES)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32)[FINITE], want.view(np.uint32)[FINITE])  # signed zeros too
    assert np.isnan(got[[0x7F, 0xFF]]).all() and np.isnan(want[[0x7F, 0xFF]]).all()


def test_encode_decode_is_identity_on_finite_codes():
    got = to_fp8_e4m3_bits(from_fp8_e4m3_bits(FINITE))
    assert got.dtype == np.uint8
    np.testing.assert_array_equal(got, FINITE)


def test_encode_matches_torch_bit_for_bit():
    rng = np.random.default_rng(0)
    x = np.concatenate([
        rng.uniform(-448, 448, 200_000), rng.normal(0, 1, 200_000), rng.uniform(-0.03, 0.03, 200_000),
        _torch_decode(FINITE).astype(np.float64), _midpoints().astype(np.float64)]).astype(np.float32)
    want = torch.from_numpy(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    got = to_fp8_e4m3_bits(x)
    bad = np.flatnonzero(got != want)  # bit patterns: +0 and -0 differ
    assert bad.size == 0, (bad.size, x[bad[:8]], got[bad[:8]], want[bad[:8]])


def test_encode_saturates_and_keeps_nan():
    big = np.array([449.0, 1e6, np.inf, 464.0, 480.0, 3e38], np.float32)
    np.testing.assert_array_equal(to_fp8_e4m3_bits(big), np.full(big.size, 0x7E, np.uint8))
    np.testing.assert_array_equal(to_fp8_e4m3_bits(-big), np.full(big.size, 0xFE, np.uint8))
    np.testing.assert_array_equal(from_fp8_e4m3_bits(to_fp8_e4m3_bits(np.array([449.0, -np.inf], np.float32))),
                                  np.array([448.0, -448.0], np.float32))
    np.testing.assert_array_equal(to_fp8_e4m3_bits(np.array([np.nan, -np.nan], np.float32)), [0x7F, 0x7F])
    np.testing.assert_array_equal(to_fp8_e4m3_bits(np.array([0.0, -0.0, 2.0 ** -9, -2.0 ** -10], np.float32)),
                                  [0x00, 0x80, 0x01, 0x80])  # 2^-10 is the tie between 0 and 2^-9: to even


# ------------------------------------------------------------------ arrays


@pytest.mark.parametrize("dtype", ["float8_e4m3fn", "fp8", "e4m3", torch.float8_e4m3fn])
@pytest.mark.parametrize("fast", [None, False])
def test_fp8_clarray(dtype, fast):
    a = ck.ClArray(64, dtype, fast=fast)
    assert a.array.dtype == np.uint8 and a.is_fp8 and not a.is_bf16
    assert a.dtype_name == "float8_e4m3fn" and a.itemsize == 1 and a.nbytes == 64
    a.array[:] = to_fp8_e4m3_bits(np.linspace(-3, 3, 64).astype(np.float32))
    t = a.to_torch()
    assert t.dtype == torch.float8_e4m3fn
    np.testing.assert_array_equal(t.float().numpy(), from_fp8_e4m3_bits(a.array))
    a.array[5] = 0x38  # 1.0: the view shares the storage
    assert float(t[5].float()) == 1.0
    b = ck.ClArray(a)
    assert b.is_fp8 and b.dtype_name == "float8_e4m3fn"


def test_fp8_fastarr_and_typed_array():
    f = ck.FastArr(32, "float8_e4m3fn")
    assert f.array.dtype == np.uint8 and f.is_fp8 and not f.is_bf16
    t = ck.ClFp8Array(48)
    assert isinstance(t, ck.FastArr) and t.array.dtype == np.uint8 and t.is_fp8 and len(t) == 48
    a = ck.ClArray(t)
    assert a.is_fp8 and a.fast_arr and a.to_torch().dtype == torch.float8_e4m3fn
    a.fast_arr = False  # storage switches keep the element type
    assert a.is_fp8 and a.array.dtype == np.uint8
    a.fast_arr = True
    assert a.is_fp8 and a._fast.is_fp8
    a.N = 16
    assert a.is_fp8 and a.N == 16 and a.dtype_name == "float8_e4m3fn"


def test_wrapped_torch_fp8_tensor_is_zero_copy():
    t = torch.tensor([1.0, -2.0, 0.5, 448.0]).to(torch.float8_e4m3fn)
    a = ck.ClArray(t)
    assert a.is_fp8 and a.array.dtype == np.uint8 and a.dtype_name == "float8_e4m3fn"
    np.testing.assert_array_equal(a.array, [0x38, 0xC0, 0x30, 0x7E])
    a.array[0] = 0x40  # 2.0, written through the array
    assert float(t[0].float()) == 2.0
    t.view(torch.uint8)[1] = 0x38  # written through the tensor
    assert a.array[1] == 0x38


def test_bf16_arrays_are_not_fp8():
    a = ck.ClArray(16, "bfloat16")
    assert a.is_bf16 and not a.is_fp8 and a.dtype_name == "bfloat16" and a.array.dtype == np.uint16
    assert ck.ClBf16Array(8).is_bf16 and not ck.ClBf16Array(8).is_fp8
    u = ck.ClArray(16, np.uint8)
    assert not u.is_fp8 and not u.is_bf16 and u.dtype_name == "uint8"
    assert ck.ClArray(4).dtype_name == "float32"


# ----------------------------------------------------------- aux functions

AUX_SRC = """
__global__ void dec(const unsigned char* c, float* f) {
  long long i = get_global_id(0);
  f[i] = cek_fp8_e4m3_to_f32(c[i]);
}
__global__ void enc(const float* f, unsigned char* c) {
  long long i = get_global_id(0);
  c[i] = cek_f32_to_fp8_e4m3(f[i]);
}
"""


def aux_codec_case(devices):
    """Decode all 256 codes and encode the finite code values, the ties and
    the range ends on ``devices``; both must equal the numpy codec exactly.
    (Shared with the GPU tier.)"""
    cr = ck.ClNumberCruncher(devices, ck.ClBuiltInAuxilliaryFunctions(fp8=True).wrap(AUX_SRC))
    assert cr.error_code() == 0, cr.error_message()
    codes = ck.ClArray(CODES.copy())
    out = ck.ClArray(np.zeros(256, np.float32))
    codes.write = False
    codes.next_param(out).compute(cr, 1, "dec", 256, 64)
    want = from_fp8_e4m3_bits(CODES)
    np.testing.assert_array_equal(out.array.view(np.uint32)[FINITE], want.view(np.uint32)[FINITE])
    assert np.isnan(out.array[[0x7F, 0xFF]]).all()

    x = np.concatenate([from_fp8_e4m3_bits(FINITE), _midpoints(),
                        np.array([449, -449, 1e6, -1e6, np.inf, -np.inf, np.nan, 1e-30, -1e-30], np.float32)])
    x = np.concatenate([x, np.zeros(-len(x) % 64, np.float32)])
    src = ck.ClArray(x)
    got = ck.ClArray(np.zeros(len(x), np.uint8))
    src.write = False
    src.next_param(got).compute(cr, 2, "enc", len(x), 64)
    np.testing.assert_array_equal(got.array, to_fp8_e4m3_bits(x))
    cr.dispose()


def test_aux_fp8_codec_on_cpu_device():
    aux_codec_case(ck.ClPlatforms.all().cpus(True))


# --------------------------------------------------------------- op objects


@pytest.fixture(scope="module")
def cpu_cr():
    cr = ck.ClNumberCruncher(ck.ClPlatforms.all().cpus(True), "__global__ void nop(float* x) {}")
    yield cr
    cr.dispose()


@pytest.mark.parametrize("tile", sorted(FP8_TILES))
def test_fp8_objects(cpu_cr, tile):
    g = GemmFp8(512, 512, 256, cruncher=cpu_cr, tile=tile)
    assert g.global_range == g.tiles * g.L and g.split_k == 1 and not g.exchange and not g.row_major_c
    assert g.A.is_fp8 and g.B.is_fp8 and g.A.array.dtype == np.uint8 and g.A.N == 512 * 256
    assert g.kernel == FP8_TILES[tile][3] and g.C.elements_per_work_item * g.L == g.BM * g.BN
    with pytest.raises(ValueError):
        GemmFp8(512, 512, 192, cruncher=cpu_cr, tile=tile)
    a = from_fp8_e4m3_bits(g.A.array).reshape(512, 256).astype(np.float64)
    b = from_fp8_e4m3_bits(g.B.array).reshape(512, 256).astype(np.float64)
    assert np.abs(a).max() <= 1.0 and np.abs(a).max() > 0.9  # uniform [-1, 1), quantised
    np.testing.assert_array_equal(g.reference(), a @ b.T)


def _plant(g, ref):
    tm, tn = tile_coords(np.arange(g.tiles), g.M, g.N, g.BM, g.BN, g.group_m)
    tiles = np.stack([ref[r * g.BM:(r + 1) * g.BM, c * g.BN:(c + 1) * g.BN].astype(np.float32)
                      for r, c in zip(tm, tn)])
    g.C.array[:] = rows_to_tile(tiles, g.geom).ravel()


@pytest.mark.parametrize("tile", sorted(FP8_TILES))
def test_fp8_verify_full_checks_every_tile(tile):
    cpu = ck.ClPlatforms.all().cpus(True)
    cr = ck.ClNumberCruncher(cpu + cpu, "__global__ void nop(float* x) {}")
    g = GemmFp8(512, 768, 256, cruncher=cr, tile=tile)
    half = g.tiles // 2 * g.L
    cr.cores.set_state(1, [half, g.tiles * g.L - half], [[0.0, 0.0] for _ in range(10)], [1.0, 1.0])
    _plant(g, g.reference())
    err, checked = g.verify_full(1, host=True, device="cpu")
    assert checked == g.tiles and err < 1e-6, (err, checked)
    assert g.verify(1, host=True) < 1e-6
    g.C.array[g.C.N - 7] += 0.5  # one element of the last tile
    err, _ = g.verify_full(1, host=True, device="cpu")
    assert err > 1e-4
    cr.dispose()


def test_fp8_verify_shells_full_checks_every_block(cpu_cr):
    g = GemmFp8(1024, 1024, 256, cruncher=cpu_cr, tile="256x256pb", group_m=2)
    P = 2
    ref = g.reference().astype(np.float32)
    pm, pn = g.M // P, g.N // P
    parts = []
    for s in range(P):  # R_s then C_s, each tile-major in grouped order
        for rows, cols in (((s * pm, (s + 1) * pm), (0, (s + 1) * pn)), ((0, s * pm), (s * pn, (s + 1) * pn))):
            m, n = rows[1] - rows[0], cols[1] - cols[0]
            if m == 0:
                continue
            blk = ref[rows[0]:rows[1], cols[0]:cols[1]]
            tm, tn = tile_coords(np.arange((m // 256) * (n // 256)), m, n, 256, 256, g.group_m)
            tiles = np.stack([blk[r * 256:(r + 1) * 256, c * 256:(c + 1) * 256] for r, c in zip(tm, tn)])
            parts.append(rows_to_tile(tiles, g.geom).ravel())
    g.C.array[:] = np.concatenate(parts)
    np.testing.assert_array_equal(g.shells_result(P), ref)
    err, blocks = g.verify_shells_full(P, device="cpu")
    assert blocks == 16 and err < 1e-6
    assert g.verify_shells(P, samples=4) < 1e-6
    g.C.array[5] += 0.5
    assert g.verify_shells_full(P, device="cpu")[0] > 1e-4


# ------------------------------------------------------------------ library


def test_fp8_library_entry():
    from cekirdekler_amd.ops.library import ARITY, LIBRARY, code_object

    names = ["cek_sgemm_fp8_128x128", "cek_sgemm_fp8_256x256pb", "cek_sgemm_fp8_256x256pbx"]
    assert sorted(LIBRARY["sgemm_fp8"]) == names == sorted(v[3] for v in FP8_TILES.values())
    assert all(ARITY[k] == 4 for k in names)
    blob = open(code_object("sgemm_fp8"), "rb").read()
    for k in names:
        assert k.encode() + b"\0" in blob, k
