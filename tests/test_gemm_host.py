"""Host-side logic of the GEMM ops (no GPU): object set-up for every tile,
the shell decomposition, tile orders and the guards that run before any
kernel does."""
import hashlib
import json
import os

import numpy as np
import pytest

import cekirdekler_amd as ck
from cekirdekler_amd.ops.gemm import F32_TILES, TILES, GemmBf16, GemmF32, tile_coords


@pytest.fixture(scope="module")
def cpu_cr():
    cr = ck.ClNumberCruncher(ck.ClPlatforms.all().cpus(True), "__global__ void nop(float* x) {}")
    yield cr
    cr.dispose()


@pytest.mark.parametrize("tile", sorted(TILES))
def test_bf16_objects(cpu_cr, tile):
    g = GemmBf16(512, 512, 256, cruncher=cpu_cr, tile=tile)
    assert g.row_major_c == (tile == "256x256pbr")
    assert g.global_range == g.tiles * g.split_k * g.L
    if g.row_major_c:
        with pytest.raises(ValueError):
            g.run(resident=False)


@pytest.mark.parametrize("tile", sorted(F32_TILES))
def test_f32_objects(cpu_cr, tile):
    g = GemmF32(512, 512, 256, cruncher=cpu_cr, tile=tile)
    assert not g.row_major_c and not g.exchange


def test_shell_bounds_cover_every_tile(cpu_cr):
    g = GemmBf16(2048, 2048, 256, cruncher=cpu_cr, tile="256x256pb")
    bounds, a_sl, b_sl = g.shell_bounds(4)
    assert bounds[0] == 0 and bounds[-1] == g.global_range
    assert len(a_sl) == len(b_sl) == 4
    assert sum(n for _, n in a_sl) == g.A.N and sum(n for _, n in b_sl) == g.B.N
    # blob s holds exactly the tiles of shell s, which need panels 0..s only
    t = np.arange(g.tiles)
    tm, tn = tile_coords(t, 2048, 2048, 256, 256, g.group_m, 4)
    assert len(set(zip(tm.tolist(), tn.tolist()))) == g.tiles
    for s in range(4):
        lo, hi = bounds[s] // g.L, bounds[s + 1] // g.L
        assert tm[lo:hi].max() < (s + 1) * 2 and tn[lo:hi].max() < (s + 1) * 2
        assert ((tm[lo:hi] // 2 == s) | (tn[lo:hi] // 2 == s)).all()
    with pytest.raises(ValueError):
        g.shell_bounds(3)


@pytest.mark.parametrize("split_last", [1, 2, 4])
def test_shell_bounds_split_last_shells(cpu_cr, split_last):
    """The last shells split into R_s (row panel s, which uploads A_s and B_s)
    and C_s (column panel s above it, no upload); every blob holds exactly
    its part's tiles and only R_s blobs upload."""
    g = GemmBf16(2048, 2048, 256, cruncher=cpu_cr, tile="256x256pb")
    P, pt = 4, 2  # 4 panels of 2 tiles each way
    bounds, a_sl, b_sl = g.shell_bounds(P, split_last)
    nsplit = min(split_last, P - 1)
    assert len(bounds) == P + 1 + nsplit and bounds[-1] == g.global_range
    assert sum(n for _, n in a_sl) == g.A.N and sum(n for _, n in b_sl) == g.B.N
    t = np.arange(g.tiles)
    tm, tn = tile_coords(t, 2048, 2048, 256, 256, g.group_m, P)
    q = 0
    for s in range(P):
        parts = ("R", "C") if s >= P - split_last and s > 0 else ("RC",)
        for part in parts:
            lo, hi = bounds[q] // g.L, bounds[q + 1] // g.L
            rows, cols = tm[lo:hi] // pt, tn[lo:hi] // pt
            if part == "R":
                assert (rows == s).all() and (cols <= s).all() and hi - lo == (s + 1) * pt * pt
                assert a_sl[q][1] > 0 and b_sl[q][1] > 0
            elif part == "C":
                assert (cols == s).all() and (rows < s).all() and hi - lo == s * pt * pt
                assert a_sl[q][1] == 0 and b_sl[q][1] == 0
            else:
                assert ((rows == s) | (cols == s)).all()
            q += 1


def test_explicit_blob_count_does_not_stretch_the_range():
    """Explicit blob bounds whose count does not divide the range (split
    shells: 6 blobs over 16 tiles) leave the one device's range at exactly the
    global range; the equal-blob step (blobs × unit) once rounded it up to
    18 tiles, launching two work-groups past C."""
    src = ("__global__ void cek_sgemm_bf16_256x256pb(const int* d, const unsigned short* a, "
           "const unsigned short* b, float* c) {}")
    cr = ck.ClNumberCruncher(ck.ClPlatforms.all().cpus(True), src)
    g = GemmBf16(1024, 1024, 512, cruncher=cr, tile="256x256pb")
    for split in (0, 2, 3):
        g.run_shells(4, compute_id=3 + split, split_last=split)
        assert cr.ranges(3 + split) == [g.global_range]
    cr.dispose()


@pytest.mark.parametrize("cls,tile", [(GemmBf16, "256x256pb"), (GemmBf16, "256x256pbr"), (GemmBf16, "256x128pe"),
                                      (GemmF32, "256x256g8i")])
def test_verify_full_checks_every_tile(cls, tile):
    """the whole-output check compares every tile a
    process owns (untiled from the kernel's fragment order / tile order on
    the torch device) with a float64 product, and catches one wrong element
    anywhere."""
    from cekirdekler_amd.ops.gemm import rows_to_tile

    cpu = ck.ClPlatforms.all().cpus(True)
    cr = ck.ClNumberCruncher(cpu + cpu, "__global__ void nop(float* x) {}")
    g = cls(512, 768, 256, cruncher=cr, tile=tile)
    unit = g.L * g.split_k
    half = g.tiles // 2 * unit
    cr.cores.set_state(1, [half, g.tiles * unit - half], [[0.0, 0.0] for _ in range(10)], [1.0, 1.0])
    ref = g.reference()
    if g.row_major_c:
        g.C.array[:] = ref.astype(np.float32).ravel()
    else:
        tm, tn = tile_coords(np.arange(g.tiles), g.M, g.N, g.BM, g.BN, g.group_m)
        blocks = [ref[r * g.BM:(r + 1) * g.BM, c * g.BN:(c + 1) * g.BN].astype(np.float32) for r, c in zip(tm, tn)]
        tiles = np.stack(blocks)
        g.C.array[:] = (rows_to_tile(tiles, g.geom) if g.geom is not None else tiles).ravel()
    err, checked = g.verify_full(1, host=True, device="cpu")
    assert checked == g.tiles and err < 1e-6, (err, checked)
    g.C.array[g.C.N - 7] += 0.5  # one element of the last tile
    err, _ = g.verify_full(1, host=True, device="cpu")
    assert err > 1e-4
    cr.dispose()


def test_verify_shells_full_checks_every_block(cpu_cr):
    """The native shell stream's host C (shell layout) checked whole."""
    from cekirdekler_amd.ops.gemm import rows_to_tile, untile  # noqa: F401

    g = GemmBf16(1024, 1024, 256, cruncher=cpu_cr, tile="256x256pb", group_m=2)
    P = 2
    ref = g.reference().astype(np.float32)
    pm, pn = g.M // P, g.N // P
    parts = []
    for s in range(P):  # R_s then C_s, each tile-major in grouped order
        for rows, cols in (((s * pm, (s + 1) * pm), (0, (s + 1) * pn)),
                           ((0, s * pm), (s * pn, (s + 1) * pn))):
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
    g.C.array[5] += 1.0
    assert g.verify_shells_full(P, device="cpu")[0] > 1e-4


# --------------------------------------------------------------------------- the bf16 codec

BF16_AUX_SRC = """
__global__ void enc(const float* f, unsigned short* h) {
  long long i = get_global_id(0);
  h[i] = cek_f32_to_bf16(f[i]);
}
__global__ void dec(const unsigned short* h, float* f) {
  long long i = get_global_id(0);
  f[i] = cek_bf16_to_f32(h[i]);
}
"""
# NaNs whose rounding increment carries: into +Inf, -0, +0 and -Inf
BF16_NAN_PATTERNS = np.array([0x7F800001, 0x7FFFFFFF, 0xFFFFFFFF, 0xFF800001], np.uint32)


def bf16_codec_inputs():
    """fp32 bit patterns: the four NaNs an adding encoder loses, further NaNs
    of both signs, ±Inf, the largest finite values (they round to Inf), every
    tie of one binade with its neighbours, subnormals, zeros and 200 000
    random patterns; padded to a multiple of 64."""
    rng = np.random.default_rng(7)
    ties = (0x3F800000 + (np.arange(128, dtype=np.uint32) << 16) + 0x8000)  # both parities of the kept bit
    u = np.concatenate([
        BF16_NAN_PATTERNS, np.array([0x7FC00000, 0xFFC00000, 0x7F800100, 0xFF80FFFF, 0x7FBFFFFF], np.uint32),
        np.array([0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF], np.uint32),
        ties, ties - 1, ties + 1, ties | 0x80000000,
        np.array([0, 0x80000000, 1, 0x80000001, 0x7FFF, 0x8000, 0x8001, 0x18000, 0x007FFFFF, 0x807F8000], np.uint32),
        rng.integers(0, 2 ** 32, 200_000, dtype=np.uint64).astype(np.uint32)])
    return np.concatenate([u, np.zeros(-len(u) % 64, np.uint32)])


def assert_bf16_like_torch(x_bits, got):
    """Bit for bit torch's fp32 → bf16 conversion, except at NaNs: there the
    result must be a NaN of the input's sign (torch returns one canonical
    NaN for every NaN input, so its sign is not the reference)."""
    import torch

    want = torch.from_numpy(x_bits.view(np.float32).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = (x_bits & 0x7FFFFFFF) > 0x7F800000
    assert nan.sum() > 500 and (~nan).sum() > 190_000  # one random pattern in 256 is a NaN
    assert got.dtype == np.uint16
    bad = np.flatnonzero(got[~nan] != want[~nan])
    assert bad.size == 0, (bad.size, [hex(v) for v in x_bits[~nan][bad[:4]]], got[~nan][bad[:4]], want[~nan][bad[:4]])
    g, w = got[nan].astype(np.uint32), want[nan].astype(np.uint32)
    assert ((w & 0x7FFF) > 0x7F80).all()                      # torch: NaN
    assert ((g & 0x7FFF) > 0x7F80).all(), [hex(v) for v in x_bits[nan][(g & 0x7FFF) <= 0x7F80][:4]]
    assert np.array_equal(g >> 15, x_bits[nan] >> 31)         # the sign is kept
    assert np.array_equal(g, (x_bits[nan] >> 16) | 0x40)      # and the top payload bits, quiet bit set


def bf16_aux_codec_case(devices):
    """cek_f32_to_bf16 and cek_bf16_to_f32 on ``devices`` over
    bf16_codec_inputs, one launch each: the encoder as assert_bf16_like_torch
    has it, the decoder the exact widening.  (Shared with the GPU tier.)"""
    from cekirdekler_amd.ops.gemm import from_bf16_bits, to_bf16_bits

    cr = ck.ClNumberCruncher(devices, ck.ClBuiltInAuxilliaryFunctions(bf16=True).wrap(BF16_AUX_SRC))
    assert cr.error_code() == 0, cr.error_message()
    u = bf16_codec_inputs()
    src = ck.ClArray(u.view(np.float32).copy())
    enc = ck.ClArray(np.zeros(len(u), np.uint16))
    src.write = False
    src.next_param(enc).compute(cr, 1, "enc", len(u), 64)
    assert_bf16_like_torch(u, enc.array)
    np.testing.assert_array_equal(enc.array, to_bf16_bits(u.view(np.float32)))
    back = ck.ClArray(np.zeros(len(u), np.float32))
    enc.write = False
    enc.next_param(back).compute(cr, 2, "dec", len(u), 64)
    np.testing.assert_array_equal(back.array.view(np.uint32), enc.array.astype(np.uint32) << 16)
    np.testing.assert_array_equal(back.array.view(np.uint32), from_bf16_bits(enc.array).view(np.uint32))
    cr.dispose()


def test_bf16_encoder_keeps_every_nan():
    from cekirdekler_amd.ops.gemm import from_bf16_bits, to_bf16_bits

    got = to_bf16_bits(BF16_NAN_PATTERNS.view(np.float32))
    np.testing.assert_array_equal(got, [0x7FC0, 0x7FFF, 0xFFFF, 0xFFC0])
    assert np.isnan(from_bf16_bits(got)).all()
    np.testing.assert_array_equal(to_bf16_bits(np.array([np.inf, -np.inf, 3.4028235e38, -3.4028235e38], np.float32)),
                                  [0x7F80, 0xFF80, 0x7F80, 0xFF80])


def test_bf16_encoder_matches_torch_bit_for_bit():
    from cekirdekler_amd.ops.gemm import to_bf16_bits

    u = bf16_codec_inputs()
    assert_bf16_like_torch(u, to_bf16_bits(u.view(np.float32)))


def test_aux_bf16_codec_on_cpu_device():
    bf16_aux_codec_case(ck.ClPlatforms.all().cpus(True))


# ---------------------------------------------------- constructed state, imports

GOLDEN_STATE = os.path.join(os.path.dirname(__file__), "golden", "gemm_state.json")
STATE_ARRAYS = ("A", "B", "C", "SA", "SB", "_SAp", "_SBp", "W", "counters")


def gemm_state_cases():
    """``(id, class, shape, keywords)``: every class × every tile of its table
    at M = BM, N = 2·BN, K = twice the class's K multiple; bf16 also with
    ``split_k=2`` on the split-K tiles, and its exchange tiles once more at a
    K long enough for a nonzero ``exchange_shift``."""
    from cekirdekler_amd.ops import gemm

    cases = []
    for cls, table, kmult in ((gemm.GemmBf16, gemm.TILES, 64), (gemm.GemmF32, gemm.F32_TILES, 32),
                              (gemm.GemmFp8, gemm.FP8_TILES, 128), (gemm.GemmMxFp8, gemm.MXFP8_TILES, 128),
                              (gemm.GemmMxFp4, gemm.MXFP4_TILES, 256)):
        for tile in sorted(table):
            BM, BN = table[tile][:2]
            cases.append((f"{cls.__name__}-{tile}", cls, (BM, 2 * BN, 2 * kmult), {"tile": tile}))
            if cls is gemm.GemmBf16 and tile in gemm.SPLIT_K_TILES:
                cases.append((f"{cls.__name__}-{tile}-sk2", cls, (BM, 2 * BN, 2 * kmult), {"tile": tile, "split_k": 2}))
            if cls is gemm.GemmBf16 and tile in gemm.EXCHANGE_TILES:
                cases.append((f"{cls.__name__}-{tile}-k1024", cls, (BM, 2 * BN, 1024), {"tile": tile}))
                cases.append((f"{cls.__name__}-{tile}-k1024-shift2", cls, (BM, 2 * BN, 1024),
                              {"tile": tile, "exchange_shift": 2, "handover_spin_limit": -1}))
    return cases


def gemm_state(g) -> dict:
    """What a constructor leaves behind, as JSON can hold it."""
    s = {k: getattr(g, k) for k in ("kernel", "global_range", "split_k", "exchange", "exchange_shift", "row_major_c")}
    s["geom"] = None if g.geom is None else list(g.geom)
    s["dims"] = g.dims.array.tolist()
    s["arrays"] = {}
    for name in STATE_ARRAYS:
        a = getattr(g, name, None)
        if a is not None:
            s["arrays"][name] = {"N": a.N, "dtype": a.dtype_name, "read": a.read, "write": a.write,
                                 "elements_per_work_item": a.elements_per_work_item}
    s["sha256"] = {name: hashlib.sha256(getattr(g, name).array.tobytes()).hexdigest()
                   for name in ("A", "B", "SA", "SB") if hasattr(g, name)}
    return s


def test_constructed_state_matches_parent(cpu_cr):
    """Every class × tile builds the object the per-class constructors built
    before they were folded into one: tests/golden/gemm_state.json was written
    by those, with ``seed=0``."""
    with open(GOLDEN_STATE) as f:
        want = json.load(f)
    cases = gemm_state_cases()
    assert sorted(want) == sorted(c[0] for c in cases)
    for cid, cls, shape, kw in cases:
        assert gemm_state(cls(*shape, cruncher=cpu_cr, seed=0, **kw)) == want[cid], cid


# every name tests/, bench/, bench.py, tools/ and __graft_entry__.py take from
# cekirdekler_amd.ops.gemm (``from … import X`` and ``gemm.X``), by home module
GEMM_NAMES = ("TILES", "TILE_WAVES", "GEMM_LIBS", "F32_TILES", "FP8_TILES", "MXFP8_TILES", "MXFP8_TILE_WAVES",
              "MXFP4_TILES", "MXFP4_TILE_WAVES", "SPLIT_K_TILES", "EXCHANGE_TILES", "EXCHANGE_SHIFT", "GemmBf16",
              "GemmF32", "GemmFp8", "GemmMxFp8", "GemmMxFp4", "decode_operand", "library")
CODEC_NAMES = ("to_bf16_bits", "from_bf16_bits", "to_fp8_e4m3_bits", "from_fp8_e4m3_bits", "e8m0_to_f64",
               "to_fp4_e2m1_codes", "from_fp4_e2m1_codes", "pack_fp4", "unpack_fp4", "to_mxfp8", "from_mxfp8",
               "to_mxfp4", "from_mxfp4")
TILING_NAMES = ("tile_to_rows", "rows_to_tile", "tile_coords", "untile", "pack_mx_scales", "unpack_mx_scales")


def test_gemm_module_keeps_its_import_surface():
    from cekirdekler_amd.ops import codecs, gemm, quantize, tiling

    for name in GEMM_NAMES + CODEC_NAMES + TILING_NAMES + ("MX_BLOCK", "FP4_E2M1_EMAX", "ROW_MAJOR_TILES"):
        assert hasattr(gemm, name), name
    for home, names in ((codecs, CODEC_NAMES), (tiling, TILING_NAMES)):
        for name in names:
            assert getattr(gemm, name) is getattr(home, name), name
            assert getattr(home, name).__module__ == home.__name__, name
    assert gemm.MX_BLOCK == codecs.MX_BLOCK == quantize.MX_BLOCK == 32 and gemm.FP4_E2M1_EMAX == codecs.FP4_E2M1_EMAX == 2
    for name in ("to_mxfp8", "to_mxfp4", "from_bf16_bits", "pack_fp4"):  # the quantisers' codecs are the same objects
        assert getattr(quantize, name) is getattr(codecs, name), name
    assert gemm.MxFp8Quantizer is quantize.MxFp8Quantizer and gemm.MxFp4Quantizer is quantize.MxFp4Quantizer
