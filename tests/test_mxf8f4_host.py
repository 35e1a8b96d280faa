"""The mixed MXFP8 × MXFP4 GEMM on the host (no GPU): the import surface and
the library and arity tables, the GemmMxFp8Fp4 op object (two operand
formats, references, refusals, take_operand's per-operand format), the code
objects, the numpy emulation of the tile under the hypothesised maps, the
host twin of the GPU tier's scale-mapping probe, the probe's buffers and the
host model of the output modes."""
import numpy as np
import pytest

import cekirdekler_amd as ck
import gemm84_oracles as g84
from cekirdekler_amd.cruncher import ClComputeError
from cekirdekler_amd.ops import gemm
from cekirdekler_amd.ops.gemm import (MX_OUT_KERNELS, MX_OUTPUTS, GemmMxFp4, GemmMxFp8, from_mxfp4, from_mxfp8,
                                      pack_mx_scales, rows_to_tile, tile_coords, to_mxfp4, to_mxfp8, unpack_mx_scales)
from cekirdekler_amd.ops.library import ARITY, LIBRARY, code_object
from cekirdekler_amd.ops.quantize import gemm_out_model
from test_gemm_mx_out_host import assert_same_output, host_codec

TILES = ("128x128", "128x256pbx")


@pytest.fixture(scope="module")
def cpu_cr():
    cr = ck.ClNumberCruncher(ck.ClPlatforms.all().cpus(True), "__global__ void nop(float* x) {}")
    yield cr
    cr.dispose()


# ------------------------------------------------------------------ surface and tables


def test_import_surface_and_tables():
    for name in ("GemmMxFp8Fp4", "MXF8F4_TILES", "MXF8F4_TILE_WAVES", "MXF8F4_OUT_KERNELS", "MXF8F4_OUT_LIB"):
        assert hasattr(gemm, name), name
    assert issubclass(gemm.GemmMxFp8Fp4, GemmMxFp8) and not issubclass(gemm.GemmMxFp8Fp4, GemmMxFp4)
    assert sorted(gemm.MXF8F4_TILES) == sorted(TILES) == sorted(gemm.MXF8F4_TILE_WAVES)
    assert gemm.MXF8F4_TILES == {"128x128": (128, 128, 256, "cek_sgemm_mxf8f4_128x128"),
                                 "128x256pbx": (128, 256, 512, "cek_sgemm_mxf8f4_128x256pbx")}
    assert gemm.MXF8F4_TILE_WAVES == {"128x128": (2, 2, 4, 4), "128x256pbx": (2, 4, 4, 4)}
    for t, (BM, BN, L, _) in gemm.MXF8F4_TILES.items():
        WM, WN, FM, FN = gemm.MXF8F4_TILE_WAVES[t]
        assert (WM * 16 * FM, WN * 16 * FN, 64 * WM * WN) == (BM, BN, L)
    plain = sorted(v[3] for v in gemm.MXF8F4_TILES.values())
    assert sorted(LIBRARY["sgemm_mxf8f4"]) == plain and all(ARITY[k] == 6 for k in plain)
    outs = sorted(gemm.MXF8F4_OUT_KERNELS.values())
    assert sorted(LIBRARY["sgemm_mxf8f4_out"]) == outs and len(outs) == 6 and gemm.MXF8F4_OUT_LIB == "sgemm_mxf8f4_out"
    assert set(gemm.MXF8F4_OUT_KERNELS) == {("mxf8f4", t, o) for t in TILES for o in MX_OUTPUTS}
    for (_, t, o), k in gemm.MXF8F4_OUT_KERNELS.items():
        assert k == gemm.MXF8F4_TILES[t][3] + "_" + ("bf16" if o == "bfloat16" else o)
        assert ARITY[k] == (6 if o == "bfloat16" else 7)
    # the pure formats' tables took no new names
    assert len(LIBRARY["sgemm_mx_out"]) == 12 == len(MX_OUT_KERNELS) and not set(outs) & set(LIBRARY["sgemm_mx_out"])
    assert len(LIBRARY["sgemm_mxfp8"]) == len(LIBRARY["sgemm_mxfp4"]) == 2


def test_code_objects_export_their_kernels():
    for lib in ("sgemm_mxf8f4", "sgemm_mxf8f4_out"):
        blob = open(code_object(lib), "rb").read()
        for k in LIBRARY[lib]:
            assert k.encode() + b"\0" in blob, k


# ------------------------------------------------------------------------- op objects


@pytest.mark.parametrize("tile", TILES)
def test_constructed_state(cpu_cr, tile):
    M, N, K = 512, 512, 512
    g = gemm.GemmMxFp8Fp4(M, N, K, cruncher=cpu_cr, tile=tile)
    BM, BN, L, kname = gemm.MXF8F4_TILES[tile]
    assert (g.BM, g.BN, g.L, g.kernel) == (BM, BN, L, kname) and g.geom == gemm.MXF8F4_TILE_WAVES[tile]
    assert g.global_range == g.tiles * L == (M // BM) * (N // BN) * L and g.split_k == 1
    assert not g.exchange and not g.row_major_c and g.dims.array.tolist() == [M, N, K, 4, 1, 0, 0, 0]
    # two operand formats: A one e4m3 byte per element, B two e2m1 elements per byte
    assert g.A.is_fp8 and not g.A.is_fp4 and g.A.N == M * K and g.A.dtype_name == "float8_e4m3fn"
    assert g.B.is_fp4 and not g.B.is_fp8 and g.B.N == N * K // 2 and g.B.dtype_name == "float4_e2m1fn_x2"
    assert g.B.nbytes * 2 == GemmMxFp8(M, N, K, cruncher=cpu_cr, fill="none").B.nbytes  # half of MXFP8's B
    assert g.SA.N == M * K // 32 and g.SB.N == N * K // 32 and g._SAp.N == M * K // 128 and g._SBp.N == N * K // 128
    for a in (g.A, g.B, g._SAp, g._SBp, g.dims):
        assert a.write is False
    assert g.C.N == M * N and g.C.read is False and g.C.elements_per_work_item * L == BM * BN
    assert g._params() == (g.A, g.B, g._SAp, g._SBp, g.C) and len(g._params()) + 1 == ARITY[kname]
    assert gemm.GemmMxFp8Fp4.__init__.__defaults__[1] == "128x256pbx" and gemm.GemmMxFp8Fp4.K_MULTIPLE == 256
    assert g.flops == 2.0 * M * N * K and g._row_items() == K and g.can_stream()
    assert g.LIBS == ("sgemm_mxf8f4", "mx_quantize", "mx4_quantize")
    # fill="random" is GemmMxFp8's draw, through to_mxfp8 for A and to_mxfp4 for B
    rng = np.random.default_rng(0)
    xs = [np.ldexp(rng.uniform(-1, 1, (rows, K // 32, 32)), rng.integers(-12, 13, (rows, K // 32, 1)))
          .astype(np.float32).reshape(rows, K) for rows in (M, N)]
    for arr, sc, (codes, scales) in ((g.A, g.SA, to_mxfp8(xs[0])), (g.B, g.SB, to_mxfp4(xs[1]))):
        np.testing.assert_array_equal(arr.array, codes.ravel())
        np.testing.assert_array_equal(sc.array, scales.ravel())
    g8 = GemmMxFp8(M, N, K, cruncher=cpu_cr, tile="128x128")
    np.testing.assert_array_equal(g8.A.array, g.A.array)
    # every host reference decodes each operand by its own format
    a = from_mxfp8(g.A.array.reshape(M, K), g.SA.array.reshape(M, K // 32)).astype(np.float64)
    b = from_mxfp4(g.B.array.reshape(N, K // 2), g.SB.array.reshape(N, K // 32)).astype(np.float64)
    np.testing.assert_array_equal(g._operand("A"), a)
    np.testing.assert_array_equal(g._operand("B"), b)
    np.testing.assert_array_equal(g._operand_t("A", "cpu").numpy(), a)
    np.testing.assert_array_equal(g._operand_t("B", "cpu").numpy(), b)
    np.testing.assert_array_equal(g.reference(), a @ b.T)
    np.testing.assert_array_equal(g.reference(slice(3, 9)), (a @ b.T)[3:9])
    # the packed scales follow the public ones, by 128-k step, for both operands
    g.SA.array[:] = np.arange(g.SA.N) % 251
    arrays = g._inputs(True)
    assert arrays[:3] == (g.dims, g.A, g.B) and len(arrays) == 5
    np.testing.assert_array_equal(arrays[3].array.reshape(K // 128, M // 64, 64), pack_mx_scales(g.SA.array.reshape(M, -1)))
    np.testing.assert_array_equal(unpack_mx_scales(arrays[4].array.reshape(K // 128, N // 64, 64)),
                                  g.SB.array.reshape(N, K // 32))


@pytest.mark.parametrize("tile", TILES)
def test_refusals(cpu_cr, tile):
    BM, BN = gemm.MXF8F4_TILES[tile][:2]
    for shape in ((BM, BN, 128), (BM, BN, 384), (BM, BN, 0), (BM + 64, BN, 256), (BM, BN - 16, 256), (0, BN, 256),
                  (BM, -BN, 256), (BM, BN, -256)):
        with pytest.raises(ValueError, match="K%256"):
            gemm.GemmMxFp8Fp4(*shape, cruncher=cpu_cr, tile=tile)
    g = gemm.GemmMxFp8Fp4(BM, BN, 256, cruncher=cpu_cr, tile=tile, fill="none")
    with pytest.raises(KeyError):
        gemm.GemmMxFp8Fp4(256, 256, 256, cruncher=cpu_cr, tile="256x256pbx")
    # the shell paths are refused as in the parent
    for call in (lambda: g.run_shells(2), lambda: g.run_host_shells(2), lambda: g.verify_shells(2),
                 lambda: g.verify_shells_full(2)):
        with pytest.raises(NotImplementedError, match="GemmMxFp8Fp4"):
            call()
    go = gemm.GemmMxFp8Fp4(BM, BN, 256, cruncher=cpu_cr, tile=tile, fill="none", out="mxfp8", act="relu")
    for shell in (go.run_shells, go.run_host_shells, go.verify_shells, go.verify_shells_full):
        with pytest.raises(ValueError, match="shell"):
            shell()
    with pytest.raises(ValueError, match="stream_blobs"):
        go.run(resident=False, stream_blobs=2)
    with pytest.raises(ClComputeError, match="sgemm_mxf8f4_out"):
        go.run()  # this cruncher has no library kernels: a missing kernel is an error
    with pytest.raises(ValueError, match="act needs an output mode"):
        gemm.GemmMxFp8Fp4(BM, BN, 256, cruncher=cpu_cr, tile=tile, fill="none", act="relu")
    with pytest.raises(ValueError, match="'A' or 'B'"):
        g.quantize("C", np.zeros((BM, 256), np.float32))
    with pytest.raises(ValueError, match="elements"):
        g.quantize("B", np.zeros((BN, 128), np.float32))


@pytest.mark.parametrize("out", MX_OUTPUTS)
@pytest.mark.parametrize("tile", TILES)
def test_output_mode_objects(cpu_cr, tile, out):
    BM, BN, L, plain = gemm.MXF8F4_TILES[tile]
    M, N, K = 3 * BM, 2 * BN, 256
    g = gemm.GemmMxFp8Fp4(M, N, K, cruncher=cpu_cr, tile=tile, fill="none", group_m=2, out=out, act="relu")
    assert g.kernel == gemm.MXF8F4_OUT_KERNELS["mxf8f4", tile, out] and g.kernel in LIBRARY["sgemm_mxf8f4_out"]
    assert g.LIBS == gemm.GemmMxFp8Fp4.LIBS + ("sgemm_mxf8f4_out",) and "sgemm_mx_out" not in g.LIBS
    assert len(g._params()) + 1 == ARITY[g.kernel] and g.dims.array.tolist() == [M, N, K, 2, 1, 1, 0, 0]
    assert g.C is None and g.A.is_fp8 and g.B.is_fp4
    n = M * N
    assert g.Y.N == (n // 2 if out == "mxfp4" else n)
    assert (g.Y.is_bf16, g.Y.is_fp8, g.Y.is_fp4) == (out == "bfloat16", out == "mxfp8", out == "mxfp4")
    if out != "bfloat16":
        assert g.SY.N == n // 32 and g.Yp.N == n // 128
    # the pure formats build what they built
    for cls, fmt, t in ((GemmMxFp8, "mxfp8", "256x256pbx"), (GemmMxFp4, "mxfp4", "128x128")):
        p = cls(256, 256, 256, cruncher=cpu_cr, tile=t, fill="none", out=out)
        assert p.kernel == MX_OUT_KERNELS[fmt, t, out] and p.LIBS == cls.LIBS + ("sgemm_mx_out",)


def test_take_operand_asks_each_operand_its_own_format(cpu_cr):
    g = gemm.GemmMxFp8Fp4(512, 512, 512, cruncher=cpu_cr, fill="none")
    p8 = gemm.GemmMxFp8Fp4(512, 512, 256, cruncher=cpu_cr, fill="none", out="mxfp8", act="relu")
    p4 = gemm.GemmMxFp8Fp4(512, 512, 256, cruncher=cpu_cr, fill="none", out="mxfp4")
    pb = gemm.GemmMxFp8Fp4(512, 512, 256, cruncher=cpu_cr, fill="none", out="bfloat16")
    with pytest.raises(ValueError, match="'A' or 'B'"):
        g.take_operand("C", p8)
    for name, bad, fmt in (("A", p4, "mxfp8"), ("A", pb, "mxfp8"), ("B", p8, "mxfp4"), ("B", pb, "mxfp4")):
        with pytest.raises(ValueError, match=f"format mismatch: GemmMxFp8Fp4 takes a producer with out='{fmt}'"):
            g.take_operand(name, bad)
    with pytest.raises(ValueError, match="format mismatch"):
        g.take_operand("A", gemm.GemmMxFp8Fp4(512, 512, 256, cruncher=cpu_cr, fill="none"))
    assert not g._stale
    g.take_operand("A", p8)
    assert g.A is p8.Y and g.SA is p8.SY and g._SAp is p8.Yp and g._stale == {"A"} and g.A.N == 512 * 512
    g.take_operand("B", p4)
    assert g.B is p4.Y and g.SB is p4.SY and g._SBp is p4.Yp and g._stale == {"A", "B"} and g.B.N == 512 * 512 // 2
    assert g._inputs(True) == (g.dims,)
    with pytest.raises(ValueError, match=r"sync_operands\(\)"):
        g.run(resident=False)
    # the pure classes' message is as it was
    with pytest.raises(ValueError, match="format mismatch: GemmMxFp8 takes a producer with out='mxfp8'"):
        GemmMxFp8(512, 512, 512, cruncher=cpu_cr, fill="none").take_operand("A", p4)
    GemmMxFp4(512, 512, 512, cruncher=cpu_cr, fill="none").take_operand("B", p4)


def _plant(g, ref):
    tm, tn = tile_coords(np.arange(g.tiles), g.M, g.N, g.BM, g.BN, g.group_m)
    tiles = np.stack([ref[r * g.BM:(r + 1) * g.BM, c * g.BN:(c + 1) * g.BN].astype(np.float32)
                      for r, c in zip(tm, tn)])
    g.C.array[:] = rows_to_tile(tiles, g.geom).ravel()


@pytest.mark.parametrize("tile", TILES)
def test_result_and_verify_decode_both_formats(tile):
    """C planted as the fragment-ordered exact product (gemm84_oracles.int_case:
    exact in fp32): result() returns it, verify_full and verify are 0, and one
    perturbed element is found."""
    cpu = ck.ClPlatforms.all().cpus(True)
    cr = ck.ClNumberCruncher(cpu + cpu, "__global__ void nop(float* x) {}")
    shape = (384, 512, 256)
    a, b, ea, eb, ref = g84.int_case(shape)
    g = gemm.GemmMxFp8Fp4(*shape, cruncher=cr, tile=tile, fill="none")
    g84.set_operands(g, a, b, ea, eb)
    np.testing.assert_array_equal(g.reference(), ref)
    assert (ref != a.astype(np.float64) @ b.astype(np.float64).T).mean() > 0.5  # the scales are in the reference
    half = g.tiles // 2 * g.L
    cr.cores.set_state(1, [half, g.tiles * g.L - half], [[0.0, 0.0] for _ in range(10)], [1.0, 1.0])
    _plant(g, ref)
    np.testing.assert_array_equal(g.result(download=False).astype(np.float64), ref)
    err, checked = g.verify_full(1, host=True, device="cpu")
    assert checked == g.tiles and err == 0.0, (err, checked)
    assert g.verify(1, host=True) == 0.0
    g.C.array[g.C.N - 7] += 0.5 * float(np.abs(ref).max())
    assert g.verify_full(1, host=True, device="cpu")[0] > 1e-4
    cr.dispose()


# --------------------------------------------------------------- the tile, emulated


@pytest.mark.parametrize("shape", [(128, 128, 256), (128, 256, 768)])
def test_emulated_tile_reproduces_the_reference(cpu_cr, shape):
    """Staging layout, read offsets, register order and scale addressing of
    kernels/sgemm_mxf8f4.hip under the hypothesised maps (gemm84_oracles.emu_tile)
    give reference(), on exact data and on the class's default fill."""
    a, b, ea, eb, ref = g84.int_case(shape)
    g = gemm.GemmMxFp8Fp4(*shape, cruncher=cpu_cr, tile="128x128", fill="none")
    g84.set_operands(g, a, b, ea, eb)
    args = (g.A.array.reshape(g.M, g.K), g.B.array.reshape(g.N, g.K // 2), g.SA.array, g.SB.array)
    np.testing.assert_array_equal(g84.emu_tile(*args), ref)
    np.testing.assert_array_equal(g.reference(), ref)
    for kw in (dict(a_order="e2m1"), dict(swap_nibbles=True), dict(swap_steps="a"), dict(swap_steps="b"),
               dict(sa_tile_step=True), dict(sa_shift_rows=16)):
        wrong = g84.emu_tile(*args, **kw)
        if shape[2] == 256 and "sa_tile_step" in kw:  # one K-tile: kt + s is 2kt + s
            np.testing.assert_array_equal(wrong, ref)
        else:
            assert (wrong != ref).mean() > 0.5, kw
    r = gemm.GemmMxFp8Fp4(*shape, cruncher=cpu_cr, tile="128x128", seed=5)
    got = g84.emu_tile(r.A.array.reshape(r.M, r.K), r.B.array.reshape(r.N, r.K // 2), r.SA.array, r.SB.array)
    want = r.reference()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()  # float64 sums in another order


# ------------------------------------------------- the scale-mapping probe


@pytest.mark.parametrize("coeff", g84.PROBE_SA_BLOCK_COEFF)
def test_scale_mapping_probe_distinguishes_on_the_host(coeff):
    """The probe's expected C against what each named wrong map would give:
    A read with the e2m1 k order, the two steps exchanged on one operand (data,
    scales, or both), nibbles swapped, SA stepped by the 256-k tile instead of
    the 128-k step, a wrong op_sel (the scale row one fragment off), and the
    MXFP8 probe's own.  Every one of them differs from the expected C in more
    than half the elements; the closed forms of the maps the tile emulation can
    express equal what it returns."""
    want, wrong = g84.probe_expected_and_wrong(coeff)
    assert len(wrong) == 13
    for name, c in wrong.items():
        assert float((c != want).mean()) > 0.5, name
    (M, N, K), pick, a, b, ea, eb = g84.probe_case(coeff)
    args = (g84.a_codes(a), g84.pack_values(b), (127 + ea).astype(np.uint8), (127 + eb).astype(np.uint8))
    np.testing.assert_array_equal(g84.emu_tile(*args), want)
    for name, kw in (("A in e2m1 k order", dict(a_order="e2m1")), ("B nibbles swapped", dict(swap_nibbles=True)),
                     ("B steps exchanged", dict(swap_steps="b")), ("SA stepped by the K-tile", dict(sa_tile_step=True)),
                     ("A row + 16 (op_sel)", dict(sa_shift_rows=16))):
        np.testing.assert_array_equal(g84.emu_tile(*args, **kw), wrong[name], err_msg=name)


def test_single_instruction_probe_problems_are_well_formed():
    """The probe's buffers (no GPU): 31 problems, every expectation an fp32
    value, and the read-back helpers return the hypothesised maps when fed the
    expected answers."""
    names, a, b, sa, sb, sel = g84.probe_buffers()
    n = len(names)
    assert n == 31 and a.shape == (n * 2048,) and b.shape == (n * 1024,)
    assert sa.shape == sb.shape == (n * 256,) and sel.shape == (n,) and sel.min() >= 0 and sel.max() < 16
    assert set(g84.PROBE_IEEE) < set(names) and {"adjacent_k", "adjacent_blocks"} < set(names)
    answers = {k: np.where(p["want"][0] == 0, p["want"][1], np.nan).astype(np.float32)
               for k, p in g84.probe_problems().items()}
    for operand in "ab":
        np.testing.assert_array_equal(g84.measured_k_map(answers, operand), np.arange(128))
        for o in range(4):
            row, block, want_block = g84.measured_scale_map(answers, operand, o)
            np.testing.assert_array_equal(row, np.arange(16))
            np.testing.assert_array_equal(block, want_block)
            assert sorted(set(want_block.tolist())) == [0, 1, 2, 3]
    # adjacent_k: the measured rule drops what IEEE keeps in 72 places, keeps the rest
    ieee = g84.probe_problems()["adjacent_k"]["want"][1]
    cut = g84.adjacent_k_as_measured()
    assert (cut != ieee).sum() == 72 and (cut[cut != ieee] == 2.0 ** 10).all() and (ieee >= cut).all()


# ----------------------------------------------------- the host model of the output modes


@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("out", MX_OUTPUTS)
def test_output_model_of_the_mixed_reference(cpu_cr, out, act):
    """gemm_out_model applied to the mixed reference (rounded once to fp32, as
    the plain kernel stores it on exact data) equals the float64 host codecs."""
    shape = (256, 512, 256)
    a, b, ea, eb, ref = g84.int_case(shape)
    g = gemm.GemmMxFp8Fp4(*shape, cruncher=cpu_cr, fill="none", out=out, act=act)
    g84.set_operands(g, a, b, ea, eb)
    c32 = g.reference().astype(np.float32)
    np.testing.assert_array_equal(c32.astype(np.float64), ref)
    assert (c32 < 0).mean() > 0.3
    model = gemm_out_model(c32, out, act)
    assert_same_output(model, host_codec(c32, out, act), out, (out, act))
    assert model[0].shape == (256, 256 if out == "mxfp4" else 512)
