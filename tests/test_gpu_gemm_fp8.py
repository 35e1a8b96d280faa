"""GPU tier of the fp8 e4m3 GEMM (kernels/sgemm_fp8.hip, GemmFp8): exact
data first (integers, a k-pairing probe, the ends of the e4m3 range), then
random data against a derived bound, then the multi-device and host-resident
paths, the auxiliary-function codec on the GPU, and the NaN-code and
ragged-tile-group cases of gemm8_oracles.py."""
import numpy as np
import pytest

import cekirdekler_amd as ck
import gemm8_oracles as g8
import gemm_oracles as go
from cekirdekler_amd.ops.gemm import FP8_TILES, GemmFp8, from_fp8_e4m3_bits, to_fp8_e4m3_bits
from cekirdekler_amd.ops.library import library

pytestmark = pytest.mark.gpu

# K/128 = 1, 2, 3, 5: the ping-pong prologue stages two K-tiles ahead and the
# Bt ring has three buffers, so these are the counts at which the loop ends
# can go wrong
K_TAIL_SHAPES = [(256, 256, 128), (512, 256, 256), (256, 512, 384), (1024, 768, 640)]
SHAPES = {"256x256pb": K_TAIL_SHAPES, "256x256pbx": K_TAIL_SHAPES,
          "128x128": K_TAIL_SHAPES + [(128, 128, 128), (384, 128, 256)]}
TILE_SHAPES = [(t, s) for t in sorted(FP8_TILES) for s in SHAPES[t]]


@pytest.fixture(scope="module")
def cr():
    c = ck.ClNumberCruncher(ck.ClPlatforms.all().gpus()[0], "", prebuilt=library("sgemm_fp8"))
    yield c
    c.dispose()


def _set(g, a, b):
    """Operands from exactly representable values (checked)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    g.A.array[:] = to_fp8_e4m3_bits(a).ravel()
    g.B.array[:] = to_fp8_e4m3_bits(b).ravel()
    assert np.array_equal(from_fp8_e4m3_bits(g.A.array), a.ravel())
    assert np.array_equal(from_fp8_e4m3_bits(g.B.array), b.ravel())


_INT_CACHE = {}


def _int_case(shape):
    """Integers in [-8, 8] (exact in e4m3) and their int64 product, once per shape."""
    if shape not in _INT_CACHE:
        M, N, K = shape
        rng = np.random.default_rng(sum(shape))
        a = rng.integers(-8, 9, (M, K))
        b = rng.integers(-8, 9, (N, K))
        ref = a @ b.T
        ref.setflags(write=False)
        _INT_CACHE[shape] = (a, b, ref)
    return _INT_CACHE[shape]


def _int_gemm(shape, **kw):
    a, b, ref = _int_case(shape)
    g = GemmFp8(*shape, fill="none", **kw)
    _set(g, a, b)
    return g, ref


def _assert_exact(c, ref):
    assert c.dtype == np.float32
    bad = np.argwhere(c.astype(np.float64) != ref)
    assert bad.size == 0, (len(bad), bad[:4].tolist(), [float(c[tuple(i)]) for i in bad[:4]],
                           [float(ref[tuple(i)]) for i in bad[:4]])


@pytest.mark.parametrize("tile,shape", TILE_SHAPES)
def test_exact_integers(cr, tile, shape):
    """Every product and partial sum is an integer below 2^24 (64·K <= 40 960):
    the fp32 result is exact in any summation order, so C equals the int64
    product bit for bit."""
    g, ref = _int_gemm(shape, cruncher=cr, tile=tile, group_m=2)
    g.C.array[:] = np.nan
    g.run(resident=True)
    _assert_exact(g.result(), ref)


@pytest.mark.parametrize("tile", sorted(FP8_TILES))
def test_k_pairing_and_orientation(cr, tile):
    """A picks one k per row, B is asymmetric in n and k: C[m][n] must be
    B[n][(37m + 11) % K].  A lane map that pairs A's k with another k of B
    fails, and so does a C store with row and column swapped."""
    M, N, K = 256, 512, 384
    pick = (37 * np.arange(M) + 11) % K
    a = np.zeros((M, K), np.float32)
    a[np.arange(M), pick] = 1
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    b = ((3 * n + 5 * k) % 17 - 8).astype(np.float32)
    g = GemmFp8(M, N, K, cruncher=cr, tile=tile, fill="none")
    _set(g, a, b)
    g.run(resident=True)
    _assert_exact(g.result(), b[:, pick].T.astype(np.float64))


@pytest.mark.parametrize("tile", sorted(FP8_TILES))
def test_range_ends(cr, tile):
    """±448: products are multiples of 2^12 and the sums fit 24 bits.  ±2^-9
    (the smallest subnormal): every C is the signed count times 2^-18;
    subnormal inputs flushed to zero would give 0."""
    M = N = K = 256
    rng = np.random.default_rng(5)
    sa = rng.choice([-1.0, 1.0], (M, K))
    sb = rng.choice([-1.0, 1.0], (N, K))
    count = sa @ sb.T
    for mag in (448.0, 2.0 ** -9):
        g = GemmFp8(M, N, K, cruncher=cr, tile=tile, fill="none")  # resident operands go up once per object
        _set(g, sa * mag, sb * mag)
        g.C.array[:] = np.nan
        g.run(resident=True)
        _assert_exact(g.result(), count * (mag * mag))
    assert np.abs(count).max() > 0


@pytest.mark.parametrize("tile", sorted(FP8_TILES))
def test_random_data_within_derived_bound(cr, tile):
    """|C - ref| <= K · 2^-23 · Σ_k |a_k·b_k| per element: the products of two
    e4m3 values are exact in fp32, what remains is K fp32 additions in some
    order, each off by at most one unit in the last place (2^-23: an adder
    that truncates is covered) of a partial sum of magnitude <= Σ|a·b|.
    (Measured since: the matrix core sums 8 neighbouring products in 14 bits,
    test_gpu_gemm_mxfp8.py::test_probe_adjacent_k_sum_as_measured, so this
    derivation is not a guarantee for every data set; on these uniform draws
    the bound holds with the margin printed below.)"""
    M, N, K = 1024, 512, 512
    g = GemmFp8(M, N, K, cruncher=cr, tile=tile, fill="random", seed=3)
    a = from_fp8_e4m3_bits(g.A.array).reshape(M, K).astype(np.float64)
    b = from_fp8_e4m3_bits(g.B.array).reshape(N, K).astype(np.float64)
    ref = a @ b.T
    bound = K * 2.0 ** -23 * (np.abs(a) @ np.abs(b).T)
    g.run(resident=True)
    err = np.abs(g.result().astype(np.float64) - ref)
    ratio = float((err / bound).max())
    rel = float(err.max() / np.abs(ref).max())
    print(f"fp8 {tile} {M}x{N}x{K}: worst |C-ref|/bound = {ratio:.3e}, max|C-ref|/max|ref| = {rel:.3e}")
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
    c2 = ck.ClNumberCruncher(g0 + g0, "", prebuilt=library("sgemm_fp8"))
    g, ref = _int_gemm((1024, 1024, 256), cruncher=c2, tile="256x256pb")
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
    g, ref = _int_gemm((1024, 512, 256), cruncher=cr, tile="256x256pb")
    g.C.array[:] = np.nan
    g.run(resident=False)
    _assert_exact(g.result(download=False), ref)


@pytest.mark.parametrize("group_m", [2, 1])
def test_host_resident_streamed_blobs(cr, group_m):
    """Four blobs per device.  The 8 tiles are 4 / group_m tile groups (the
    blob unit: one A row panel each), so group_m = 1 runs the event pipeline
    and group_m = 2, with fewer groups than blobs, the plain path."""
    g, ref = _int_gemm((1024, 512, 256), cruncher=cr, tile="256x256pb", group_m=group_m)
    assert g.can_stream()
    g.C.array[:] = np.nan
    g.run(resident=False, stream_blobs=4)
    assert cr.last_record()["pipelined"] == (group_m == 1)
    _assert_exact(g.result(download=False), ref)


def test_shells_through_compute(cr):
    g, ref = _int_gemm((1024, 1024, 256), cruncher=cr, tile="256x256pb")
    g.C.array[:] = np.nan
    g.run_shells(2, compute_id=3)
    rec = cr.last_record()
    assert rec["pipelined"] and rec["h2d_bytes"] == g.A.array.nbytes + g.B.array.nbytes + g.dims.array.nbytes, rec
    _assert_exact(g.result(download=False), ref)
    assert g.verify(compute_id=3, host=True) == 0.0


def test_host_shells(cr):
    g, ref = _int_gemm((1024, 1024, 256), cruncher=cr, tile="256x256pb", group_m=2)
    g.C.array[:] = np.nan
    g.run_host_shells(2)
    _assert_exact(g.shells_result(2), ref)
    err, blocks = g.verify_shells_full(2)
    assert blocks == 16 and err == 0.0


def test_aux_fp8_decode_on_gpu():
    """The case of the CPU tier on the GPU: all 256 codes decoded; the finite
    code values, every rounding tie, saturation and NaN encoded."""
    from test_fp8_host import aux_codec_case

    aux_codec_case(ck.ClPlatforms.all().gpus()[0])


# --------------------------------------------------------------------------- NaN codes and ragged tile groups
# (tests/gemm8_oracles.py has the cases, test_gemm8_oracles.py what they reject)

def _set_codes(g, case):
    """Operands from a gemm8_oracles case: the codes as they are (NaN codes included)."""
    a, b, _, _, want = case
    g.A.array[:] = a.ravel()
    g.B.array[:] = b.ravel()
    return want


@pytest.mark.parametrize("shape", g8.CLASS_SHAPES)
@pytest.mark.parametrize("tile", sorted(FP8_TILES))
def test_nonfinite(cr, tile, shape):
    """The e4m3 NaN codes 0x7F and 0xFF in A (first and last K-tile) and 0x7F
    in Bt (middle K-tile) poison exactly their row or column of C, 0·NaN
    included; every other element, in other fragments, waves and tiles, is
    the exact integer product."""
    g = GemmFp8(*shape, cruncher=cr, tile=tile, fill="none")
    want = _set_codes(g, g8.fp8_nonfinite(shape))
    g.C.array[:] = 1.0  # a leftover NaN must not pass for a computed one
    g.run(resident=True)
    go.assert_nonfinite(g.result(), want)


@pytest.mark.parametrize("tile,shape,group_m", [(t, s, gm) for t in sorted(FP8_TILES) for s, gm in g8.ragged_groups(t)])
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
    c2 = ck.ClNumberCruncher(g0 + g0, "", prebuilt=library("sgemm_fp8"))
    g = GemmFp8(*g8.SPLIT_SHAPE, cruncher=c2, fill="none")
    want = _set_codes(g, g8.fp8_nonfinite(g8.SPLIT_SHAPE))
    for _ in range(2):
        g.C.array[:] = 1.0
        g.run(resident=False)
        r = c2.ranges(1)
        assert len(r) == 2 and sum(r) == g.global_range and min(r) > 0, r
        go.assert_nonfinite(g.result(download=False), want)
    c2.dispose()


@pytest.mark.parametrize("shape", g8.CLASS_SHAPES)
@pytest.mark.parametrize("tile", sorted(FP8_TILES))
def test_wide_groups_as_measured(cr, tile, shape):
    """±448 among small integers: the kernels return what the matrix core's
    14-bit sum over 8 neighbouring k gives (gemm8_oracles.emu_group_sums, the
    rule measured with single instructions, composed over K), element for
    element, with both instructions: not the integer product, and nothing
    else either.  GemmFp8's docstring and docs/API.md state the rule;
    test_gpu_gemm_mxfp8.py::test_probe_adjacent_k_sum_is_exact is the IEEE twin."""
    a, b, want, exact = g8.wide_groups(shape)
    g = GemmFp8(*shape, cruncher=cr, tile=tile, fill="none")
    g.A.array[:] = a.ravel()
    g.B.array[:] = b.ravel()
    g.C.array[:] = np.nan
    g.run(resident=True)
    _assert_exact(g.result(), want)
