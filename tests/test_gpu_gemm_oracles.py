"""GPU tier of the bf16 and fp32 GEMM oracles (kernels/sgemm_bf16.hip,
kernels/sgemm_f32.hip; tests/gemm_oracles.py): every tile on exact data first
(integers, integers that need all 24 bits, a k-pairing probe, the ends of the
number range, non-finite inputs), compared with ==, then row-scaled random
data against the derived per-element bound; the split-K and hand-over tiles
at several K, on one and two logical devices and through their forced
fall-backs; the host-resident paths.  The CPU tier (test_gemm_oracles.py)
shows that these comparisons reject wrong kernels."""
import contextlib
import itertools

import numpy as np
import pytest

import cekirdekler_amd as ck
import gemm_oracles as go
from cekirdekler_amd.ops.gemm import (EXCHANGE_TILES, F32_TILES, SPLIT_K_TILES, TILES, GemmBf16, GemmF32,
                                      from_bf16_bits, to_bf16_bits)
from cekirdekler_amd.ops.library import library

pytestmark = pytest.mark.gpu

# what the tests below are parametrised over (test_gemm_oracles.py checks
# these lists against the tile dictionaries of ops/gemm.py)
BF16_TILE_NAMES = sorted(TILES)
F32_TILE_NAMES = sorted(F32_TILES)
# (tile, shape, group_m): every shape at group_m 2, the three-tile-row shape with the default 4 too
BF16_TILE_SHAPES = [(t, s, gm) for t in BF16_TILE_NAMES for s in go.bf16_shapes(t)
                    for gm in ((2, 4) if s == go.BF16_GROUPED_SHAPE else (2,))]
F32_TILE_SHAPES = [(t, s) for t in F32_TILE_NAMES for s in go.f32_shapes(t)]
ONE_SHAPE_CASES = [c for c in go.EXACT_CASES if c != "exact_integers"]
SPLIT_CASES = [(t, K, S) for t in sorted(SPLIT_K_TILES) for K, S in go.SPLIT_K_CASES]
# (tile, K, handover_spin_limit): 0 the designed wait, -1 the owner claims at
# once, -2 (tiles with a hand-back) the helper claims the hand-back at once
HANDOVER_CASES = [(t, K, lim) for t in sorted(EXCHANGE_TILES) for K in go.HANDOVER_K
                  for lim in ((0, -1) if t == "256x256pbw" else (0, -1, -2))]
CALLS = 4  # consecutive calls per split-K / hand-over object: the re-armed counters are used

_ids = itertools.count(10)  # a compute id of its own per GEMM object


@pytest.fixture(scope="module")
def crunchers():
    """One cruncher per (library, number of logical devices), made on first
    use; of two logical devices the second is made slower."""
    made = {}

    def get(lib, devices=1):
        if (lib, devices) not in made:
            g = ck.ClPlatforms.all().gpus()[0]
            cr = ck.ClNumberCruncher(g if devices == 1 else g + g, "", prebuilt=library(lib))
            if devices == 2:
                cr.set_time_scale(1, 2.0)
            made[lib, devices] = cr
        return made[lib, devices]

    yield get
    for cr in made.values():
        cr.dispose()


@contextlib.contextmanager
def _gemm(fmt, cr, shape, a, b, **kw):
    """A GEMM object on `cr` holding exactly the operands a and b, with a
    compute id of its own; its arrays leave the devices at the end."""
    g = (GemmBf16 if fmt == "bf16" else GemmF32)(*shape, cruncher=cr, fill="none", **kw)
    g.cid = next(_ids)
    try:
        if fmt == "bf16":
            g.A.array[:] = to_bf16_bits(a).ravel()
            g.B.array[:] = to_bf16_bits(b).ravel()
            assert np.array_equal(from_bf16_bits(g.A.array), a.ravel(), equal_nan=True)
            assert np.array_equal(from_bf16_bits(g.B.array), b.ravel(), equal_nan=True)
        else:
            g.A.array[:] = a.ravel()
            g.B.array[:] = b.ravel()
        yield g
    finally:
        for arr in (g.A, g.B, g.C, g.dims, *g.extra):
            arr.dispose()


def _run(g, resident=True, nan_on_device=True, **kw):
    """One call with the host C full of NaN; `nan_on_device` sends that C to
    the devices first, so an element no work-group writes comes back NaN
    whatever the device memory held."""
    g.C.array[:] = np.nan
    g.C.read = nan_on_device
    try:
        g.run(compute_id=g.cid, resident=resident, **kw)
    finally:
        g.C.read = False
    return g.result(download=resident)


def _case(fmt, cr, tile, case, shape, resident=True, **kw):
    a, b, want = go.build(case, shape, fmt)
    with _gemm(fmt, cr, shape, a, b, tile=tile, **kw) as g:
        return go.check(case, _run(g, resident), a, b, want, fmt)


# --------------------------------------------------------------------------- every bf16 tile

@pytest.mark.parametrize("tile,shape,group_m", BF16_TILE_SHAPES)
def test_bf16_exact_integers(crunchers, tile, shape, group_m):
    """C equals the int64 product bit for bit, at K-tile counts 1, 2, 3, 5 and
    16 and with a short last tile group (768 rows)."""
    _case("bf16", crunchers("sgemm_bf16"), tile, "exact_integers", shape, group_m=group_m)


@pytest.mark.parametrize("case", ONE_SHAPE_CASES)
@pytest.mark.parametrize("tile", BF16_TILE_NAMES)
def test_bf16_exact_case(crunchers, tile, case):
    """wide_integers: no accumulator or workspace narrower than fp32;
    k_pairing: A's k meets the same k of B and C is stored the right way
    round; range_large / range_subnormal: the exact IEEE value at both ends of
    the range (bf16 subnormal inputs are not flushed); nonfinite: Inf and NaN
    stay in their own rows."""
    _case("bf16", crunchers("sgemm_bf16"), tile, case, go.bf16_multi(tile), group_m=2)


@pytest.mark.parametrize("tile", BF16_TILE_NAMES)
def test_bf16_row_scaled_random_within_derived_bound(crunchers, tile):
    """|C - ref| <= K · 2^-23 · Σ|a·b| element by element, on rows whose
    magnitudes span 2^-20 … 2^20 (go.accumulation_bound)."""
    ratio = _case("bf16", crunchers("sgemm_bf16"), tile, "row_scaled_random", go.BF16_RANDOM)
    print(f"bf16 {tile} {go.BF16_RANDOM}: worst |C-ref|/bound = {ratio:.3e}")
    assert ratio <= 1.0


# --------------------------------------------------------------------------- every fp32 tile

@pytest.mark.parametrize("tile,shape", F32_TILE_SHAPES)
def test_f32_exact_integers(crunchers, tile, shape):
    _case("f32", crunchers("sgemm_f32"), tile, "exact_integers", shape, group_m=2)


@pytest.mark.parametrize("case", ONE_SHAPE_CASES)
@pytest.mark.parametrize("tile", F32_TILE_NAMES)
def test_f32_exact_case(crunchers, tile, case):
    """As test_bf16_exact_case; k_pairing's B uses all 24 mantissa bits, so an
    operand truncated or rounded on its way to the matrix core fails here."""
    _case("f32", crunchers("sgemm_f32"), tile, case, go.F32_MULTI, group_m=2)


@pytest.mark.parametrize("tile", F32_TILE_NAMES)
def test_f32_row_scaled_random_within_derived_bound(crunchers, tile):
    """|C - ref| <= K · 2^-24 · Σ|a·b| element by element: a k-ordered fp32
    fma chain, one rounding per step (go.accumulation_bound).  Operands of a
    TF32-like format are 18x beyond it at this shape (CPU tier)."""
    ratio = _case("f32", crunchers("sgemm_f32"), tile, "row_scaled_random", go.F32_RANDOM)
    print(f"f32 {tile} {go.F32_RANDOM}: worst |C-ref|/bound = {ratio:.3e}")
    assert ratio <= 1.0


# --------------------------------------------------------------------------- split-K

@pytest.mark.parametrize("case", ["exact_integers", "wide_integers", "nonfinite"])
@pytest.mark.parametrize("devices", [1, 2])
@pytest.mark.parametrize("tile,K,S", SPLIT_CASES)
def test_split_k(crunchers, tile, K, S, devices, case):
    """1, 3, 4 and 8 K-tiles per split, four consecutive calls per object (the
    arrival counters re-arm), the K-splits of a tile kept on one device.  The
    fp32 partial tiles hold wide_integers exactly; nonfinite has its Inf in
    the first split's K-range and its NaN in the last one's."""
    cr = crunchers("sgemm_bf16", devices)
    shape = (*go.SPLIT_MN, K)
    a, b, want = go.build(case, shape, "bf16")
    with _gemm("bf16", cr, shape, a, b, tile=tile, split_k=S, group_m=2) as g:
        for _ in range(CALLS):
            go.check(case, _run(g, resident=False), a, b, want, "bf16")
        r = cr.ranges(g.cid)
        assert len(r) == devices and sum(r) == g.global_range and all(x % (g.L * S) == 0 for x in r), r
        for dev in range(devices):
            cr.download(g.counters, dev)
            assert not g.counters.array.any()


# --------------------------------------------------------------------------- hand-over tiles

@pytest.mark.parametrize("case,devices", [("exact_integers", 1), ("exact_integers", 2), ("wide_integers", 1),
                                          ("nonfinite", 1)])
@pytest.mark.parametrize("tile,K,limit", HANDOVER_CASES)
def test_handover(crunchers, tile, K, limit, case, devices):
    """Helper/owner K-tiles (1,1), (1,3), (1,9), (4,12) (even split: (1,1),
    (2,2), (5,5), (8,8)), through the hand-over and through both forced
    fall-backs, in which one side multiplies the other's K-range itself.  At
    -1 every owner must fall back even when the helper has one K-tile (the
    helper waits for the claim: it once published first, 23 of 24)."""
    cr = crunchers("sgemm_bf16", devices)
    shape = (*go.SPLIT_MN, K)
    a, b, want = go.build(case, shape, "bf16")
    with _gemm("bf16", cr, shape, a, b, tile=tile, group_m=2, handover_spin_limit=limit) as g:
        assert g.split_k == 2 and (K // 128 - g.exchange_shift, K // 128 + g.exchange_shift) == go.handover_ktiles(tile, K)
        for _ in range(CALLS):
            go.check(case, _run(g, resident=False), a, b, want, "bf16")
        fb = g.handover_fallbacks()
        if limit == 0:
            assert fb == 0, fb
        if limit == -1:
            assert fb == CALLS * g.tiles, fb  # every owner of every call fell back
        for dev in range(devices):  # re-armed: only the fall-back counter is nonzero
            cr.download(g.counters, dev)
            assert not g.counters.array[:-1].any()
        r = cr.ranges(g.cid)
        assert sum(r) == g.global_range and all(x % (2 * g.L) == 0 for x in r), r


# --------------------------------------------------------------------------- other paths

HOST_SHAPE = go.HOST_SHAPE


@pytest.mark.parametrize("fmt,tile", [("bf16", "256x256pb"), ("f32", "256x256g8i")])
def test_host_resident_run_is_exact(crunchers, fmt, tile):
    a, b, want = go.build("exact_integers", HOST_SHAPE, fmt)
    with _gemm(fmt, crunchers("sgemm_" + fmt), HOST_SHAPE, a, b, tile=tile) as g:
        go.assert_exact(_run(g, resident=False), want)
        err, checked = g.verify_full(g.cid, host=True)
        assert checked == g.tiles and err == 0.0, (err, checked)
        assert g.verify(g.cid, host=True) == 0.0


@pytest.mark.parametrize("fmt,tile", [("bf16", "256x256pb"), ("f32", "256x256g8i")])
def test_host_resident_streamed_blobs_are_exact(crunchers, fmt, tile):
    """Four blobs, one tile group (A row panel) each: the event pipeline."""
    cr = crunchers("sgemm_" + fmt)
    a, b, want = go.build("exact_integers", HOST_SHAPE, fmt)
    with _gemm(fmt, cr, HOST_SHAPE, a, b, tile=tile, group_m=1) as g:
        assert g.can_stream()
        go.assert_exact(_run(g, resident=False, nan_on_device=False, stream_blobs=4), want)
        assert cr.last_record()["pipelined"]


@pytest.mark.parametrize("fmt,tile", [("bf16", "256x256pb"), ("bf16", "256x256pbr"), ("f32", "256x256g8i")])
def test_resident_verify_reports_zero_on_exact_data(crunchers, fmt, tile):
    a, b, want = go.build("exact_integers", HOST_SHAPE, fmt)
    with _gemm(fmt, crunchers("sgemm_" + fmt), HOST_SHAPE, a, b, tile=tile) as g:
        go.assert_exact(_run(g), want)
        err, checked = g.verify_full(g.cid)
        assert checked == g.tiles and err == 0.0, (err, checked)
        assert g.verify(g.cid) == 0.0


def test_aux_bf16_codec_on_gpu():
    """cek_f32_to_bf16 / cek_bf16_to_f32 on the GPU over the inputs of the
    CPU tier (NaNs of every kind, ±Inf, the largest finite values, every tie
    of a binade, subnormals, 200 000 random patterns), one launch each way."""
    from test_gemm_host import bf16_aux_codec_case

    bf16_aux_codec_case(ck.ClPlatforms.all().gpus()[0])
