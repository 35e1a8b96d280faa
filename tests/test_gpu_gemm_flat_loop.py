"""The flat K loops of the bf16 ping-pong GEMM (kernels/sgemm_bf16.hip, FLAT)
against their reference tile 256x256pb0, the loop written once for both wave
groups: the same barriers, waits and MFMA order, so C must be the same to the
bit, call after call.

Shapes: one 256² tile at K = 64·n, n = 1…8 — the prologue with one and two
K-tiles, every phase of the A (2) × Bt (3) buffer rotation and the peeled last
K-tiles of both groups (G0 peels one, G1 two) — and 512 × 768 × 448 at
group_m 2, six tiles in grouped order."""
import functools
import itertools

import numpy as np
import pytest

import cekirdekler_amd as ck
import gemm_oracles as go
from cekirdekler_amd.ops.gemm import GemmBf16, from_bf16_bits, to_bf16_bits
from cekirdekler_amd.ops.library import library

pytestmark = pytest.mark.gpu

REFERENCE_TILE = "256x256pb0"
FLAT_TILES = ["256x256pb", "256x256pbr"]  # every kernel built with the flat loops
CASES = [((256, 256, 64 * n), 4) for n in range(1, 9)] + [((512, 768, 448), 2)]  # (shape, group_m)
RUNS = 3

_ids = itertools.count(400)  # a compute id of its own per GEMM object


@pytest.fixture(scope="module")
def cr():
    c = ck.ClNumberCruncher(ck.ClPlatforms.all().gpus()[0], "", prebuilt=library("sgemm_bf16"))
    yield c
    c.dispose()


@functools.lru_cache(maxsize=None)
def uniform(shape):
    """bf16-representable uniform [-1, 1) operands (a [M][K], b [N][K]), frozen."""
    M, N, K = shape
    rng = np.random.default_rng(sum(shape))
    ops = [from_bf16_bits(to_bf16_bits(rng.uniform(-1, 1, (r, K)).astype(np.float32))).reshape(r, K) for r in (M, N)]
    for x in ops:
        x.setflags(write=False)
    return ops


def calls(cr, tile, shape, group_m, a, b, runs):
    """`runs` resident calls of one GEMM object on a and b, each with C full
    of NaN on the device beforehand: per call (raw device C, C by rows)."""
    g = GemmBf16(*shape, cruncher=cr, tile=tile, group_m=group_m, fill="none")
    g.cid = next(_ids)
    try:
        g.A.array[:] = to_bf16_bits(a).ravel()
        g.B.array[:] = to_bf16_bits(b).ravel()
        out = []
        for _ in range(runs):
            g.C.array[:] = np.nan
            g.C.read = True
            try:
                g.run(compute_id=g.cid, resident=True)
            finally:
                g.C.read = False
            rows = g.result(download=True)
            out.append((g.C.array.copy(), rows))
        return out
    finally:
        for arr in (g.A, g.B, g.C, g.dims, *g.extra):
            arr.dispose()


_reference = {}


def reference(cr, shape, group_m):
    """The reference tile's C on the uniform operands, computed once per shape."""
    if shape not in _reference:
        (raw, rows), = calls(cr, REFERENCE_TILE, shape, group_m, *uniform(shape), 1)
        assert not np.isnan(raw).any()
        for x in (raw, rows):
            x.setflags(write=False)
        _reference[shape] = raw, rows
    return _reference[shape]


@pytest.mark.parametrize("shape,group_m", CASES)
@pytest.mark.parametrize("tile", FLAT_TILES)
def test_c_equals_reference_tile_bit_for_bit(cr, tile, shape, group_m):
    """Uniform [-1, 1) data, three calls: the raw device C equals that of
    256x256pb0 bit for bit (the row-major tile: both brought to rows)."""
    want_raw, want_rows = reference(cr, shape, group_m)
    for n, (raw, rows) in enumerate(calls(cr, tile, shape, group_m, *uniform(shape), RUNS)):
        if tile == "256x256pbr":
            assert np.array_equal(rows, want_rows), f"call {n}: {int((rows != want_rows).sum())} elements differ"
        else:
            assert np.array_equal(raw, want_raw), f"call {n}: {int((raw != want_raw).sum())} elements differ"


@pytest.mark.parametrize("shape,group_m", CASES)
@pytest.mark.parametrize("tile", FLAT_TILES + [REFERENCE_TILE])
def test_exact_integers(cr, tile, shape, group_m):
    """Integers in [-8, 8]: C equals the int64 product element for element
    (the reference tile too: it is no member of TILES, so the oracles that
    run over every tile do not reach it)."""
    a, b, want = go.exact_integers(shape)
    (_, rows), = calls(cr, tile, shape, group_m, a, b, 1)
    go.assert_exact(rows, want)


@pytest.mark.parametrize("tile", FLAT_TILES)
def test_second_resident_call(cr, tile):
    """resident=True twice on one object (operands stay on the device, C is
    NaN before each call): both launches give the exact product."""
    shape = (512, 768, 448)
    a, b, want = go.exact_integers(shape)
    for _, rows in calls(cr, tile, shape, 2, a, b, 2):
        go.assert_exact(rows, want)
