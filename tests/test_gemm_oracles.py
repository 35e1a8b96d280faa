"""CPU tier for tests/gemm_oracles.py: honest emulators of the bf16 and fp32
GEMM kernels pass every case at every shape the GPU tier runs, and each
subtly wrong kernel (mutant) is rejected by the case named beside it."""
import numpy as np
import pytest

import gemm_oracles as go
from cekirdekler_amd.ops import gemm

BF16_ALL = go.BF16_SHAPES + go.BF16_SMALL_TILE_SHAPES + [go.bf16_multi("256x256pbw")]
SPLIT_SHAPE = lambda K: (*go.SPLIT_MN, K)  # noqa: E731


def _bf16_layout(c, shape, group_m=2, mutate=None):
    """An emulated C through the fragment-ordered tile-major buffer and back."""
    tile = "128x128" if shape[0] % 256 or shape[1] % 256 else "256x256pb"
    BM, BN = gemm.TILES[tile][:2]
    return go.through_device_layout(c, BM, BN, gemm.TILE_WAVES[tile], group_m, mutate)


def _f32_layout(c, group_m=2, mutate=None):
    return go.through_device_layout(c, 256, 256, None, group_m, mutate)


def _run_case(case, shape, fmt, kernel):
    a, b, want = go.build(case, shape, fmt)
    return go.check(case, kernel(a, b), a, b, want, fmt)


def _rejects(case, shape, fmt, kernel):
    try:
        _run_case(case, shape, fmt, kernel)
    except AssertionError:
        return True
    return False


# --------------------------------------------------------------------------- honest kernels

@pytest.mark.parametrize("shape", BF16_ALL)
def test_honest_bf16_emulator_passes_every_exact_case(shape):
    for case in go.EXACT_CASES:
        _run_case(case, shape, "bf16", lambda a, b: _bf16_layout(go.emu_chunked(a, b), shape))


@pytest.mark.parametrize("shape", go.F32_SHAPES)
def test_honest_f32_emulator_passes_every_exact_case(shape):
    for case in go.EXACT_CASES:
        _run_case(case, shape, "f32", lambda a, b: _f32_layout(go.emu_chain_f32(a, b)))


@pytest.mark.parametrize("shape", [go.HOST_SHAPE, go.BF16_RANDOM, go.F32_RANDOM])
def test_honest_emulators_pass_exact_integers_at_the_other_shapes(shape):
    """The shapes of the host-resident paths and of the random-data case."""
    _run_case("exact_integers", shape, "bf16", lambda a, b: _bf16_layout(go.emu_chunked(a, b), shape))
    _run_case("exact_integers", shape, "f32", lambda a, b: _f32_layout(go.emu_chain_f32(a, b)))


@pytest.mark.parametrize("K,S", go.SPLIT_K_CASES)
def test_honest_split_k_emulator_passes(K, S):
    for case in ("exact_integers", "wide_integers", "nonfinite"):
        _run_case(case, SPLIT_SHAPE(K), "bf16", lambda a, b: _bf16_layout(go.emu_split_k(a, b, S), SPLIT_SHAPE(K)))


@pytest.mark.parametrize("K", go.HANDOVER_K)
@pytest.mark.parametrize("tile", sorted(gemm.EXCHANGE_TILES))
def test_honest_handover_emulator_passes(tile, K):
    helper, owner = go.handover_ktiles(tile, K)
    assert helper >= 1 and helper + owner == K // 64
    for case in ("exact_integers", "wide_integers", "nonfinite"):
        _run_case(case, SPLIT_SHAPE(K), "bf16",
                  lambda a, b: _bf16_layout(go.emu_handover(a, b, helper), SPLIT_SHAPE(K)))


def test_handover_splits_are_the_designed_ones():
    got = {t: [go.handover_ktiles(t, K) for K in go.HANDOVER_K] for t in gemm.EXCHANGE_TILES}
    assert got["256x256pbw"] == got["256x256pbh"] == [(1, 1), (1, 3), (1, 9), (4, 12)]
    assert got["256x256pbs"] == [(1, 1), (2, 2), (5, 5), (8, 8)]
    for t in gemm.EXCHANGE_TILES:  # what GemmBf16.__init__ stores in dims[5]
        for K in go.HANDOVER_K:
            helper, owner = go.handover_ktiles(t, K)
            assert (owner - helper) // 2 == max(0, min(gemm.EXCHANGE_SHIFT[t], K // 128 - 1))


def test_honest_emulators_within_the_derived_bounds(capsys):
    """The worst err / bound of every honest structure on the random-data
    case (the figures of profiles/gemm_oracles.md's emulator column)."""
    a, b, ref = go.build("row_scaled_random", go.BF16_RANDOM, "bf16")
    bound = go.accumulation_bound(a, b, go.UNIT_BF16)
    kernels = {"bf16 32-deep chunks": lambda: go.emu_chunked(a, b),
               "bf16 split-K 2": lambda: go.emu_split_k(a, b, 2), "bf16 split-K 4": lambda: go.emu_split_k(a, b, 4),
               "bf16 hand-over 1/7 K-tiles": lambda: go.emu_handover(a, b, go.handover_ktiles("256x256pbw", 512)[0]),
               "bf16 hand-over 4/4 K-tiles": lambda: go.emu_handover(a, b, go.handover_ktiles("256x256pbs", 512)[0]),
               "bf16 k-ordered chain": lambda: go.emu_chain_f32(a, b)}
    ratios = {}
    for name, k in kernels.items():
        ratios[name] = go.check_within_bound(_bf16_layout(k(), go.BF16_RANDOM), ref, bound, name)
    a, b, ref = go.build("row_scaled_random", go.F32_RANDOM, "f32")
    ratios["f32 k-ordered chain"] = go.check_within_bound(_f32_layout(go.emu_chain_f32(a, b)), ref,
                                                         go.accumulation_bound(a, b, go.UNIT_F32), "f32")
    with capsys.disabled():
        for name, r in ratios.items():
            print(f"\n  honest {name}: worst err / bound = {r:.3e}", end="")
    assert 0 < max(ratios.values()) <= 1.0, ratios


# --------------------------------------------------------------------------- wrong kernels

def _r16(x):
    return go.round_mantissa(x, 16)


def _r7(x):
    return go.round_mantissa(x, 7)


def _flush(x):
    return np.where(np.abs(x) < 2.0 ** -126, 0.0, x)


def _kxor1(a, b):
    return go.emu_chunked(a, b[:, np.arange(b.shape[1]) ^ 1])


def _ktile0_twice(a, b):
    a2, b2 = a.copy(), b.copy()
    a2[:, -64:], b2[:, -64:] = a[:, :64], b[:, :64]
    return go.emu_chunked(a2, b2)


def _k_dropped(a, b):
    a2 = a.copy()
    a2[:, 77] = 0
    return go.emu_chunked(a2, b)


def _frag_transposed(buf):
    f = buf.reshape(-1, 4, 16, 4)                                   # fq fr r: row fq·4 + r, column fr
    m = f.transpose(0, 1, 3, 2).reshape(-1, 16, 16).transpose(0, 2, 1)  # [row][col], swapped
    return np.ascontiguousarray(m.reshape(-1, 4, 4, 16).transpose(0, 1, 3, 2)).reshape(-1)


def _frags_exchanged(buf):
    buf[:256], buf[256:512] = buf[256:512].copy(), buf[:256].copy()
    return buf


def _tile_unwritten(buf):
    buf[-256 * 256:] = np.nan  # the NaN the host C was filled with
    return buf


def _nan_leak(a, b):
    c = go.emu_chunked(a, b)
    c[a.shape[0] - 6 + 1, 17] = np.nan  # the row below the NaN row
    return c


def _small_row_scaled(emu):
    def kernel(a, b):
        c = emu(a, b)
        c[np.abs(a).max(axis=1).argmin()] *= np.float32(1.001)
        return c
    return kernel


M3 = go.BF16_MULTI
S3 = SPLIT_SHAPE(384)
# mutant -> (fmt, kernel, the cases that must reject it, shape)
MUTANTS = {
    "f32 operands truncated to a 10-bit mantissa": (
        "f32", lambda a, b: go.emu_chain_f32(go.trunc_mantissa(a, 10), go.trunc_mantissa(b, 10)),
        ["k_pairing", "row_scaled_random"], go.F32_RANDOM),
    "f32 operands rounded to bf16": (
        "f32", lambda a, b: go.emu_chain_f32(_r7(a), _r7(b)), ["k_pairing", "row_scaled_random"], go.F32_RANDOM),
    "accumulator rounded to a 16-bit mantissa after every K-tile": (
        "bf16", lambda a, b: go.emu_chunked(a, b, after_ktile=_r16), ["wide_integers"], M3),
    "accumulator rounded to bf16 after every K-tile": (
        "bf16", lambda a, b: go.emu_chunked(a, b, after_ktile=_r7), ["wide_integers"], M3),
    "f32 accumulator rounded to a 16-bit mantissa after every K-tile": (
        "f32", lambda a, b: go.emu_chunked(a, b, chunk=1, ktile=32, after_ktile=_r16), ["wide_integers"], go.F32_MULTI),
    "split-K partial rounded to a 16-bit mantissa": (
        "bf16", lambda a, b: go.emu_split_k(a, b, 2, partial=_r16), ["wide_integers"], S3),
    "split-K partial rounded to bf16": (
        "bf16", lambda a, b: go.emu_split_k(a, b, 2, partial=_r7), ["wide_integers"], S3),
    "hand-over partial rounded to a 16-bit mantissa": (
        "bf16", lambda a, b: go.emu_handover(a, b, 1, partial=_r16), ["wide_integers"], SPLIT_SHAPE(256)),
    "one k dropped": ("bf16", _k_dropped, ["exact_integers"], M3),
    "K-tile 0 used twice and the last one skipped": ("bf16", _ktile0_twice, ["exact_integers", "wide_integers"], M3),
    "A's k paired with k^1 of B": ("bf16", _kxor1, ["k_pairing"], M3),
    "C stored with row and column swapped inside a 16x16 fragment": (
        "bf16", lambda a, b: _bf16_layout(go.emu_chunked(a, b), M3, mutate=_frag_transposed), ["k_pairing"], M3),
    "two fragments exchanged": (
        "bf16", lambda a, b: _bf16_layout(go.emu_chunked(a, b), M3, mutate=_frags_exchanged),
        ["k_pairing", "exact_integers"], M3),
    "one tile left unwritten": (
        "bf16", lambda a, b: _bf16_layout(go.emu_chunked(a, b), M3, mutate=_tile_unwritten),
        ["exact_integers", "row_scaled_random"], M3),
    "f32 one tile left unwritten": (
        "f32", lambda a, b: _f32_layout(go.emu_chain_f32(a, b), mutate=_tile_unwritten), ["exact_integers"], go.F32_MULTI),
    "NaN leaking into a neighbouring row": ("bf16", _nan_leak, ["nonfinite"], M3),
    "bf16 subnormal inputs flushed": (
        "bf16", lambda a, b: go.emu_chunked(_flush(a), _flush(b)), ["range_subnormal"], M3),
    "f32 subnormal inputs flushed": (
        "f32", lambda a, b: go.emu_chain_f32(_flush(a), _flush(b)), ["range_subnormal"], go.F32_MULTI),
    "bf16 a row of small magnitude multiplied by 1.001": (
        "bf16", _small_row_scaled(go.emu_chunked), ["row_scaled_random"], go.BF16_RANDOM),
    "f32 a row of small magnitude multiplied by 1.001": (
        "f32", _small_row_scaled(go.emu_chain_f32), ["row_scaled_random"], go.F32_RANDOM),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutant_is_rejected_by_its_named_cases(mutant):
    fmt, kernel, cases, shape = MUTANTS[mutant]
    for case in cases:
        assert _rejects(case, shape, fmt, kernel), f"{mutant!r} passes {case} at {shape}"


def test_what_the_old_fp32_formula_lets_through():
    """test_gemm_f32_matches_fp64's max-norm formula at (512, 512, 256), on
    its own operands (seed 0): operands truncated to a 10-bit mantissa pass it
    (max error 1.9e-2 against a tolerance of 3.9e-2) and sit far beyond the
    per-element bound; on row-scaled data a small row times 1.001 passes it
    too.  Operands rounded to bf16 were expected to pass as well; measured,
    they miss it by 1.3x (5.0e-2 against 3.9e-2, 56x the per-element bound),
    so that is what is asserted for them: the old tolerance sits between an
    11-bit and an 8-bit operand format."""
    shape = go.F32_RANDOM
    K = shape[2]
    a, b, ref = go.old_uniform_case(shape)
    bound = go.accumulation_bound(a, b, go.UNIT_F32)
    honest = go.emu_chain_f32(a, b)
    assert go.old_f32_formula_passes(honest, ref, K)
    assert go.check_within_bound(honest, ref, bound) <= 1.0
    tol = 1e-4 * np.sqrt(K) * max(1.0, np.abs(ref).max())
    for name, f, passes_old in (("trunc10", lambda x: go.trunc_mantissa(x, 10), True), ("bf16", _r7, False)):
        c = go.emu_chain_f32(f(a), f(b))
        err = np.abs(c - ref)
        print(f"{name}: max error {err.max():.3e}, old tolerance {tol:.3e}, err / new bound {(err / bound).max():.1f}")
        assert go.old_f32_formula_passes(c, ref, K) == passes_old
        with pytest.raises(AssertionError):
            go.check_within_bound(c, ref, bound)
    a, b, ref = go.build("row_scaled_random", shape, "f32")
    c = _small_row_scaled(go.emu_chain_f32)(a, b)
    assert go.old_f32_formula_passes(c, ref, K)
    with pytest.raises(AssertionError):
        go.check_within_bound(c, ref, go.accumulation_bound(a, b, go.UNIT_F32))


# --------------------------------------------------------------------------- layout and coverage

@pytest.mark.parametrize("tile", sorted(gemm.TILE_WAVES))
@pytest.mark.parametrize("group_m", [1, 2, 4])
def test_layout_round_trip_is_the_identity(tile, group_m):
    BM, BN = gemm.TILES[tile][:2]
    c = np.arange(768 * 512, dtype=np.float32).reshape(768, 512)
    got = go.through_device_layout(c, BM, BN, gemm.TILE_WAVES[tile], group_m)
    assert np.array_equal(got, c)
    assert np.array_equal(go.through_device_layout(c, BM, BN, None, group_m), c)


def test_gpu_tier_runs_every_tile():
    """Every TILES and F32_TILES name is in the GPU tier's parameter lists,
    with every shape it can run, so a tile added later cannot go untested."""
    import test_gpu_gemm_oracles as gpu

    assert sorted({t for t, _, _ in gpu.BF16_TILE_SHAPES}) == sorted(gemm.TILES)
    assert sorted({t for t, _ in gpu.F32_TILE_SHAPES}) == sorted(gemm.F32_TILES)
    assert sorted(gpu.BF16_TILE_NAMES) == sorted(gemm.TILES) and sorted(gpu.F32_TILE_NAMES) == sorted(gemm.F32_TILES)
    for t in gemm.TILES:
        assert {s for tt, s, _ in gpu.BF16_TILE_SHAPES if tt == t} == set(go.bf16_shapes(t))
    for t in gemm.F32_TILES:
        assert [s for tt, s in gpu.F32_TILE_SHAPES if tt == t] == go.f32_shapes(t) != []
    assert sorted({t for t, _, _ in gpu.SPLIT_CASES}) == sorted(gemm.SPLIT_K_TILES)
    assert sorted({t for t, _, _ in gpu.HANDOVER_CASES}) == sorted(gemm.EXCHANGE_TILES)
