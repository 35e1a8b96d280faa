"""CPU tier for tests/gemm8_oracles.py: an honest emulation of the fp8 and
MXFP8 GEMMs passes every case, each named wrong behaviour is rejected in every
element it affects, the ragged tile groups reach the branch they are meant
for, and the single-instruction probe cross-compiles for gfx950."""
import numpy as np
import pytest

import gemm8_oracles as g8
import gemm_oracles as go
from cekirdekler_amd import cek
from cekirdekler_amd.ops import gemm

SMALL, MULTI = g8.CLASS_SHAPES


def _rejects(c, want):
    try:
        go.assert_nonfinite(c, want)
    except AssertionError:
        return True
    return False


def _differs(c, want):
    """Elements of c that the comparison of assert_nonfinite counts wrong."""
    cls, expected = want
    fin = cls == go.FINITE
    return (go.classify(c) != cls) | (fin & (np.where(fin, c, 0).astype(np.float64) != expected))


# --------------------------------------------------------------------------- honest kernels

@pytest.mark.parametrize("shape", g8.CLASS_SHAPES)
def test_honest_emulator_passes_the_class_cases(shape):
    cases = [g8.fp8_nonfinite(shape), g8.mx_nonfinite(shape)] + [g8.mx_scale_ends(shape, k)
                                                                 for k in g8.SCALE_END_KINDS[:3]]
    for a, b, sa, sb, want in cases:
        go.assert_nonfinite(g8.emu_gemm8(a, b, sa, sb), want)


@pytest.mark.parametrize("shape", g8.UNDERFLOW_SHAPES)
def test_honest_emulator_passes_the_underflow_cases(shape):
    for kind in ("underflow", "underflow_zero"):
        a, b, sa, sb, want = g8.mx_scale_ends(shape, kind)
        c = g8.emu_gemm8(a, b, sa, sb)
        go.assert_nonfinite(c, want)
        assert (c != 0).mean() > 0.9 if kind == "underflow" else not c.any()


def test_builders_at_the_split_shape():
    """The builders' own assertions at the shape of the two-device tests: the
    NaN rows lie in the first and the last of four tile rows, the NaN column
    in the second tile column."""
    (m1, _), (m2, _), (n3, _), m4 = g8.nan_sites(g8.SPLIT_SHAPE)
    assert (m1 // 256, m2 // 256, m4 // 256, n3 // 256) == (0, 3, 0, 1)
    for build in (g8.fp8_nonfinite, g8.mx_nonfinite):
        cls = build(g8.SPLIT_SHAPE)[4][0]
        assert (cls[[m1, m2]] == go.NAN).all() and (cls[:, n3] == go.NAN).all()
    assert (g8.mx_nonfinite(g8.SPLIT_SHAPE)[4][0][m4] == go.NAN).all()


def test_nan_sites_are_in_different_fragments_waves_and_tiles():
    for shape in g8.CLASS_SHAPES + [g8.SPLIT_SHAPE]:
        (m1, k1), (m2, k2), (n3, k3), m4 = g8.nan_sites(shape)
        M, N, K = shape
        for BM, rows_per_wave in ((256, 128), (128, 64)):
            wave = lambda m: m % BM // rows_per_wave  # noqa: E731
            assert wave(m1) != wave(m2) and m1 % rows_per_wave // 16 != m2 % rows_per_wave // 16
        if M > 256:
            assert m1 // 256 != m2 // 256
        assert k1 // 128 == 0 and k2 // 128 == K // 128 - 1 and k3 // 128 == K // 128 // 2


# --------------------------------------------------------------------------- wrong behaviours

def test_nan_codes_read_as_480_are_rejected_everywhere():
    """An e4m3 without NaN holds ±480 at 0x7F / 0xFF: rows m1, m2 and column
    n3 come out finite, every one of their elements in the wrong class."""
    for a, b, sa, sb, want in (g8.fp8_nonfinite(MULTI), g8.mx_nonfinite(MULTI)):
        (m1, _), (m2, _), (n3, _), m4 = g8.nan_sites(MULTI)
        c = g8.emu_gemm8(a, b, sa, sb, nan_as_480=True)
        bad = _differs(c, want)
        rows = np.arange(MULTI[0]) != (m4 if sa is not None else -1)  # row m4 is NaN by its scale
        assert bad[[m1, m2]].all() and bad[rows, n3].all() and _rejects(c, want)
        assert not np.isnan(c[[m1, m2]]).any() and not np.isnan(c[rows, n3]).any()


def test_scale_byte_ff_read_as_2_to_128_is_rejected_in_all_of_row_m4():
    a, b, sa, sb, want = g8.mx_nonfinite(MULTI)
    _, _, (n3, _), m4 = g8.nan_sites(MULTI)
    c = g8.emu_gemm8(a, b, sa, sb, nan_as_128=True)
    cols = np.arange(MULTI[1]) != n3  # column n3 is NaN by Bt's element
    assert not np.isnan(c[m4][cols]).any() and _differs(c, want)[m4][cols].all()
    rest = np.ones(len(c), bool)
    rest[m4] = False
    assert not _differs(c, want)[rest].any()  # and nothing else changes


@pytest.mark.parametrize("kind", ["cancel_hi_lo", "cancel_lo_hi"])
def test_scales_applied_per_operand_in_fp32_are_rejected_everywhere(kind):
    """2^127 times any |x| >= 2 is beyond fp32: the operand under byte 254
    turns into ±Inf (and 0), and all of C into ±Inf or NaN.  The same with
    fp32 subnormals flushed on the way (the operand under byte 0 → 0)."""
    a, b, sa, sb, want = g8.mx_scale_ends(SMALL, kind)
    c = g8.emu_gemm8(a, b, sa, sb, operand_f32=True)
    assert _differs(c, want).all() and not np.isfinite(c).any()


def test_exponent_sums_wrapped_or_clamped_are_rejected():
    """Wrapped to 8 signed bits, 254 − 127 + 254 − 127 = 254 is −2 and
    −140 is 116; clamped to [−127, 127], 2^-18·2^227 stays finite and 2^-140
    becomes 2^-127."""
    a, b, sa, sb, want = g8.mx_scale_ends(MULTI, "overflow")
    m5, m6 = g8.overflow_sites(MULTI)
    big = np.arange(MULTI[1]) % 4 == 0
    c = g8.emu_gemm8(a, b, sa, sb, exp_sum=g8.wrap8)
    assert _differs(c, want)[[m5, m6]][:, big].all() and np.isfinite(c[[m5, m6]][:, big]).all()
    c = g8.emu_gemm8(a, b, sa, sb, exp_sum=g8.clamp8)
    assert _differs(c, want)[m6][big].all() and np.isfinite(c[m6]).all()
    for shape in g8.UNDERFLOW_SHAPES:
        a, b, sa, sb, want = g8.mx_scale_ends(shape, "underflow")
        nonzero = want[1] != 0
        for f in (g8.wrap8, g8.clamp8):
            assert _differs(g8.emu_gemm8(a, b, sa, sb, exp_sum=f), want)[nonzero].all()
        a, b, sa, sb, want = g8.mx_scale_ends(shape, "underflow_zero")
        c = g8.emu_gemm8(a, b, sa, sb, exp_sum=g8.clamp8)
        assert _differs(c, want)[c != 0].all() and (c != 0).mean() > 0.9


@pytest.mark.parametrize("shape", g8.UNDERFLOW_SHAPES)
def test_flushed_subnormal_results_are_rejected(shape):
    a, b, sa, sb, want = g8.mx_scale_ends(shape, "underflow")
    c = g8.emu_gemm8(a, b, sa, sb, flush=True)
    assert not c.any() and _differs(c, want)[want[1] != 0].all() and (want[1] != 0).mean() > 0.9


def test_nan_in_the_neighbouring_fragment_is_rejected():
    """The NaN row 16 rows off (the next fragment of the same wave): every
    element of both rows is wrong, but for the NaN column."""
    for a, b, sa, sb, want in (g8.fp8_nonfinite(MULTI), g8.mx_nonfinite(MULTI)):
        (m1, _), _, (n3, _), _ = g8.nan_sites(MULTI)
        c = g8.emu_gemm8(a, b, sa, sb).copy()
        c[[m1, m1 + 16]] = c[[m1 + 16, m1]]
        bad = _differs(c, want)
        cols = np.arange(MULTI[1]) != n3
        assert bad[m1][cols].all() and bad[m1 + 16][cols].all() and bad.sum() == 2 * cols.sum()


def test_a_leftover_nan_cannot_pass_for_a_computed_one():
    """What the GPU tests prefill C with (1.0) is in the wrong class in every
    NaN element, and wrong in every finite one but where the product is 1."""
    a, b, sa, sb, want = g8.fp8_nonfinite(SMALL)
    bad = _differs(np.ones(want[0].shape, np.float32), want)
    assert bad[want[0] == go.NAN].all() and bad.mean() > 0.98


# --------------------------------------------------------------------------- ragged tile groups

def test_ragged_groups_reach_the_short_last_group():
    """M / BM = 3: with group_m = 2 a full group, then a group of one tile
    row; with group_m = 4 one group of three.  Both are the gsz < group_m
    branch of tile_coords, and every tile is visited once."""
    for BM, cases in g8.RAGGED_GROUPS.items():
        for (M, N, K), gm in cases:
            ntm, ntn = M // BM, N // BM
            assert ntm % gm != 0
            tm, tn = gemm.tile_coords(np.arange(ntm * ntn), M, N, BM, BM, gm)
            assert sorted(zip(tm.tolist(), tn.tolist())) == [(r, c) for r in range(ntm) for c in range(ntn)]
            last = ntm // gm * gm  # first tile row of the short group
            assert (tm[last * ntn:] >= last).all() and (tm[:last * ntn] < last).all()
            plain = gemm.tile_coords(np.arange(ntm * ntn), M, N, BM, BM, 1)
            assert not np.array_equal(tm, plain[0])  # and the order is not the ungrouped one
        assert any(M // BM > gm for (M, _, _), gm in cases)  # a full group comes first


# --------------------------------------------------------------------------- the probe

def test_probe_kernel_cross_compiles_for_gfx950():
    ok, code, log = cek.compile_gpu(g8.PROBE_SRC, [], "gfx950")
    assert ok, log
    assert code[:4] == b"\x7fELF" and g8.PROBE_KERNEL.encode() in code


def test_probe_problems_ask_what_they_should():
    """Every question's expectation holds the classes it is about, and the
    report of an honest answer shows no difference."""
    pr = g8.probe_problems()
    assert (pr["baseline"][4][0] == go.FINITE).all() and (pr["baseline"][4][1] != 0).mean() > 0.9
    cls = pr["element_nan"][4][0]
    assert (cls[[3, 9]] == go.NAN).all() and (cls[:, 6] == go.NAN).all()
    cls = pr["scale_nan"][4][0]
    assert (cls[[4, 12]] == go.NAN).all() and (cls[:, 7] == go.NAN).all()
    cls, exp = pr["scale_sums"][4]
    assert set(cls[:8, :8].ravel()) == {go.POS_INF, go.NEG_INF} and (exp[:8, 8:] != 0).all() and (exp[8:, :8] != 0).all()
    names, A, Bt, SA, SB = g8.probe_buffers()
    assert A.size == Bt.size == 2048 * len(names) and SA.size == SB.size == 64 * len(names)
    for n in names:
        a, b, sa, sb, want, _ = pr[n]
        c = g8.emu_gemm8(a, b, sa, sb)
        go.assert_nonfinite(c, want)
        assert "0 finite values differ" in g8.probe_report(n, c)


# --------------------------------------------------------------------------- the measured 14-bit group sum

def test_group_sum_emulator_cuts_only_what_lies_14_bits_below_a_neighbour():
    """On the integer data of the exact cases the measured rule changes
    nothing; on wide_groups it misses the integer product in most elements,
    by less than 8 per group of 8 k; and the probe's adjacent_k question is the
    rule at its smallest."""
    a, b, _, _, (cls, expected) = g8.fp8_nonfinite(SMALL)
    fin = ~((a & 0x7F) == 0x7F).any(axis=1)
    cols = ~((b & 0x7F) == 0x7F).any(axis=1)
    got = g8.emu_group_sums(a[fin], b[cols])
    assert np.array_equal(got, expected[fin][:, cols])
    a, b, want, exact = g8.wide_groups(SMALL)
    assert (want != exact).mean() > 0.5 and np.abs(want - exact).max() < 8 * SMALL[2] // 8
    pa, pb = g8.probe_problems()["adjacent_k"][:2]  # rows 14, 15 hold e4m3 subnormals, which the emulator leaves out
    assert np.array_equal(g8.emu_group_sums(pa[:14], pb[:14]), g8.adjacent_k_as_measured()[:14, :14])
