"""CPU tier for tests/kernel_oracles.py: the oracles agree with independent
float32 emulations wherever they claim to decide, and the comparison functions
the GPU tier uses reject subtly wrong kernels (mutants)."""
import functools
import types

import numpy as np
import pytest

import kernel_oracles as ko

f32 = np.float32
ALL_SHAPES = ko.MANDEL_BAND_SHAPES + ko.MANDEL_QUAD_EXTRA_SHAPES


# --------------------------------------------------------------------------- mandelbrot

@functools.lru_cache(maxsize=None)
def _orbits(shape, view):
    W, H = shape
    return ko.mandelbrot_orbits(ko.mandel_view_f32(view, W, H), W, H, max(ko.MANDEL_MAX_ITERS))


def _reference(view_f32, W, H, max_iter):
    """MandelbrotRenderer.reference() on a stub that holds what it reads."""
    from cekirdekler_amd.models.mandelbrot import MandelbrotRenderer

    stub = types.SimpleNamespace(view=types.SimpleNamespace(array=view_f32), width=W, height=H, max_iter=max_iter)
    with np.errstate(over="ignore", invalid="ignore"):  # escaped pixels run on to inf and NaN
        return MandelbrotRenderer.reference(stub)


@pytest.mark.parametrize("view", ko.MANDEL_VIEWS)
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_mandelbrot_oracle_validity(shape, view):
    """On every case of the GPU tier: the project's float32 reference and a
    fused float32 emulation equal the oracle on all decidable pixels, and the
    undecidable share stays at most 0.04."""
    W, H = shape
    vf = ko.mandel_view_f32(view, W, H)
    esc, und = _orbits(shape, view)
    worst = 0.0
    for it in ko.MANDEL_MAX_ITERS:
        n, dec = ko.mandelbrot_from_orbits(esc, und, it)
        ko.check_mandelbrot(_reference(vf, W, H, it), n, dec, it)
        ko.check_mandelbrot(ko.mandelbrot_f32_fused(vf, W, H, it), n, dec, it)
        worst = max(worst, 1.0 - dec.mean())
    print(f"mandelbrot {shape} {view}: worst undecidable share {worst:.4f}")
    assert worst <= ko.MANDEL_MAX_UNDECIDABLE


@pytest.mark.parametrize("it", [1, 9, 33, 100])
def test_mandelbrot_oracle_single_run_equals_derived(it):
    """mandelbrot_oracle(max_iter) is what a longer orbit run gives for it."""
    shape, view = (48, 96), ko.MANDEL_VIEWS[2]
    n, dec = ko.mandelbrot_oracle(ko.mandel_view_f32(view, *shape), *shape, it)
    n2, dec2 = ko.mandelbrot_from_orbits(*_orbits(shape, view), it)
    assert np.array_equal(n, n2) and np.array_equal(dec, dec2)


def _mandel_case(shape, view, it):
    n, dec = ko.mandelbrot_from_orbits(*_orbits(shape, view), it)
    good = n.copy()  # a correct kernel's image (any value would do where undecidable)
    ko.check_mandelbrot(good, n, dec, it)
    return n, dec, good


def _rejected(img, n, dec, it):
    assert not np.array_equal(img, n), "the mutant equals the original"
    with pytest.raises(AssertionError):
        ko.check_mandelbrot(img, n, dec, it)


@pytest.mark.parametrize("shape,view", [((48, 96), ko.MANDEL_VIEWS[0]), ((256, 128), ko.MANDEL_VIEWS[2]),
                                        ((64, 8), ko.MANDEL_VIEWS[0])])
def test_mandelbrot_mutant_block_shifted(shape, view):
    """Every 8×16 block whose right-hand neighbour differs from it: writing
    the neighbour's counts in its place is rejected."""
    W, H = shape
    n, dec, good = _mandel_case(shape, view, 100)
    tried = 0
    for r in range(0, H, 8):
        for c in range(0, W - 16, 16):
            if np.array_equal(good[r:r + 8, c:c + 16], good[r:r + 8, c + 16:c + 32]):
                continue
            img = good.copy()
            img[r:r + 8, c:c + 16] = good[r:r + 8, c + 16:c + 32]
            _rejected(img, n, dec, 100)
            tried += 1
    assert tried > 0


def test_mandelbrot_mutant_bands_swapped():
    shape, view = (48, 96), ko.MANDEL_VIEWS[0]
    n, dec, good = _mandel_case(shape, view, 64)
    for a, b in [(0, 1), (5, 6), (4, 7), (10, 11)]:  # (5, 6) mirror each other about the real axis…
        img = good.copy()
        img[8 * a:8 * a + 8], img[8 * b:8 * b + 8] = good[8 * b:8 * b + 8], good[8 * a:8 * a + 8]
        if np.array_equal(img, good):
            continue  # …and may hold the same counts
        _rejected(img, n, dec, 64)
    img = good.copy()
    img[0:8], img[8:16] = good[8:16], good[0:8]
    _rejected(img, n, dec, 64)


@pytest.mark.parametrize("it", [5, 9, 16, 17, 32, 33, 40, 64, 65])
def test_mandelbrot_mutant_last_counted_iteration(it):
    """+1 on every pixel whose count is max_iter − 1 (an escape at the last
    counted iteration taken for none)."""
    hit = 0
    for view in ko.MANDEL_VIEWS:
        n, dec, good = _mandel_case((256, 128), view, it)
        if not (dec & (n == it - 1)).any():
            continue
        img = good.copy()
        img[good == it - 1] += 1
        _rejected(img, n, dec, it)
        hit += 1
    assert hit > 0


def test_mandelbrot_mutant_block_switch_iteration():
    """+1 on every pixel with count 32 (the switch from 8- to 32-iteration blocks)."""
    for it in (40, 100):
        n, dec, good = _mandel_case((256, 128), ko.MANDEL_VIEWS[2], it)
        assert (dec & (n == 32)).any()
        img = good.copy()
        img[good == 32] += 1
        _rejected(img, n, dec, it)


@pytest.mark.parametrize("it", [8, 9, 33, 100])
def test_mandelbrot_mutant_interior_one_short(it):
    """Interior pixels returned as max_iter − 1."""
    n, dec, good = _mandel_case((256, 128), ko.MANDEL_VIEWS[1], it)
    assert (dec & (n == it)).any()
    img = good.copy()
    img[good == it] = it - 1
    _rejected(img, n, dec, it)


def test_mandelbrot_out_of_range_rejected():
    n, dec, good = _mandel_case((64, 8), ko.MANDEL_VIEWS[0], 16)
    for v in (-1, 17):
        img = good.copy()
        img[~dec] = v  # even where only undecidable pixels are off
        img[0, 0] = v
        with pytest.raises(AssertionError):
            ko.check_mandelbrot(img, n, dec, 16)


# --------------------------------------------------------------------------- n-body

def _force_f32(pos, eps2, G, order=None, lanes=1, drop_term=None):
    """float32 emulation of the force loop: the j bodies in `order`,
    accumulated in `lanes` interleaved partial sums that are added at the
    end (1: the kernel's sequential order)."""
    p = pos.reshape(-1, 4).astype(f32)
    n = len(p)
    order = np.arange(n) if order is None else order
    acc = np.zeros((lanes, n, 3), f32)
    x = p[:, :3]
    for k, j in enumerate(order):
        if drop_term is not None and j == drop_term:
            continue
        d = p[j, :3][None, :] - x                                            # 1 rounding each
        r2 = (d.astype(np.float64) ** 2).sum(1) + np.float64(eps2)           # fma chain: about one rounding
        inv = (1.0 / np.sqrt(r2.astype(f32).astype(np.float64))).astype(f32)
        s = (p[j, 3] * inv) * (inv * inv)
        acc[k % lanes] = (d.astype(np.float64) * s[:, None] + acc[k % lanes]).astype(f32)
    out = acc[0]
    for q in range(1, lanes):
        out = out + acc[q]
    return f32(G) * out


NB_N = 768


@functools.lru_cache(maxsize=None)
def _nbody_case():
    pos = ko.nbody_bodies(NB_N)
    eps2 = float(f32(ko.NBODY_EPS * ko.NBODY_EPS))
    a, S = ko.nbody_accel_oracle(pos, eps2, ko.NBODY_G)
    return pos, eps2, a, ko.nbody_accel_bound(S, NB_N)


def test_nbody_oracle_matches_model_reference():
    from cekirdekler_amd.models.nbody import nbody_accel_reference

    pos, eps2, a, _ = _nbody_case()
    np.testing.assert_allclose(a, nbody_accel_reference(pos.reshape(-1), eps2, ko.NBODY_G), rtol=1e-12, atol=1e-300)


def test_nbody_float32_orders_inside_bound():
    """Sequential accumulation and two differently ordered tilings stay inside
    the bound, on plain, shifted and coincident bodies."""
    tiles = np.arange(NB_N).reshape(-1, 256)
    orders = [(None, 1), (tiles[::-1].reshape(-1), 1), (tiles[:, ::-1].reshape(-1), 4)]
    for kind in ("normal", "shifted", "coincident"):
        pos = ko.nbody_bodies(NB_N, kind)
        eps2 = float(f32(ko.NBODY_EPS * ko.NBODY_EPS))
        a, S = ko.nbody_accel_oracle(pos, eps2, ko.NBODY_G)
        for order, lanes in orders:
            worst = ko.check_bound(_force_f32(pos, eps2, ko.NBODY_G, order, lanes), a, ko.nbody_accel_bound(S, NB_N),
                                   f"float32 emulation ({kind})")
            print(f"nbody float32 emulation {kind} lanes {lanes}: worst err/bound {worst:.3f}")
            assert worst < 1.0


def _nbody_rejected(got):
    _, _, a, bound = _nbody_case()
    with pytest.raises(AssertionError):
        ko.check_bound(got, a, bound, "mutant")


def test_nbody_mutant_one_term_dropped():
    pos, eps2, _, _ = _nbody_case()
    heavy = int(np.argmax(pos[:, 3]))
    _nbody_rejected(_force_f32(pos, eps2, ko.NBODY_G, drop_term=heavy))


def test_nbody_mutant_last_tile_dropped():
    pos, eps2, _, _ = _nbody_case()
    _nbody_rejected(_force_f32(pos, eps2, ko.NBODY_G, order=np.arange(NB_N - 256)))


def test_nbody_mutant_masses_rolled():
    pos, eps2, _, _ = _nbody_case()
    rolled = pos.copy()
    rolled[:, 3] = np.roll(pos[:, 3], 1)
    _nbody_rejected(_force_f32(rolled, eps2, ko.NBODY_G))


def test_nbody_mutant_g_ignored():
    pos, eps2, _, _ = _nbody_case()
    _nbody_rejected(_force_f32(pos, eps2, 1.0))


def test_nbody_quiet_body_is_checked():
    """The bound is per body: an error in one quiet body alone, far below
    the largest acceleration of all bodies, is rejected."""
    pos, eps2, a, bound = _nbody_case()
    got = _force_f32(pos, eps2, ko.NBODY_G)
    quiet = int(np.argmin(np.abs(a).max(1)))
    got[quiet] *= f32(1.01)
    assert np.abs(got[quiet] - a[quiet]).max() < 1e-4 * np.abs(a).max()  # the old tolerance lets it through
    _nbody_rejected(got)


def test_leapfrog_oracle_one_ulp_rule():
    rng = np.random.default_rng(3)
    n = 512
    pos, vel, acc = (rng.standard_normal((n, 4)).astype(f32) for _ in range(3))
    dt = float(f32(ko.NBODY_DT))
    # the kernel's fmaf: exact product and sum, one rounding (float64 holds a·dt exactly)
    v_k = np.zeros((n, 4), f32)
    v_k[:, :3] = (acc[:, :3].astype(np.float64) * dt + vel[:, :3]).astype(f32)
    x_k = (v_k[:, :3].astype(np.float64) * dt + pos[:, :3]).astype(f32)
    x1, v1 = ko.leapfrog_oracle(pos, vel, acc, dt, v_kernel=v_k)
    ko.check_bound(v_k[:, :3], v1, ko.ulp32(v1), "v'")
    ko.check_bound(x_k, x1, ko.ulp32(x1), "x'")
    # x advanced with the old velocity, or v kicked with dt twice, is beyond 1 ulp
    with pytest.raises(AssertionError):
        ko.check_bound((vel[:, :3].astype(np.float64) * dt + pos[:, :3]).astype(f32), x1, ko.ulp32(x1), "x' mutant")
    with pytest.raises(AssertionError):
        ko.check_bound((acc[:, :3].astype(np.float64) * 2 * dt + vel[:, :3]).astype(f32), v1, ko.ulp32(v1), "v' mutant")


# --------------------------------------------------------------------------- reduce

def _tree_sum_f32(x, block):
    """Pairwise float32 tree per block (the shape of the kernels' sums)."""
    b = x.astype(f32).reshape(-1, block)
    while b.shape[1] > 1:
        b = b[:, 0::2] + b[:, 1::2]
    return b[:, 0]


@pytest.mark.parametrize("kernel,block", [("cek_reduce_sum_f32", 2048), ("cek_reduce_sum_f32_x32", 8192)])
def test_reduce_tree_sum_inside_bound_and_mutants_outside(kernel, block):
    x = ko.reduce_data(4, block)
    sums, abs_sums = ko.block_sums_oracle(x, block)
    assert len(set(sums.tolist())) == 4
    bound = ko.block_sum_bound(abs_sums, ko.REDUCE_DEPTH[kernel])
    good = _tree_sum_f32(x, block)  # depth log2(block) <= the kernels' chain
    assert np.log2(block) <= ko.REDUCE_DEPTH[kernel]
    assert ko.check_bound(good, sums, bound, kernel) < 1.0
    swapped = good.copy()
    swapped[[1, 2]] = good[[2, 1]]  # right total, wrong group index
    assert np.isclose(swapped.sum(), good.sum())
    with pytest.raises(AssertionError):
        ko.check_bound(swapped, sums, bound, "swapped partials")
    y = x.copy()
    i = 2 * block + int(np.argmax(np.abs(x[2 * block:3 * block])))
    y[i] = 0  # one element dropped from one block
    with pytest.raises(AssertionError):
        ko.check_bound(_tree_sum_f32(y, block), sums, bound, "dropped element")


def test_reduce_final_and_energy_depths():
    assert [ko.reduce_final_depth(n) for n in (0, 1, 256, 257, 4096)] == [10, 11, 11, 12, 26]
    assert ko.energy_depth(2) == 15 and ko.energy_depth(4) == 17


def test_energy_terms_oracle_rejects_swapped_groups():
    rng = np.random.default_rng(5)
    B, groups = 2, 4
    n = groups * 256 * B
    pos = ko.nbody_bodies(n)
    vel = rng.standard_normal((n, 4)).astype(f32) * np.repeat(10.0 ** np.arange(groups), 256 * B)[:, None].astype(f32)
    sums, abs_sums = ko.block_sums_oracle(ko.kinetic_terms(pos, vel), 256 * B)
    bound = ko.block_sum_bound(abs_sums, ko.energy_depth(B))
    good = _tree_sum_f32(ko.kinetic_terms(pos, vel).astype(f32), 256 * B)
    assert ko.check_bound(good, sums, bound, "energy") < 1.0
    with pytest.raises(AssertionError):
        ko.check_bound(good[::-1], sums, bound, "energy, groups reversed")


# --------------------------------------------------------------------------- coverage

def test_gpu_file_launches_every_library_kernel():
    """The GPU tier's kernel lists (what its tests are parametrised over)
    cover every mandelbrot, nbody, reduce and stream kernel of the library."""
    import test_gpu_kernel_oracles as gpu
    from cekirdekler_amd.ops.library import LIBRARY

    for lib in ("mandelbrot", "nbody", "reduce", "stream"):
        assert sorted(gpu.LAUNCHED[lib]) == sorted(LIBRARY[lib]), lib
