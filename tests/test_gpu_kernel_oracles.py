"""GPU tier: every mandelbrot, nbody, reduce and stream kernel of the library
against the float64 oracles of tests/kernel_oracles.py, element by element,
at the smallest shapes where its indexing and block logic can still go wrong.
The bounds come from the kernels' arithmetic (see kernel_oracles.py); the CPU
tier shows that the same comparisons reject wrong kernels."""
import itertools

import numpy as np
import pytest

import cekirdekler_amd as ck
import kernel_oracles as ko
from cekirdekler_amd.models.mandelbrot import KERNELS as MANDEL_LIBRARY_NAMES

pytestmark = pytest.mark.gpu

f32 = np.float32

MANDEL_KERNELS = ["quad", "blk8", "blk8h", "blk8k", "blk8m", "blk8t", "blk8u", "blk8r", "blk8y"]
NBODY_FORCE = {2: "cek_nbody_f32_b2", 4: "cek_nbody_f32_b4"}
NBODY_INTEGRATE = {2: "cek_nbody_integrate_f32_b2", 4: "cek_nbody_integrate_f32_b4"}
NBODY_ENERGY = {2: "cek_nbody_energy_f32_b2", 4: "cek_nbody_energy_f32_b4"}
REDUCE_PARTIAL = {"cek_reduce_sum_f32": 8, "cek_reduce_sum_f32_x32": 32}  # floats per work item
REDUCE_FINAL = "cek_reduce_sum_f32_final"
STREAM_KERNELS = ["cek_saxpy_f32", "cek_copy_u8", "cek_vec_add_f32"]

# what the tests below are parametrised over (test_kernel_oracles.py checks
# these lists against ops/library.py)
LAUNCHED = {
    "mandelbrot": [MANDEL_LIBRARY_NAMES[k][0] for k in MANDEL_KERNELS],
    "nbody": [*NBODY_FORCE.values(), *NBODY_INTEGRATE.values(), *NBODY_ENERGY.values()],
    "reduce": [*REDUCE_PARTIAL, REDUCE_FINAL],
    "stream": STREAM_KERNELS,
}

_ids = itertools.count(10)  # a compute id of its own per shape and launch mode (1 is the n-body step's)


@pytest.fixture(scope="module")
def crunchers():
    """One cruncher per (library, number of logical devices), made on first
    use and disposed of when the module is done."""
    from cekirdekler_amd.ops.library import library

    made = {}

    def get(lib, devices=1):
        if (lib, devices) not in made:
            g = ck.ClPlatforms.all().gpus()[0]
            made[lib, devices] = ck.ClNumberCruncher(g if devices == 1 else g + g, "", prebuilt=library(lib))
        return made[lib, devices]

    yield get
    for cr in made.values():
        cr.dispose()


class _Arrays:
    """ClArrays of one test case, released from the devices at its end."""

    def __init__(self):
        self.made = []

    def __call__(self, data, dtype=None, **flags):
        a = ck.ClArray(data) if dtype is None else ck.ClArray(data, dtype)
        for k, v in flags.items():
            setattr(a, k, v)
        self.made.append(a)
        return a

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for a in self.made:
            a.dispose()


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


PIPELINES = {"event": ck.PIPELINE_EVENT, "driver": ck.PIPELINE_DRIVER}
MODES = ["one", "two", "event", "driver"]


# --------------------------------------------------------------------------- mandelbrot

_orbits = {}


def _mandel_oracle(shape, view, it):
    if (shape, view) not in _orbits:
        W, H = shape
        _orbits[shape, view] = ko.mandelbrot_orbits(ko.mandel_view_f32(view, W, H), W, H, max(ko.MANDEL_MAX_ITERS))
    return ko.mandelbrot_from_orbits(*_orbits[shape, view], it)


def _mandel_blobs(kernel, W, H):
    """Pipeline blob counts: one band per chunk, and where the band count
    allows it an odd number (> 1) of bands per chunk."""
    if kernel == "quad":  # 256-item groups of 4-pixel work items, no bands
        return {(48, 64): [3], (256, 128): [32, 4], (768, 128): [8]}[W, H]
    bands = H // 8
    return [bands] + ([bands // 3] if bands % 3 == 0 and bands > 3 else [])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", MANDEL_KERNELS)
def test_mandelbrot_equals_oracle_on_decidable_pixels(crunchers, kernel, mode):
    """Exact equality with the float64 oracle on every pixel whose escape
    test a float32 kernel cannot get wrong: one band, one block per band, the
    division path, 12 bands, on one device, two logical devices (a launch
    offset, a centre band per launch) and both pipelines with one band and
    with an odd number of bands per chunk; max_iter at the edges of every
    block-length switch and remainder."""
    from cekirdekler_amd.models.mandelbrot import MandelbrotRenderer

    cr = crunchers("mandelbrot", 2 if mode == "two" else 1)
    shapes = ko.mandel_quad_shapes() if kernel == "quad" else ko.MANDEL_BAND_SHAPES
    worst = 0.0
    for W, H in shapes:
        m = MandelbrotRenderer(W, H, max_iter=1, cruncher=cr, kernel=kernel)
        units = m.global_range // (m.granularity or m.local)  # bands, or work-groups
        try:
            for blobs in (_mandel_blobs(kernel, W, H) if mode in PIPELINES else [1]):
                cid = next(_ids)
                first = True
                for view in ko.MANDEL_VIEWS:
                    m.view.array[:] = ko.mandel_view_f32(view, W, H)
                    for it in ko.MANDEL_MAX_ITERS:
                        m.size.array[2] = m.max_iter = it
                        m.out.array[:] = -1
                        img = m.render(cid, pipeline=mode in PIPELINES, blobs=blobs,
                                       pipeline_type=PIPELINES.get(mode, ck.PIPELINE_EVENT))
                        if first:
                            first = False
                            if mode == "two" and units >= 2:
                                assert all(r > 0 for r in cr.ranges(cid)), cr.ranges(cid)
                            if mode in PIPELINES and blobs > 1:
                                assert cr.last_record()["pipelined"], cr.last_record()
                        n, dec = _mandel_oracle((W, H), view, it)
                        worst = max(worst, 1.0 - float(dec.mean()))
                        try:
                            ko.check_mandelbrot(img, n, dec, it)
                        except AssertionError as e:
                            raise AssertionError(f"{kernel} {mode} {W}x{H} view {view} max_iter {it} "
                                                 f"blobs {blobs}: {e}") from None
        finally:
            for a in (m.view, m.size, m.out):
                a.dispose()
    print(f"[oracle] mandelbrot {kernel} {mode}: worst undecidable share {worst:.4f}")


@pytest.mark.parametrize("devices", [1, 2])
def test_mandelbrot_renderer_returns_to_earlier_parameters(crunchers, devices):
    """The renderer uploads view and size only when they changed: going back
    to parameters it has used before, under the same compute id or another,
    must upload them again (a device holds one copy per array)."""
    from cekirdekler_amd.models.mandelbrot import MandelbrotRenderer

    cr = crunchers("mandelbrot", devices)
    W, H = 48, 32
    m = MandelbrotRenderer(W, H, max_iter=1, cruncher=cr, kernel="blk8y")
    ids = [next(_ids), next(_ids)]
    try:
        for cid, view, it in [(0, 0, 12), (0, 0, 33), (0, 0, 12), (1, 2, 12), (0, 0, 12), (0, 2, 33), (1, 0, 12)]:
            view = ko.MANDEL_VIEWS[view]
            m.view.array[:] = ko.mandel_view_f32(view, W, H)
            m.size.array[2] = m.max_iter = it
            m.out.array[:] = -1
            img = m.render(ids[cid], pipeline=False)
            ko.check_mandelbrot(img, *_mandel_oracle((W, H), view, it), it)
    finally:
        for a in (m.view, m.size, m.out):
            a.dispose()


# --------------------------------------------------------------------------- n-body

def _nbody_params(n):
    return np.array([ko.NBODY_EPS * ko.NBODY_EPS, ko.NBODY_G, float(n), ko.NBODY_DT], f32)


def _owned(B, n):
    """Bodies of the whole work-groups (256·B bodies each) that n holds: the
    range the kernels are launched over."""
    return n // (256 * B) * (256 * B)


def _devices_for(B, n):
    return [1, 2] if _owned(B, n) // (256 * B) >= 2 else [1]


FORCE_CASES = [(B, n, "normal") for B, n in ko.NBODY_SIZES] + [
    (2, 1024, "shifted"), (4, 2048, "shifted"), (2, 768, "coincident"), (4, 1024, "coincident")]


@pytest.mark.parametrize("B,n,kind,devices", [(B, n, k, d) for B, n, k in FORCE_CASES for d in _devices_for(B, n)])
def test_nbody_force_within_per_body_bound(crunchers, B, n, kind, devices):
    """Per body and per component |a − a64| <= (n + 32)·2^-24·S with
    heterogeneous masses (some 0), G = 6.5, two and three j tiles, one and two
    work-groups.  n = 768 with two bodies per item holds one whole work-group:
    its 512 bodies feel all 768."""
    cr = crunchers("nbody", devices)
    bodies = ko.nbody_bodies(n, kind)
    params = _nbody_params(n)
    own = _owned(B, n)
    with _Arrays() as A:
        e = 4 * B
        pos = A(bodies.reshape(-1).copy(), write=False, elements_per_work_item=e)
        vel = A(np.zeros(4 * n, f32), read=False, write=False, elements_per_work_item=e)
        acc = A(np.full(4 * n, np.nan, f32), read=False, elements_per_work_item=e)
        par = A(params, write=False)
        cid = next(_ids)
        pos.next_param(vel, acc, par).compute(cr, cid, NBODY_FORCE[B], own // B, 256)
        if devices == 2:
            assert all(r > 0 for r in cr.ranges(cid)), cr.ranges(cid)
        got = acc.array.reshape(-1, 4).copy()
    a, S = ko.nbody_accel_oracle(bodies, float(params[0]), float(params[1]))
    worst = ko.check_bound(got[:own, :3], a[:own], ko.nbody_accel_bound(S, n)[:own],
                           f"{NBODY_FORCE[B]} n={n} {kind} devices={devices}")
    assert not got[:own, 3].any()            # acc.w = 0
    assert np.isnan(got[own:]).all()         # nothing written past the launched bodies
    print(f"[oracle] {NBODY_FORCE[B]} n={n} {kind} devices={devices}: worst err/bound {worst:.4f}")


@pytest.mark.parametrize("B,n,devices", [(B, n, d) for B, n in ko.NBODY_SIZES for d in _devices_for(B, n)])
def test_nbody_integrate_alone_one_ulp(crunchers, B, n, devices):
    """The kick-drift kernel on its own: v' and x' within 1 float32 ulp of the
    float64 a·dt + v and v'·dt + x; pos.w, vel.w and acc come back
    bit-identical, and so does everything past the launched bodies."""
    cr = crunchers("nbody", devices)
    rng = np.random.default_rng(11)
    pos0, vel0, acc0 = (rng.standard_normal((n, 4)).astype(f32) for _ in range(3))
    params = _nbody_params(n)
    own = _owned(B, n)
    with _Arrays() as A:
        flags = dict(partial_read=True, elements_per_work_item=4 * B)
        pos, vel, acc = (A(x.reshape(-1).copy(), **flags) for x in (pos0, vel0, acc0))
        par = A(params, write=False)
        cid = next(_ids)
        pos.next_param(vel, acc, par).compute(cr, cid, NBODY_INTEGRATE[B], own // B, 256)
        if devices == 2:
            assert all(r > 0 for r in cr.ranges(cid)), cr.ranges(cid)
        p1, v1, a1 = (x.array.reshape(-1, 4).copy() for x in (pos, vel, acc))
    x64, v64 = ko.leapfrog_oracle(pos0[:own], vel0[:own], acc0[:own], float(params[3]), v_kernel=v1[:own])
    what = f"{NBODY_INTEGRATE[B]} n={n} devices={devices}"
    wv = ko.check_bound(v1[:own, :3], v64, ko.ulp32(v64), what + " v'")
    wx = ko.check_bound(p1[:own, :3], x64, ko.ulp32(x64), what + " x'")
    assert np.array_equal(_bits(p1[:, 3]), _bits(pos0[:, 3])) and np.array_equal(_bits(v1[:, 3]), _bits(vel0[:, 3]))
    assert np.array_equal(_bits(a1), _bits(acc0))
    assert np.array_equal(_bits(p1[own:]), _bits(pos0[own:])) and np.array_equal(_bits(v1[own:]), _bits(vel0[own:]))
    print(f"[oracle] {what}: worst err/ulp v' {wv:.3f}, x' {wx:.3f}")


@pytest.mark.parametrize("resident", [True, False])
@pytest.mark.parametrize("B,n,devices", [(2, 1024, 1), (2, 1024, 2), (4, 2048, 1), (4, 2048, 2)])
def test_nbody_step_matches_leapfrog_of_oracle(crunchers, B, n, devices, resident):
    """One NBodySimulation.step() from rest against the leapfrog of the
    float64 acceleration, the force bound propagated: dt·bound on v,
    dt²·bound on x, plus 1 ulp."""
    from cekirdekler_amd.models.nbody import NBodySimulation

    cr = crunchers("nbody", devices)
    sim = NBodySimulation(n, cruncher=cr, eps=ko.NBODY_EPS, dt=ko.NBODY_DT, g=ko.NBODY_G, resident=resident,
                          bodies_per_item=B)
    try:
        bodies = ko.nbody_bodies(n, seed=2)
        sim.pos.array[:] = bodies.reshape(-1)
        sim.step(1)
        sim.download()
        p1 = sim.pos.array.reshape(-1, 4).copy()
        v1 = sim.vel.array.reshape(-1, 4).copy()
        params = sim.params.array.copy()
    finally:
        for a in (sim.pos, sim.vel, sim.acc, sim.params):
            a.dispose()
    dt = float(params[3])
    a, S = ko.nbody_accel_oracle(bodies, float(params[0]), float(params[1]))
    bound = ko.nbody_accel_bound(S, n)
    x64, v64 = ko.leapfrog_oracle(bodies, np.zeros((n, 4)), np.c_[a, np.zeros(n)], dt)
    what = f"step b{B} n={n} devices={devices} resident={resident}"
    wv = ko.check_bound(v1[:, :3], v64, dt * bound + ko.ulp32(v64), what + " v")
    wx = ko.check_bound(p1[:, :3], x64, dt * dt * bound + ko.ulp32(x64), what + " x")
    assert np.array_equal(_bits(p1[:, 3]), _bits(bodies[:, 3]))
    print(f"[oracle] {what}: worst err/bound v {wv:.4f}, x {wx:.4f}")


@pytest.mark.parametrize("devices", [1, 2])
@pytest.mark.parametrize("B", [2, 4])
def test_nbody_energy_per_group(crunchers, B, devices):
    """energy[g] = Σ ½·m·|v|² over group g's 256·B bodies, every group with
    masses and a velocity scale of its own, within (B + 13)·2^-24·energy[g]."""
    groups = 4
    n = groups * 256 * B
    cr = crunchers("nbody", devices)
    rng = np.random.default_rng(5)
    bodies = ko.nbody_bodies(n, seed=4)
    vel0 = rng.standard_normal((n, 4)).astype(f32)
    vel0 *= np.repeat(f32(10.0) ** np.arange(groups, dtype=f32), 256 * B)[:, None]
    with _Arrays() as A:
        flags = dict(partial_read=True, write=False, elements_per_work_item=4 * B)
        pos, vel = A(bodies.reshape(-1).copy(), **flags), A(vel0.reshape(-1).copy(), **flags)
        en = A(np.full(groups, np.nan, f32), read=False, elements_per_group=1)
        cid = next(_ids)
        pos.next_param(vel, en).compute(cr, cid, NBODY_ENERGY[B], n // B, 256)
        if devices == 2:
            assert all(r > 0 for r in cr.ranges(cid)), cr.ranges(cid)
        got = en.array.copy()
    sums, abs_sums = ko.block_sums_oracle(ko.kinetic_terms(bodies, vel0), 256 * B)
    assert len(set(sums.tolist())) == groups
    worst = ko.check_bound(got, sums, ko.block_sum_bound(abs_sums, ko.energy_depth(B)),
                           f"{NBODY_ENERGY[B]} devices={devices}")
    print(f"[oracle] {NBODY_ENERGY[B]} devices={devices}: worst err/bound {worst:.4f}")


# --------------------------------------------------------------------------- reduce

@pytest.mark.parametrize("kernel", list(REDUCE_PARTIAL))
def test_reduce_partials_per_group(crunchers, kernel):
    """Every partials[g] against its own block on two logical devices: signed
    data over six decades, all block sums distinct."""
    per_item = REDUCE_PARTIAL[kernel]
    groups, block = 4, 256 * per_item
    cr = crunchers("reduce", 2)
    data = ko.reduce_data(groups, block)
    with _Arrays() as A:
        x = A(data.copy(), write=False, elements_per_work_item=per_item)
        part = A(np.full(groups, np.nan, f32), read=False, elements_per_group=1)
        cid = next(_ids)
        x.next_param(part).compute(cr, cid, kernel, groups * 256, 256)
        assert all(r > 0 for r in cr.ranges(cid)), cr.ranges(cid)
        got = part.array.copy()
    sums, abs_sums = ko.block_sums_oracle(data, block)
    worst = ko.check_bound(got, sums, ko.block_sum_bound(abs_sums, ko.REDUCE_DEPTH[kernel]), kernel)
    print(f"[oracle] {kernel}: worst err/bound {worst:.4f}")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 255, 256, 257, 1000, 4096])
def test_reduce_final(crunchers, n):
    """One group folds n partials; the array goes on past n filled with NaN,
    so an over-read shows; n = 0 gives exactly 0."""
    cr = crunchers("reduce", 1)
    rng = np.random.default_rng(n)
    data = np.full(n + 64, np.nan, f32)
    data[:n] = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 3, n)).astype(f32)
    with _Arrays() as A:
        sizes = A(np.array([n], np.int32), write=False)
        part = A(data.copy(), write=False)
        out = A(np.full(1, np.nan, f32), read=False, elements_per_group=1)
        sizes.next_param(part, out).compute(cr, next(_ids), REDUCE_FINAL, 256, 256)
        got = out.array.copy()
    if n == 0:
        assert got[0] == 0.0 and not np.signbit(got[0])
        return
    sums, abs_sums = ko.block_sums_oracle(data[:n], n)
    worst = ko.check_bound(got, sums, ko.block_sum_bound(abs_sums, ko.reduce_final_depth(n)), f"{REDUCE_FINAL} n={n}")
    print(f"[oracle] {REDUCE_FINAL} n={n}: worst err/bound {worst:.4f}")


# --------------------------------------------------------------------------- stream

STREAM_ITEMS = 2 * 8 * 256  # work items: two devices, or 8 blobs, of one 256-item group each at the least


def _stream_compute(cr, mode, group, kernel):
    cid = next(_ids)
    if mode in PIPELINES:
        group.compute(cr, cid, kernel, STREAM_ITEMS, 256, 0, True, PIPELINES[mode], 8)
        assert cr.last_record()["pipelined"], cr.last_record()
    else:
        group.compute(cr, cid, kernel, STREAM_ITEMS, 256)
        if mode == "two":
            assert all(r > 0 for r in cr.ranges(cid)), cr.ranges(cid)


@pytest.mark.parametrize("mode", MODES)
def test_stream_copy_u8_exact(crunchers, mode):
    cr = crunchers("stream", 2 if mode == "two" else 1)
    data = np.random.default_rng(1).integers(0, 256, 16 * STREAM_ITEMS, dtype=np.uint8)
    with _Arrays() as A:
        src = A(data.copy(), partial_read=True, write=False, elements_per_work_item=16)
        dst = A(np.zeros_like(data), read=False, elements_per_work_item=16)
        _stream_compute(cr, mode, src.next_param(dst), "cek_copy_u8")
        got = dst.array.copy()
    np.testing.assert_array_equal(got, data)


@pytest.mark.parametrize("mode", MODES)
def test_stream_vec_add_exact(crunchers, mode):
    cr = crunchers("stream", 2 if mode == "two" else 1)
    rng = np.random.default_rng(2)
    a0, b0 = (rng.standard_normal(4 * STREAM_ITEMS).astype(f32) * f32(1e3) for _ in range(2))
    with _Arrays() as A:
        a, b = (A(x.copy(), partial_read=True, write=False, elements_per_work_item=4) for x in (a0, b0))
        c = A(np.full(4 * STREAM_ITEMS, np.nan, f32), read=False, elements_per_work_item=4)
        _stream_compute(cr, mode, a.next_param(b, c), "cek_vec_add_f32")
        got = c.array.copy()
    assert np.array_equal(_bits(got), _bits(a0 + b0))


@pytest.mark.parametrize("mode", MODES)
def test_stream_saxpy(crunchers, mode):
    """Exact on integer-valued data below 2^12 (fused and unfused agree), and
    within 1 ulp of the float64 result on random data."""
    cr = crunchers("stream", 2 if mode == "two" else 1)
    rng = np.random.default_rng(3)
    nel = 4 * STREAM_ITEMS
    cases = [(f32(4093.0), rng.integers(-4095, 4096, nel).astype(f32), rng.integers(-4095, 4096, nel).astype(f32)),
             (f32(rng.standard_normal()), rng.standard_normal(nel).astype(f32), rng.standard_normal(nel).astype(f32))]
    for k, (s, x0, y0) in enumerate(cases):
        with _Arrays() as A:
            a = A(np.array([s], f32), write=False)
            x = A(x0.copy(), partial_read=True, write=False, elements_per_work_item=4)
            y = A(y0.copy(), partial_read=True, elements_per_work_item=4)
            _stream_compute(cr, mode, a.next_param(x, y), "cek_saxpy_f32")
            got = y.array.copy()
        ref = np.float64(s) * x0.astype(np.float64) + y0.astype(np.float64)
        if k == 0:
            assert np.array_equal(got.astype(np.float64), ref)
        else:
            worst = ko.check_bound(got, ref, ko.ulp32(ref), f"cek_saxpy_f32 {mode}")
            print(f"[oracle] cek_saxpy_f32 {mode}: worst err/ulp {worst:.3f}")
