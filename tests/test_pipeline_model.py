"""CPU tier of the pipeline model (tests/pipeline_model.py).

Model against itself: every fault in FAULTS / DP_FAULTS is rejected by its
named case, and the fault-free per-device models equal the one-device oracle.
Model against the real pipelines on CPU devices (``cpus(True)``, ``cpu +
cpu``): every push of every case, element by element, and every feed of the
DevicePipeline case in its four feed modes.

CPU devices of one stage share the stage's host arrays, so this tier cannot
see incoherence between replicas: it validates the emulator, the stage
kernels, the swap rules and the ready-counter rule.  Replicas are the GPU
tier's subject (tests/test_gpu_pipeline_model.py).
"""
import numpy as np
import pytest

import cekirdekler_amd as ck
import pipeline_model as pm

CASES = pm.cases()


# ------------------------------------------------------------------ the case lists


def test_case_list_covers_what_it_claims():
    stages = [s for c in CASES for s in c.stages]
    assert {s.kind for s in stages} == {"acc", "two", "join", "init"}
    assert {len(s.devices) for s in stages} == {1, 2, 3}
    assert any(s.devices == "gc" for s in stages)
    assert {s.E for s in stages if s.kind == "acc"} == {1, 3}
    assert any(s.tail == pm.TAIL for s in stages)
    transitions = {(len(a.devices), len(b.devices)) for c in CASES for a, b in zip(c.stages, c.stages[1:])}
    assert {(3, 1), (1, 2), (2, 3)} <= transitions
    assert {c.mode for c in CASES} == {"both", "drain", "gaps"}
    assert {c.data_form for c in CASES} == {"array", "list", "strided"}
    assert {c.type_name for c in CASES} == set(pm.TYPES)
    # an input shorter than the output feeding it, and one that takes the tail too
    pairs = [(pm.buffers_of(a)[-1].n, b.xn) for c in CASES for a, b in zip(c.stages, c.stages[1:]) if a.kind == "acc"]
    assert any(src > dst for src, dst in pairs) and any(src == dst and src > 3 * pm.N for src, dst in pairs)
    # the unaligned per-group record: uchar slices at multiples of 7 bytes
    assert any(c.type_name == "uchar" and any(s.kind == "two" and len(s.devices) > 1 for s in c.stages) for c in CASES)
    for c in CASES:
        assert 1 <= len(c.stages) <= 3 and c.pushes == 2 * len(c.stages) + 6
        plan = pm.push_plan(c)
        assert len(plan) == c.pushes
        if c.mode == "gaps":
            assert {(False, False), (True, False), (False, True), (True, True)} == set(plan)
    assert len({c.name for c in CASES}) == len(CASES)


def test_synthetic_splits_move_differ_and_leave_no_device_idle():
    for c in CASES:
        per_push = [pm.synthetic_splits(c, p) for p in range(c.pushes)]
        for si, s in enumerate(c.stages):
            D = len(s.devices)
            for sp in per_push:
                for ranges, refs in sp[si]:
                    assert sum(ranges) == pm.N and all(r > 0 and r % pm.L == 0 for r in ranges)
                    assert refs == [sum(ranges[:d]) for d in range(D)]
            if D > 1:
                assert len({tuple(sp[si][0][0]) for sp in per_push}) > 1
                if s.kind == "two":
                    assert any(sp[si][0][0] != sp[si][1][0] for sp in per_push)


# ------------------------------------------------------------------ model against itself


@pytest.mark.parametrize("case", CASES, ids=str)
def test_per_device_model_equals_the_one_device_oracle(case):
    oracle = pm.run_model(case, coherent=True)
    assert pm.first_difference(pm.run_model(case), oracle) is None
    assert any(ready for ready, _, _ in oracle) and not oracle[0][0]


@pytest.mark.parametrize("name", sorted({pm.FAULT_CASES[f] for f in pm.PER_DEVICE_OUTPUTS}))
def test_per_output_ownership_variant_equals_the_oracle(name):
    case = pm.case_named(name)
    assert pm.first_difference(pm.run_model(case, per_device_outputs=True), pm.run_model(case, coherent=True)) is None


def test_every_fault_has_a_named_case():
    assert set(pm.FAULT_CASES) == set(pm.FAULTS)
    assert set(pm.DP_FAULT_CASES) == set(pm.DP_FAULTS)


@pytest.mark.parametrize("fault", pm.FAULTS)
def test_fault_is_rejected_by_its_case(fault):
    case = pm.case_named(pm.FAULT_CASES[fault])
    diff = pm.first_difference(pm.run_model(case, faults=[fault]), pm.run_model(case, coherent=True))
    assert diff is not None, f"{fault} passes {case.name}"


def test_unknown_fault_is_refused():
    with pytest.raises(KeyError):
        pm.Emulator(CASES[0], faults=["no_such_rule"])
    with pytest.raises(KeyError):
        pm.DpEmulator(np.int32, faults=["no_such_rule"])


def test_model_byte_counts_follow_the_layout():
    """All-GPU layout: h2d is the data to every device of stage 0, d2h the
    results once, nothing through host memory, and the peer bytes are every
    source byte once per destination device."""
    case = pm.case_named("stateful-3-1-2")
    seen = pm.run_model(case)
    item = case.dtype.itemsize
    P = case.pushes
    assert seen[-1][2] == {"h2d": P * 3 * pm.N * item, "d2h": P * (pm.N * item), "host": 0,
                           "p2p": P * (1 * pm.N * item + 2 * pm.N * item)}


# ------------------------------------------------------------------ model against the real ClPipeline


@pytest.fixture(scope="module")
def cpu():
    return ck.ClPlatforms.all().cpus(True)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_real_pipeline_on_cpu_devices_equals_the_oracle(case, cpu):
    on_cpu = case.on_cpu()
    pipe, stages = pm.build_pipeline(on_cpu, lambda ch: cpu)
    try:
        run = pm.run_pipeline(on_cpu, pipe, stages)
    finally:
        pipe.dispose()
    pm.check_against_oracle(case, run["seen"], "cpu devices")
    # host memory only: the bytes the per-device model counts for this layout
    model = pm.run_model(on_cpu, splits_of=lambda c, p: run["splits"][p])
    assert [s[2] for s in run["seen"]] == [s[2] for s in model]
    assert run["seen"][-1][2]["host"] > 0 and run["seen"][-1][2]["p2p"] == 0
    for s, g in zip(stages, run["gather_bytes"][-1]):
        assert g == 0  # CPU devices share the host arrays: nothing to gather


def test_hidden_tail_on_a_multi_device_stage_is_refused(cpu):
    """State past range * epw belongs to no device's slice: make_pipeline()
    names the stage and the buffer, and takes the same buffer when it is
    read_only or the stage has one device."""
    from cekirdekler_amd.parallel.pipeline import ClPipelineStage

    src = "__global__ void k(const int* x, int* h, int* y) { long long i = get_global_id(0); y[i] = x[i] + h[i]; }"

    def stage(devs, hidden):
        s = ClPipelineStage()
        s.add_devices(devs)
        s.add_kernels(src, "k", [pm.N], [pm.L])
        s.add_input_buffers(np.zeros(pm.N, np.int32))
        s.add_hidden_buffers(hidden)
        s.add_output_buffers(np.zeros(pm.N, np.int32))
        return s

    first = stage(cpu, np.zeros(pm.N, np.int32))
    bad = stage(cpu + cpu, np.zeros(pm.N + pm.TAIL, np.int32))
    first.prepend_to_stage(bad)
    with pytest.raises(ValueError, match=r"stage 1: hidden buffer 0 has 1543 elements .* own only 1536"):
        first.make_pipeline()
    first.cruncher.dispose()
    assert bad.cruncher is None  # refused before anything was built for it
    const = ck.ClArray(np.zeros(pm.N + pm.TAIL, np.int32))
    const.read_only = True
    for s in (stage(cpu + cpu, const), stage(cpu, np.zeros(pm.N + pm.TAIL, np.int32))):
        s.make_pipeline().dispose()
    assert not const.gather_resident


def test_multi_device_stage_marks_what_it_keeps_coherent(cpu):
    case = pm.case_named("two-kernel-2-3").on_cpu()
    pipe, stages = pm.build_pipeline(case, lambda ch: cpu)
    try:
        for s in stages:
            many = len(s.devices) > 1
            assert many
            assert all(a.gather_resident for a in s.outputs + s._out_dup)
            assert [a.gather_resident for a in s.hiddens] == [not a.read_only for a in s.hiddens]
            assert not any(a.gather_resident for a in s.inputs + s._in_dup)
        assert any(a.read_only for a in stages[1].hiddens)
    finally:
        pipe.dispose()
    pipe, stages = pm.build_pipeline(case.single(), lambda ch: cpu)
    try:
        assert not any(a.gather_resident for s in stages for a in s.outputs + s._out_dup + s.hiddens)
    finally:
        pipe.dispose()


def test_push_data_keeps_copied_inputs_alive_until_the_copies_are_done(cpu):
    """A list or a strided view is copied into a temporary ClArray whose
    memory an asynchronous copy reads: the pipeline holds it until after the
    engine's sync, and lets go of it then."""
    import weakref

    from cekirdekler_amd import arrays

    case = pm.case_named("init-2-3").on_cpu()
    pipe, stages = pm.build_pipeline(case, lambda ch: cpu)
    made, held_at_sync = [], []
    real_sync = pipe.engine.sync

    class Engine:  # the engine, with a look at the wrappers at sync time
        def __getattr__(self, name):
            return getattr(pipe_engine, name)

        def sync(self):
            held_at_sync.append([r() is not None for r in made])
            real_sync()

    pipe_engine = pipe.engine
    pipe.engine = Engine()
    real = arrays.ClArray.__init__

    def spy(self, *a, **k):
        real(self, *a, **k)
        made.append(weakref.ref(self))

    arrays.ClArray.__init__ = spy
    try:
        pipe.push_data(pm.make_data(case, 0), None)
    finally:
        arrays.ClArray.__init__ = real
        pipe.engine = pipe_engine
    try:
        assert len(made) == 1 and held_at_sync == [[True]]
        assert made[0]() is None  # dropped once the push is over
    finally:
        pipe.dispose()


# ------------------------------------------------------------------ DevicePipeline


@pytest.mark.parametrize("fault", pm.DP_FAULTS)
def test_device_pipeline_fault_is_rejected(fault):
    dtype = pm.TYPES[pm.DP_FAULT_CASES[fault]][1]
    good, bad = pm.run_dp_model(dtype), pm.run_dp_model(dtype, faults=[fault])
    assert any(not np.array_equal(g, b) for g, b in zip(good, bad)), fault


def test_device_pipeline_model_stop_freezes_the_inputs_on_a_gpu_only():
    dtype = np.int32
    stopped, running = pm.run_dp_model(dtype, "gpu", stop=True), pm.run_dp_model(dtype, "gpu", stop=False)
    lag = 3  # a value written before feed f leaves at feed f + 3
    for f in range(pm.DP_FEEDS):
        same = np.array_equal(stopped[f], running[f])
        assert same == (f <= pm.DP_STOP_AFTER + lag - 1), f
    # a CPU device computes in host memory: the writes still arrive
    for a, b in zip(pm.run_dp_model(dtype, "cpu", stop=True), pm.run_dp_model(dtype, "cpu", stop=False)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("type_name", ["int", "uchar"])
def test_device_pipeline_on_the_cpu_device_equals_the_model(type_name, cpu):
    want = pm.run_dp_model(pm.TYPES[type_name][1], "cpu")
    for mode in pm.DP_MODES:
        got = pm.run_dp_real(cpu, type_name, mode)
        for f, (g, w) in enumerate(zip(got, want)):
            bad = np.flatnonzero(g != w)
            assert not len(bad), f"{mode}, feed {f}, element {bad[0]}: got {g[bad[0]]}, want {w[bad[0]]}"
