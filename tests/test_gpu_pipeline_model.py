"""GPU tier of the pipeline model (tests/pipeline_model.py).

Every case runs three times: on the coherent emulator (the oracle), on a real
ClPipeline with every stage on one device, and on a real ClPipeline whose
stages span logical devices of GPU 0 (``g0 + g0 + g0``; one case GPU + CPU).
All three must agree in every push: the ready flag and every element of every
result.  A logical device has replicas of its own, so what one device wrote
and another reads has to travel: this tier sees incoherence between replicas,
which the CPU tier cannot.

The splits are forced (``cores.set_state`` per compute id before every push,
one device slowed with ``set_time_scale``), read back after the push and
handed to the per-device model, which then also gives the bytes each path
must have moved.  A case asserts its own preconditions: the split of every
multi-device stage moved, the two kernels of a two-kernel stage split
differently, and no device stayed idle.

The DevicePipeline case runs on GPU 0, where the stages run on streams of
their own: every feed mode against the parity emulator, feed by feed.
"""
import numpy as np
import pytest

import cekirdekler_amd as ck
import pipeline_model as pm
from cekirdekler_amd._native import cek

pytestmark = pytest.mark.gpu

CASES = pm.cases()


def _device_of():
    plats = ck.ClPlatforms.all()
    g0, cpu = plats.gpus()[0], plats.cpus(True)
    return lambda ch: g0 if ch == "g" else cpu


def _force_splits(case):
    """Before push p: every compute id of every multi-device stage starts
    from the synthetic split of that push (the balancer takes it from
    there), and the last device is the slow one."""
    def before(p, stages):
        want = pm.synthetic_splits(case, p)
        for si, s in enumerate(stages):
            D = len(s.devices)
            if D == 1:
                continue
            if p == 0:
                s.cruncher.set_time_scale(D - 1, 2.0)
            for k in range(len(s.kernel_names)):
                s.cruncher.cores.set_state(1 + k, want[si][k][0], [[0.0] * D for _ in range(10)], [1.0] * D)
    return before


def _run(case, forced=True):
    pipe, stages = pm.build_pipeline(case, _device_of())
    try:
        return pm.run_pipeline(case, pipe, stages, _force_splits(case) if forced else None)
    finally:
        pipe.dispose()


def _check_preconditions(case, run):
    for si, s in enumerate(case.stages):
        D = len(s.devices)
        if D == 1:
            continue
        per_push = [sp[si] for sp in run["splits"]]
        for kernels in per_push:
            for ranges, refs in kernels:
                assert sum(ranges) == pm.N and refs == [sum(ranges[:d]) for d in range(D)], (ranges, refs)
        assert len({tuple(k[0][0]) for k in per_push}) > 1, f"stage {si}: the split never moved"
        if len(per_push[0]) > 1:
            assert any(k[0][0] != k[1][0] for k in per_push), f"stage {si}: compute ids 1 and 2 always split alike"
        for d in range(D):
            assert any(r[d] > 0 for k in per_push for r, _ in k), f"stage {si}: device {d} never computed"


def _check(case, engine_note=""):
    multi = _run(case)
    single = _run(case.single(), forced=False)
    pm.check_against_oracle(case, single["seen"], "every stage on one device" + engine_note)
    pm.check_against_oracle(case, multi["seen"], f"stages on {[s.devices for s in case.stages]}" + engine_note)
    _check_preconditions(case, multi)
    # the bytes each path moved, push by push: the per-device model with the splits the pipeline reported
    model = pm.run_model(case, splits_of=lambda c, p: multi["splits"][p])
    assert pm.first_difference(model, pm.run_model(case, coherent=True)) is None
    for p, (got, want) in enumerate(zip(multi["seen"], model)):
        assert got[2] == want[2], f"push {p}: transfer_stats {got[2]}, the model expects {want[2]}"
    if all(s.devices.count("c") == 0 for s in case.stages):
        item, P = case.dtype.itemsize, case.pushes
        plan = pm.push_plan(case)
        first_in = sum(b.n for b in pm.buffers_of(case.stages[0]) if b.role == "in")
        outs = sum(b.n for b in pm.buffers_of(case.stages[-1]) if b.role == "out")
        last = multi["seen"][-1][2]
        assert last["host"] == 0
        assert last["h2d"] == sum(d for d, _ in plan) * len(case.stages[0].devices) * first_in * item
        assert last["d2h"] == sum(r for _, r in plan) * outs * item
        assert (last["p2p"] > 0) == (len(case.stages) > 1)
    # a single-device stage gathers nothing; a multi-device stage gathers what its last kernel may write
    assert all(g == 0 for per_push in single["gather_bytes"] for g in per_push)
    for si, s in enumerate(case.stages):
        D = len(s.devices)
        if s.kind == "join" and D > 1 and "c" not in s.devices:
            # y alone: the read_only constant and the inputs are not gathered
            assert {per_push[si] for per_push in multi["gather_bytes"]} == {(D - 1) * pm.N * case.dtype.itemsize}
        elif D > 1:
            assert all(per_push[si] > 0 for per_push in multi["gather_bytes"])
    return multi


def test_case_list_is_the_cpu_tiers():
    assert [c.name for c in CASES] == [c.name for c in pm.cases()] and len(CASES) >= 7
    assert set(pm.FAULT_CASES.values()) <= {c.name for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=str)
def test_one_device_and_multi_device_pipelines_equal_the_oracle(case):
    _check(case)


def test_unaligned_group_records_through_the_copy_kernel_engine():
    """The uchar case whose per-group record is 7 bytes, with the copy-kernel
    engine forced for the transitions and the gather."""
    cek.set_copy_engine_override(1)
    try:
        _check(pm.case_named("two-kernel-3-1-2"), " (copy-kernel engine)")
    finally:
        cek.set_copy_engine_override(-1)


@pytest.mark.parametrize("type_name", ["int", "uchar"])
def test_device_pipeline_feed_modes_equal_the_model(type_name):
    g0 = ck.ClPlatforms.all().gpus()[0]
    want = pm.run_dp_model(pm.TYPES[type_name][1], "gpu")
    for mode in pm.DP_MODES:
        got = pm.run_dp_real(g0, type_name, mode)
        for f, (g, w) in enumerate(zip(got, want)):
            bad = np.flatnonzero(g != w)
            assert not len(bad), f"{mode}, feed {f}, element {bad[0]}: got {g[bad[0]]}, want {w[bad[0]]}"


def test_device_pipeline_without_stop_equals_the_model():
    g0 = ck.ClPlatforms.all().gpus()[0]
    want = pm.run_dp_model(np.int64, "gpu", stop=False)
    got = pm.run_dp_real(g0, "llong", "parallel", stop=False)
    for f, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), f"feed {f}"
