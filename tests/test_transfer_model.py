"""CPU tier of the transfer model (tests/transfer_model.py).

1. The honest emulator, over GPU-kind devices, passes every sequence against
   itself (the harness, the case generators and the synthetic partitions are
   sound, and every sequence changes its partition).
2. Every fault the emulator can be given is rejected by a named case
   (FAULT_CASES): a runtime with that single rule wrong would fail that test
   of the GPU tier.  All but one are rejected on the data alone, with the byte
   counts not looked at.
3. The real runtime on 1, 2 and 3 CPU devices equals the model over CPU-kind
   devices on every sequence and path the CPU device supports (all but graph
   capture): work-item ids, epw/epg slices, offsets, pipelines, repeat,
   enqueue modes and the byte accounting, which a CPU device shares with a GPU.
4. The model's flag rules are those of ClArray's setters.
"""
import numpy as np
import pytest

import cekirdekler_amd as ck
import transfer_model as tm

ALL_CASES = (tm.flag_cases() + tm.epw_cases() + tm.epg_cases() + tm.path_cases() + tm.late_cases() + tm.clip_cases()
             + tm.ids_cases())
CPU_CASES = [c for c in ALL_CASES if c.path != "graph"]
BY_NAME = {c.name: c for c in ALL_CASES}

# fault -> (the case that rejects it, whether only the byte counts can show it)
FAULT_CASES = {
    "partial_uploads_all": ("flags-partial-write", False),
    "partial_no_epw": ("flags-partial-write", False),
    "partial_prev_ranges": ("flags-partial-neither", False),
    "partial_shift_group": ("flags-partial-write_all", False),
    "read_skipped": ("flags-read-write", False),
    "read_when_off": ("flags-neither-write", False),
    "read_wins_over_partial": ("flags-both-write", False),
    "write_whole_replica": ("flags-partial-write", False),
    "write_no_epw": ("flags-partial-write", False),
    "download_without_write": ("flags-partial-neither", False),
    "write_all_owner0": ("flags-partial-write_all", False),
    "write_all_without_write": ("flags-partial-all_alone", False),
    "write_all_slices": ("flags-neither-write_all", False),
    "epg_as_epw": ("epg-2x2", False),
    "epg_from_ref": ("epg-2x2-offset", False),
    "offset_dropped_slices": ("epw-2-3", False),
    "offset_dropped_ids": ("ids-plain-128", False),
    "zero_copy_copied": ("flags-zero_copy-zero_copy", False),
    "no_phase_separation": ("late-read-inplace", False),
    "gather_missing": ("flags-partial-gather", False),
    "gather_dev0_only": ("late-partial-gather", False),
    "zero_range_transfers": ("late-read-inplace", False),
    "repeat_reuploads": ("repeat-both-inplace", False),
    "bytes_by_epw": ("epw-2-3", True),
    "gather_before_downloads": ("flags-partial-all_gather", False),
}


def test_case_names_are_unique_and_sizes_stay_small():
    assert len(BY_NAME) == len(ALL_CASES)
    for c in ALL_CASES:
        plan = tm.Plan(c, 3, np.int64)
        assert plan.G <= 1536
        if c.kernel != "ids":
            assert max(h.nbytes for h in plan.hosts) < 40 * 1024, c.name


def test_every_flag_set_and_dimension_is_generated():
    flags = {(c.src, c.dst) for c in tm.flag_cases()}
    assert flags == {(s, d) for s in tm.SRC_FLAGS for d in tm.DST_FLAGS}
    assert {(c.E, c.F) for c in tm.epw_cases()} == {(e, f) for e in (1, 2, 3) for f in (1, 2, 3)}
    assert {c.offset for c in ALL_CASES} == {0, 2 * tm.L}
    assert {c.path for c in ALL_CASES} == set(tm.PATHS)
    assert {c.path for c in tm.ids_cases()} == set(tm.PATHS)
    assert any(c.tail for c in ALL_CASES) and any(c.epg for c in ALL_CASES)


@pytest.mark.parametrize("role,name", [("src", n) for n in tm.SRC_FLAGS] + [("dst", n) for n in tm.DST_FLAGS]
                         + [("dst", "observe"), ("dst", "const")])
def test_flag_rules_are_those_of_clarray(role, name):
    a = ck.ClArray(8, np.int32)
    for attr, v in tm.user_settings(role, name):
        setattr(a, attr, v)
    f = tm.flags_of(role, name)
    assert (a.read, a.partial_read, a.write, a.write_all, a.read_only, a.write_only, bool(a.zero_copy),
            bool(a.gather_resident)) == (f.read, f.partial, f.write, f.write_all, f.ro, f.wo, f.zc, f.gather)
    a.dispose()


def test_flag_exclusions_are_those_of_clarray():
    """read_only refuses write, write_all and write_only; write_only refuses
    read, partial_read and read_only; switching a hint off lifts the refusal."""
    orders = [[("read_only", True), ("write", True), ("write_all", True), ("write_only", True)],
              [("write_only", True), ("read", True), ("partial_read", True), ("read_only", True)],
              [("read_only", True), ("read_only", False), ("write", True)],
              [("write_only", True), ("write_only", False), ("partial_read", True), ("read_only", True)]]
    for order in orders:
        a, f = ck.ClArray(8, np.int32), tm.Flags()
        for attr, v in order:
            setattr(a, attr, v)
            f.assign(attr, v)
            assert (a.read, a.partial_read, a.write, a.write_all, a.read_only, a.write_only) == \
                   (f.read, f.partial, f.write, f.write_all, f.ro, f.wo), (order, attr)
        a.dispose()


# ---------------------------------------------------------------- 1. honest emulator


@pytest.mark.parametrize("case", ALL_CASES, ids=str)
def test_honest_emulator_passes_every_sequence(case):
    for D in (1, 2, 3):
        for dtype in (np.uint8, np.int32):
            kinds = ["gpu"] * D
            res = tm.run_case(case, tm.EmulatorBackend(kinds), kinds, dtype)
            assert D == 1 or len(set(res["ranges"])) >= 2
            if case.kernel == "ids":
                tm.check_ids(res, case, D)


def test_mixed_kinds_differ_from_gpu_kinds_where_they_should():
    """A CPU-kind device reads the host array itself: a resident src is stale
    on a GPU and fresh on a CPU device, and the harness tells the two apart."""
    case = BY_NAME["flags-neither-write"]
    with pytest.raises(tm.Mismatch):
        tm.run_case(case, tm.EmulatorBackend(["gpu", "cpu"]), ["gpu", "gpu"], np.int32)
    tm.run_case(case, tm.EmulatorBackend(["gpu", "cpu"]), ["gpu", "cpu"], np.int32)


# ---------------------------------------------------------------- 2. faults


def test_fault_table_is_complete():
    assert set(FAULT_CASES) == set(tm.FAULTS)
    assert all(name in BY_NAME for name, _ in FAULT_CASES.values())


@pytest.mark.parametrize("fault", tm.FAULTS)
def test_fault_is_rejected_by_its_named_case(fault):
    name, bytes_only = FAULT_CASES[fault]
    case = BY_NAME[name]
    kinds = ["gpu"] * 3
    for dtype in (np.uint16, np.int32, np.int64):
        tm.run_case(case, tm.EmulatorBackend(kinds), kinds, dtype)
        with pytest.raises(tm.Mismatch) as e:
            tm.run_case(case, tm.EmulatorBackend(kinds, [fault]), kinds, dtype, check_bytes=bytes_only)
        assert ("bytes" in str(e.value)) == bytes_only, str(e.value)


def test_only_the_byte_fault_needs_the_byte_counts():
    kinds = ["gpu"] * 3
    for case in ALL_CASES:
        tm.run_case(case, tm.EmulatorBackend(kinds, ["bytes_by_epw"]), kinds, np.int32, check_bytes=False)


# ---------------------------------------------------------------- 3. the runtime on CPU devices

_crunchers = {}


@pytest.fixture(scope="module")
def cpu_backend():
    def get(D: int, type_name: str) -> tm.CruncherBackend:
        key = (D, type_name)
        if key not in _crunchers:
            cpu = ck.ClPlatforms.all().cpus(True)
            devs = cpu
            for _ in range(D - 1):
                devs = devs + cpu
            cr = ck.ClNumberCruncher(devs, tm.probe_source(tm.TYPES[type_name][0]))
            assert cr.error_code() == 0, cr.error_message()
            _crunchers[key] = (cr, tm.CruncherBackend(cr, ["cpu"] * D))
        return _crunchers[key][1]

    yield get
    for cr, _ in _crunchers.values():
        cr.dispose()
    _crunchers.clear()


@pytest.mark.parametrize("D", (1, 2, 3))
@pytest.mark.parametrize("case", CPU_CASES, ids=str)
def test_cpu_devices_equal_the_model(cpu_backend, case, D):
    res = tm.run_case(case, cpu_backend(D, "int"), ["cpu"] * D, np.int32)
    if case.kernel == "ids":
        tm.check_ids(res, case, D)
    if case.path in ("event", "driver") and case.dst not in ("inplace", "gather"):
        assert all(r["pipelined"] for r in res["records"][1:]), "the pipeline was asked for and admitted"


@pytest.mark.parametrize("type_name", [t for t in tm.TYPES if t != "int"])
@pytest.mark.parametrize("case", [c for c in CPU_CASES if c.kernel != "ids"], ids=str)
def test_cpu_devices_equal_the_model_other_types(cpu_backend, case, type_name):
    tm.run_case(case, cpu_backend(3, type_name), ["cpu"] * 3, tm.TYPES[type_name][1])


def test_repeat_kernel_launch_shape(cpu_backend):
    tm.check_repeat_kernel_shape(cpu_backend(1, "int").cr)
    tm.check_repeat_kernel_shape(cpu_backend(3, "int").cr)


WORKED = """
__global__ void worked(const int* a, int* b, int* c) {
  const long long i = get_global_id(0);
  b[2 * i] = a[2 * i] + 1; b[2 * i + 1] = a[2 * i + 1] + 2;
  c[3 * i] = a[2 * i]; c[3 * i + 1] = b[2 * i]; c[3 * i + 2] = (int)i;
}
"""


def test_byte_counts_of_the_worked_example():
    """The figures quoted when this model was proposed, from the runtime's
    record on three CPU devices and from the model: a 1536-element
    partial_read array (write off), a default-flag array of 1536 and an
    observation array (read off), 4-byte elements, G = 512, epw 2/2/3:
    22528 bytes up, 10240 down, whatever the ranges."""
    G = 512
    cpu = ck.ClPlatforms.all().cpus(True)
    cr = ck.ClNumberCruncher(cpu + cpu + cpu, WORKED)
    assert cr.error_code() == 0, cr.error_message()
    arrays = [ck.ClArray(1536, np.int32) for _ in range(3)]
    arrays[0].array[:] = np.arange(1536)
    names = ("partial", None, "observe")
    for a, name, epw in zip(arrays, names, (2, 2, 3)):
        for attr, v in (tm.user_settings("src" if name == "partial" else "dst", name) if name else []):
            setattr(a, attr, v)
        a.elements_per_work_item = epw
    flags = [tm.flags_of("src", "partial"), tm.Flags(), tm.flags_of("dst", "observe")]
    for _ in range(2):
        cr.compute(ck.ClParameterGroup(arrays), 77, "worked", G, tm.L)
        rec = cr.last_record()
        assert (rec["h2d_bytes"], rec["d2h_bytes"]) == (22528, 10240), rec
        hosts = [np.zeros(1536, np.int32) for _ in range(3)]
        arrs = [tm.Arr(h, f, e) for h, f, e in zip(hosts, flags, (2, 2, 3))]
        for kinds in (["cpu"] * 3, ["gpu"] * 3):
            assert tm.Emulator(kinds).call(arrs, lambda *a: None, G, 0, rec["ranges"], rec["references"]) == \
                (22528, 10240)
    i = np.arange(G)
    assert np.array_equal(arrays[1].array[:2 * G:2], arrays[0].array[:2 * G:2] + 1)
    assert np.array_equal(arrays[2].array[2:3 * G:3], i)
    cr.dispose()
    for a in arrays:
        a.dispose()
