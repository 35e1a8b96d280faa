"""GPU tier of the transfer model (tests/transfer_model.py): compute() on
logical duplicates of GPU 0 (g, g+g, g+g+g) and on g+cpu equals the model,
call by call: every element of every host array, both byte counts and the
path taken.  Every flag combination runs on the plain path for all four
element types; the other paths, the epw/epg families, the mid-sequence flag
changes, the clipped slices and the work-item functions run with ``int``.

The read fan-out is off and every array is far below peer_read_min_bytes, so
h2d_bytes means host-to-device copies only (run_case also asserts that no
byte was staged and that the device-to-device bytes are the gather's alone).

Left out on g+cpu, with the reason: graph capture (refused with a CPU
device), and ``late-read-inplace`` (a CPU device has no replica: its kernel
writes its slice of the host array while the GPU uploads that array whole, so
what the GPU's replica holds outside its own slice is not defined, and that
case looks at it one call later).
"""
import numpy as np
import pytest

import cekirdekler_amd as ck
import transfer_model as tm

pytestmark = pytest.mark.gpu

SETS = {"g": ["gpu"], "g+g": ["gpu", "gpu"], "g+g+g": ["gpu", "gpu", "gpu"], "g+cpu": ["gpu", "cpu"]}

_current = {}  # one cruncher alive at a time: (set, type) -> backend


def _backend(set_name: str, type_name: str) -> tm.CruncherBackend:
    key = (set_name, type_name)
    if key not in _current:
        _dispose()
        plats = ck.ClPlatforms.all()
        g, cpu = plats.gpus()[0], plats.cpus(True)
        devs = None
        for kind in SETS[set_name]:
            one = g if kind == "gpu" else cpu
            devs = one if devs is None else devs + one
        cr = ck.ClNumberCruncher(devs, tm.probe_source(tm.TYPES[type_name][0]))
        assert cr.error_code() == 0, cr.error_message()
        cr.peer_reads = False
        _current[key] = (cr, tm.CruncherBackend(cr, SETS[set_name]))
    return _current[key][1]


def _dispose() -> None:
    for cr, _ in _current.values():
        cr.dispose()
    _current.clear()


@pytest.fixture(scope="module", autouse=True)
def _crunchers():
    yield
    _dispose()


def _run(set_name: str, type_name: str, case: tm.Case) -> dict:
    kinds = SETS[set_name]
    return tm.run_case(case, _backend(set_name, type_name), kinds, tm.TYPES[type_name][1])


def _allowed(set_name: str, case: tm.Case) -> bool:
    return set_name != "g+cpu" or (case.path != "graph" and case.name != "late-read-inplace")


# grouped by (device set, type) so that each cruncher is built once
FLAG_RUNS = [(s, t, c) for s in SETS for t in tm.TYPES for c in tm.flag_cases()]
INT_CASES = tm.path_cases() + tm.epw_cases() + tm.epg_cases() + tm.late_cases() + tm.clip_cases()
INT_RUNS = [(s, c) for s in SETS for c in INT_CASES if _allowed(s, c)]
IDS_RUNS = [(s, c) for s in SETS for c in tm.ids_cases() if _allowed(s, c)]


@pytest.mark.parametrize("set_name,type_name,case", FLAG_RUNS, ids=lambda v: str(v))
def test_every_flag_combination_on_the_plain_path(set_name, type_name, case):
    _run(set_name, type_name, case)


@pytest.mark.parametrize("set_name,case", INT_RUNS, ids=lambda v: str(v))
def test_paths_epw_epg_and_flag_changes(set_name, case):
    _run(set_name, "int", case)


@pytest.mark.parametrize("set_name,case", IDS_RUNS, ids=lambda v: str(v))
def test_work_item_functions(set_name, case):
    tm.check_ids(_run(set_name, "int", case), case, len(SETS[set_name]))


@pytest.mark.parametrize("set_name", ["g", "g+g+g"])
def test_repeat_kernel_launch_shape(set_name):
    tm.check_repeat_kernel_shape(_backend(set_name, "int").cr)


def test_zero_copy_is_taken_as_zero_copy_on_the_gpu():
    """The zero-copy cases are not silently copied cases: the native spec of
    a pinned array keeps the flag."""
    a = ck.ClArray(256, np.int32)
    a.zero_copy = True
    assert a._spec().zc
    a.dispose()
