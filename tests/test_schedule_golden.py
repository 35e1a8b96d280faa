"""The recorded pipeline schedules, tuple for tuple, against fixtures recorded
before the pipelines moved onto one ordering primitive (csrc/cores_run.cpp,
`Ordering`): that refactor may not change a single logged operation.

Every case runs on a fresh cruncher with an explicit queue concurrency (so
GPU_MAX_HW_QUEUES cannot alter the log) and looks at the first compute() only
(the deterministic equal split).  The result is checked against numpy, then
`cores.schedule()`, grouped by device (the device threads append concurrently:
only the per-device order is defined), is compared with
tests/golden/schedules/<case>.json, on the GPU tier with gpu_<case>.json.

    python tests/test_schedule_golden.py --record

writes the fixtures of the tiers this machine can run.  They record what the
code did before a change: never regenerate them from the code under test.

Explicit blobs need one device holding the whole range; split over two devices
(the explicit_* cases) the call takes the plain path, which logs nothing, and
that empty log is what their fixtures pin.  The explicit1_* cases run the same
calls on one device, where the explicit-blob pipeline itself is recorded.
"""
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "schedules")

PLAIN = "__global__ void k(const float* x, float* y) { long long i = get_global_id(0); y[i] = x[i] * 2.0f; }"
# w: per-blob panels of L elements (explicit blob slices)
PANEL = """__global__ void k(const float* x, const float* w, float* y) {
  long long i = get_global_id(0); y[i] = x[i] * 2.0f + w[i % %L%]; }"""
# f: a full-`read` array; z: a `write_all` array that every device fills whole
# (all writers of z[j] store the same value)
FULL = """__global__ void k(const float* x, const float* f, float* y, float* z) {
  long long i = get_global_id(0); y[i] = x[i] * 2.0f + f[i % %L%]; z[i % %L%] = f[i % %L%] * 3.0f; }"""

EVENT, DRIVER = True, False  # ck.PIPELINE_EVENT / ck.PIPELINE_DRIVER

# name: (kernel, pipeline type, blobs, devices, queue concurrency, layout)
CASES = {
    "event_b4": (PLAIN, EVENT, 4, 2, 3, {}),
    "event_b3": (PLAIN, EVENT, 3, 2, 3, {}),
    "event_b8": (PLAIN, EVENT, 8, 2, 3, {}),
    "event_reads_own_stream": (PLAIN, EVENT, 4, 2, 3, {"pipeline_reads_on_main_stream": False}),
    "event_writes_one_stream": (PLAIN, EVENT, 4, 2, 3, {"pipeline_writes_one_stream": True}),
    "event_writes_on_compute_stream": (PLAIN, EVENT, 4, 2, 3, {"pipeline_writes_on_compute_stream": True}),
    "explicit_two_reads": (PANEL, EVENT, None, 2, 3, {"pipeline_reads_two_streams": True}),
    "explicit": (PANEL, EVENT, None, 2, 3, {"pipeline_reads_two_streams": False}),
    "explicit_reads_own_stream": (PANEL, EVENT, None, 2, 3, {"pipeline_reads_on_main_stream": False}),
    "explicit1_two_reads": (PANEL, EVENT, None, 1, 3, {"pipeline_reads_two_streams": True}),
    "explicit1": (PANEL, EVENT, None, 1, 3, {"pipeline_reads_two_streams": False}),
    "explicit1_reads_own_stream": (PANEL, EVENT, None, 1, 3, {"pipeline_reads_on_main_stream": False}),
    "driver_q3": (PLAIN, DRIVER, 8, 2, 3, {"driver_reads_on_main_stream": True}),
    "driver_q1": (PLAIN, DRIVER, 8, 2, 1, {}),
    "driver_downloads_in_queue": (PLAIN, DRIVER, 8, 2, 3, {"driver_downloads_own_stream": False}),
    "driver_reads_in_queue": (PLAIN, DRIVER, 8, 2, 3, {"driver_reads_on_main_stream": False}),
    "event_full_write_all": (FULL, EVENT, 4, 2, 3, {}),
    "driver_full_write_all": (FULL, DRIVER, 8, 2, 3, {}),
}


def record(case, device, L):
    """Run `case` on copies of `device` with local size L, check the result
    and return the schedule as {device index: [[op, stream, begin, count, event], ...]}."""
    import cekirdekler_amd as ck

    src, ptype, blobs, ndev, qc, layout = CASES[case]
    devices = device
    for _ in range(ndev - 1):
        devices = devices + device
    cr = ck.ClNumberCruncher(devices, src.replace("%L%", str(L)), queue_concurrency=qc)
    assert cr.error_code() == 0, cr.error_message()
    cr.cores.record_schedule = True
    for k, v in layout.items():
        setattr(cr.cores, k, v)
    if blobs is None:  # explicit blobs of 1, 3, 5 and 7 work-groups
        blobs = [0, L, 4 * L, 9 * L, 16 * L]
        n = blobs[-1]
    else:
        n = L * blobs * 2 * 4
    x = ck.ClArray(np.arange(n, dtype=np.float32))
    x.partial_read = True
    x.write = False
    y = ck.ClArray(np.zeros(n, np.float32))
    y.read = False
    want = 2 * x.array
    params = [y]
    if src is PANEL:
        w = ck.ClArray(np.arange(4 * L, dtype=np.float32))  # blob k uploads panel k
        w.partial_read = True
        w.write = False
        w.blob_slices = [(L * k, L) for k in range(4)]
        params = [w, y]
        want = want + w.array[np.arange(n) % L]
    elif src is FULL:
        f = ck.ClArray(np.arange(L, dtype=np.float32) + 1)
        f.write = False
        z = ck.ClArray(np.zeros(L, np.float32))
        z.read = False
        z.write_all = True
        params = [f, y, z]
        want = want + f.array[np.arange(n) % L]
    x.next_param(*params).compute(cr, 1, "k", n, L, 0, True, ptype, blobs)
    np.testing.assert_array_equal(y.array, want)
    if src is FULL:
        np.testing.assert_array_equal(z.array, 3 * f.array)
    sched = cr.cores.schedule()
    cr.dispose()
    by_dev = {}
    for dev, op, stream, begin, count, event in sched:
        by_dev.setdefault(str(dev), []).append([op, stream, begin, count, event])
    return by_dev


def fixture(case, prefix=""):
    return os.path.join(GOLDEN, prefix + case + ".json")


def check(case, device, L, prefix):
    got = record(case, device, L)
    with open(fixture(case, prefix)) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    for dev in want:
        assert got[dev] == want[dev], f"device {dev}"


@pytest.mark.parametrize("case", sorted(CASES))
def test_schedule_matches_fixture_cpu(case):
    import cekirdekler_amd as ck

    check(case, ck.ClPlatforms.all().cpus(True), 64, "")


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_schedule_matches_fixture_gpu(case):
    import cekirdekler_amd as ck

    check(case, ck.ClPlatforms.all().gpus()[0], 256, "gpu_")


def _record_all():
    import cekirdekler_amd as ck

    os.makedirs(GOLDEN, exist_ok=True)
    tiers = [("", ck.ClPlatforms.all().cpus(True), 64)]
    gpus = ck.ClPlatforms.all().gpus()
    if len(gpus) > 0:
        tiers.append(("gpu_", gpus[0], 256))
    for prefix, device, L in tiers:
        for case in sorted(CASES):
            with open(fixture(case, prefix), "w") as f:
                json.dump(record(case, device, L), f, separators=(",", ":"))
                f.write("\n")
            print("recorded", os.path.relpath(fixture(case, prefix)))


if __name__ == "__main__":
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_schedule_golden.py --record")
    _record_all()
