"""Both marker modes of the worker on a GPU.  The mode is read from
CEK_MARKERS when a worker is built: event markers by default (covered all
over the suite), hipStreamWriteValue64 into pinned words with
CEK_MARKERS=writevalue.  A fresh child process per mode runs the same
enqueue-mode computes (tests/marker_mode_worker.py); the default mode is the
control."""
import json
import os
import subprocess
import sys

import pytest

from cekirdekler_amd.utils.multigpu import child_env

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("markers", ["writevalue", ""])
def test_enqueue_mode_markers_in_both_marker_modes(markers):
    """Six enqueue-mode computes of a 4096-element integer kernel on the main
    stream, then on two async queues: exact results, and after the flush
    every issued marker is reached."""
    env = child_env()
    env.pop("CEK_MARKERS", None)
    if markers:
        env["CEK_MARKERS"] = markers
    r = subprocess.run([sys.executable, os.path.join(HERE, "marker_mode_worker.py")], cwd=HERE, env=env,
                       capture_output=True, text=True, timeout=120)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = json.loads(lines[-1])
    assert out["ok"] and out["markers"] == markers, out
    assert [run["async"] for run in out["runs"]] == [False, True]
    for run in out["runs"]:
        assert run["exact"], out
        assert run["reached"] == run["issued"] >= 6, out
