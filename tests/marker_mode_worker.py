"""Child of test_gpu_marker_modes.py: enqueue-mode computes with fine-grained
queue control on one GPU, on the main stream and on two async queues.  The
marker mode (events, or CEK_MARKERS=writevalue) is read when the worker is
built, so the parent sets it in this process's environment.  Prints one JSON
line; exit code 0 = every check held."""
import json
import os
import sys

import numpy as np

import cekirdekler_amd as ck

N = 4096
COMPUTES = 6
SRC = "__global__ void step(int* x) { long long i = get_global_id(0); x[i] = x[i] * 3 + (int)i; }"


def main() -> int:
    gpus = ck.ClPlatforms.all().gpus()
    if len(gpus) == 0:
        print(json.dumps({"error": "no GPU visible"}))
        return 2
    want = np.arange(N, dtype=np.int32)
    for _ in range(COMPUTES):
        want = want * np.int32(3) + np.arange(N, dtype=np.int32)
    out = {"markers": os.environ.get("CEK_MARKERS", ""), "runs": []}
    ok = True
    for async_enqueue in (False, True):
        cr = ck.ClNumberCruncher(gpus[0], SRC, queue_concurrency=2)
        assert cr.error_code() == 0, cr.error_message()
        x = ck.ClArray(np.arange(N, dtype=np.int32))
        cr.fine_grained_queue_control = True
        cr.enqueue_mode_async_enable = async_enqueue
        cr.enqueue_mode = True
        for _ in range(COMPUTES):
            x.compute(cr, 1, "step", N, 256)
        cr.enqueue_mode = False  # flushes: drains every queue
        cr.enqueue_mode_async_enable = False
        cr.fine_grained_queue_control = False
        run = {"async": async_enqueue, "exact": bool(np.array_equal(x.array, want)),
               "issued": int(cr.cores.markers_issued()), "reached": cr.count_markers_reached()}
        ok = ok and run["exact"] and run["reached"] == run["issued"] >= COMPUTES
        out["runs"].append(run)
        cr.dispose()
    out["ok"] = ok
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
