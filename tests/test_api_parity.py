"""Reference API members that are not compute paths: ClArray's IList<T>
members (NotImplementedException stubs in ClArray.cs:1105-1353; read-only
queries work here, size changes are refused) and the usage-type-2 Cores
mode switches / error state (Cores.cs:80-140)."""
import json
import os

import numpy as np
import pytest

import cekirdekler_amd as ck

GOLDEN_API = os.path.join(os.path.dirname(__file__), "golden", "cores_api.json")


def cores_api_state() -> dict:
    """The public names of every class the native extension exports, and the
    plain bool / int / float attributes of a fresh CPU-device Cores."""
    from cekirdekler_amd._native import cek

    classes = {name: sorted(a for a in dir(obj) if not a.startswith("_"))
               for name, obj in sorted(vars(cek).items()) if isinstance(obj, type)}
    c = ck.Cores("cpu", "__global__ void k(float* a) { a[get_global_id(0)] += 1.0f; }", ["k"])
    native = c.cruncher._cores
    defaults = {}
    for a in classes["Cores"]:
        if a == "build_ms":  # a measurement, not a default
            continue
        v = getattr(native, a)
        if type(v) in (bool, int, float):
            defaults[a] = v
    c.dispose()
    return {"classes": classes, "cores_defaults": defaults}


def test_native_api_is_pinned():
    """The scheduler was split into owning parts behind an unchanged API:
    tests/golden/cores_api.json was written by this function from the
    extension built at the commit before the split, and the built extension
    must still export exactly those names and defaults."""
    with open(GOLDEN_API) as f:
        want = json.load(f)
    got = cores_api_state()
    assert sorted(got["classes"]) == sorted(want["classes"])
    for name in want["classes"]:
        assert got["classes"][name] == want["classes"][name], name
    assert got["cores_defaults"] == want["cores_defaults"]


def test_clarray_list_queries():
    a = ck.ClArray(np.array([1, 2, 3, 2], np.float32))
    assert list(a) == [1, 2, 3, 2]
    assert 2 in a and 7 not in a
    assert a.Contains(3) and not a.contains(9)
    assert a.IndexOf(2) == 1 and a.index_of(9) == -1
    assert a.IsReadOnly is False
    for op in (lambda: a.Add(1), lambda: a.Insert(0, 1), lambda: a.Remove(1), lambda: a.RemoveAt(0),
               lambda: a.Clear()):
        with pytest.raises(NotImplementedError):
            op()
    assert len(a) == 4
    b = ck.ClArray(16, np.float32)  # pinned native array
    b.array[:] = np.arange(16)
    assert b.IndexOf(5) == 5 and list(b)[:3] == [0, 1, 2]


def test_cores_usage_type_2_modes_and_errors():
    src = "__global__ void k(float* a) { a[get_global_id(0)] += 1.0f; }"
    c = ck.Cores("cpu", src, ["k"])
    assert c.errorCode() == 0 and c.errorMessage() == "" and c.allErrorsString == ""
    assert c.smoothLoadBalancer is True
    for name in ("enqueueMode", "enqueueModeAsyncEnable", "fineGrainedQueueControl", "noComputeMode"):
        assert getattr(c, name) is False
    a = ck.ClArray(np.zeros(256, np.float32))
    c.enqueueMode = True
    assert c.cruncher.enqueue_mode
    for _ in range(3):
        c.compute("k", 1, "", [a], ["read write"], [1], 256, 1)
    c.enqueueMode = False  # drains
    np.testing.assert_array_equal(a.array, 3.0)
    c.noComputeMode = True
    c.compute("k", 1, "", [a], ["read write"], [1], 256, 1)
    c.noComputeMode = False
    np.testing.assert_array_equal(a.array, 3.0)  # no kernel ran
    c.dispose()


def test_cluster_balancer_reference_call_shapes():
    """ClusterLoadBalancer.dengeleEsit / balanceOnPerformances / obeb / okek
    (ClusterLoadBalancer.cs:72-330): ranges filled in place, the mainframe's
    remainder returned."""
    from cekirdekler_amd.parallel.balancer import ClusterLoadBalancer

    cb = ClusterLoadBalancer()
    assert cb.obeb(256, 768) == 256 and cb.okek([256, 768]) == 768
    r = [0, 0]
    rem = cb.dengeleEsit(10 * 768, r, [256, 768])
    assert sum(r) + rem == 10 * 768 and r == cb.tmpMenziller
    new, rem_t = cb.balance([10.0, 5.0], 10 * 768, list(r), [256, 768])
    rem2 = cb.balanceOnPerformances([10.0, 5.0], 10 * 768, r, [256, 768])
    assert r == new and rem2 == rem_t and r[1] > r[0]
    assert cb.tmpHizlar is not None and len(cb.tmpHizlar) == 2


def test_native_array_copy_to_from_index():
    """FastArr.CopyTo_ / CopyFrom_ (CSpaceArrays.cs:710-740): elements
    [index, N) between equal-length native arrays."""
    a, b = ck.ClFloatArray(8), ck.ClFloatArray(8)
    a.array[:] = np.arange(8)
    b.array[:] = -1
    a.CopyTo_(b, 3)
    np.testing.assert_array_equal(b.array, [-1, -1, -1, 3, 4, 5, 6, 7])
    b.CopyFrom_(a, 0)
    np.testing.assert_array_equal(b.array, np.arange(8))
    with pytest.raises(ValueError):
        a.CopyTo_(ck.ClFloatArray(4), 0)
