"""GPU tier of the kernel-string oracles (tests/kernel_lang.py) on the MI355X:
device-side enqueue against the queue model on every compute path, work-group
semantics and the OpenCL dialect against the models the CPU tier uses.  One
cruncher per corpus source, built once per module."""
import numpy as np
import pytest

import cekirdekler_amd as ck

import kernel_lang as kl

pytestmark = pytest.mark.gpu

LEVELS = kl.K_LEVELS - 1


@pytest.fixture(scope="module")
def gpu():
    return ck.ClPlatforms.all().gpus()


@pytest.fixture(scope="module")
def crs(gpu):
    """name -> cruncher on GPU 0; "path2" is the path source on two logical devices."""
    out = {}
    for name, src in kl.SOURCES.items():
        out[name] = ck.ClNumberCruncher(gpu[0], src)
    out["path2"] = ck.ClNumberCruncher(gpu[0] + gpu[0], kl.PATH_SRC)
    for name, c in out.items():
        assert c.error_code() == 0, (name, c.error_message())
    yield out
    for c in out.values():
        c.dispose()


@pytest.fixture(scope="module")
def threads(crs):
    """The dispatcher's thread count, from the device the runtime launches on."""
    return kl.dispatcher_threads(crs["enq"].cores.device(0).compute_units)


# ------------------------------------------------------------ part A: the queue

def run_table(cr, name, threads, levels=LEVELS, model=None):
    """One ``table`` launch of a corpus case on the GPU and under the model:
    arrays equal, and the rise of device_enqueue_errors() equal to the model's."""
    case = kl.table_case(name, threads)
    model = model or kl.QueueModel(kl.ENQ_CHILDREN)
    want, want_errors = kl.table_model(model, case, levels, threads)
    before = cr.device_enqueue_errors()
    got = kl.run(cr, 1, "table", kl.table_arrays(case), kl.ENQ_ARRAYS, case["G"], case["L"], outputs=kl.ENQ_OUTPUTS)
    rose = cr.device_enqueue_errors() - before
    print(f"{name} levels={levels}: device_enqueue_errors rose by {rose}, model {want_errors}")
    assert kl.mismatches(got, {k: want[k] for k in kl.ENQ_OUTPUTS}) == []
    assert rose == want_errors
    return got, rose


def test_three_child_levels_and_a_fourth_attempt(crs, threads):
    got, rose = run_table(crs["enq"], "levels", threads)
    assert list(got["cnt"][:4]) == [0, 48, 96, 192] and rose == 192


@pytest.mark.parametrize("name", ["kinds", "param64", "nvals", "nothing"])
def test_child_kinds_param_and_n(crs, threads, name):
    run_table(crs["enq"], name, threads)


def test_grid_stride_tail(crs, threads):
    got, _ = run_table(crs["enq"], "tail", threads)
    assert len(got["x"]) == threads + 257 and np.all(got["x"] == 1)


def test_capacity_of_a_level(crs, threads):
    """Exactly kDynCap enqueues: no error; 512 more: 512 errors and kDynCap
    children run; the next compute is exact again."""
    cr = crs["enq"]
    model = kl.QueueModel(kl.ENQ_CHILDREN)       # one model across the launches, as one queue
    got, rose = run_table(cr, "cap_exact", threads, model=model)
    assert got["cnt"][0] == kl.K_CAP + 4 and rose == 0
    got, rose = run_table(cr, "cap_over", threads, model=model)
    assert got["cnt"][0] == kl.K_CAP and rose == 512
    got, rose = run_table(cr, "few", threads, model=model)
    assert got["cnt"][0] == 3 and rose == 0


def test_set_device_enqueue_levels(crs, threads):
    cr = crs["enq"]
    try:
        for levels in range(kl.K_LEVELS):
            cr.set_device_enqueue_levels(levels)
            run_table(cr, "levels", threads, levels=levels)
        for bad in (-1, kl.K_LEVELS):
            with pytest.raises(Exception, match=r"device enqueue levels must be in \[0, %d\]" % LEVELS):
                cr.set_device_enqueue_levels(bad)
    finally:
        cr.set_device_enqueue_levels(LEVELS)


def test_parent_parameter_lists(crs, threads):
    """Arrays named like the dispatcher's own words, const __restrict__, three
    element types, two parents sharing a child, a kernel that enqueues nothing."""
    cr = crs["names"]
    G, L = 512, 64
    A = kl.names_arrays(G)
    want = {k: v.copy() for k, v in A.items()}
    before = cr.device_enqueue_errors()
    for cid, kernel in enumerate(("pa", "pb", "plain"), 1):
        errors = kl.QueueModel(kl.NAMES_CHILDREN).launch(kl.NAMES_PARENTS[kernel], want, 0, G, L, LEVELS, threads)
        assert errors == 0
        A = kl.run(cr, cid, kernel, A, kl.NAMES_ARRAYS, G, L, outputs=kl.NAMES_ARRAYS[1:])
        assert kl.mismatches(A, want) == [], kernel
    assert cr.device_enqueue_errors() - before == 0


def test_dialect_parent(crs):
    G, L = 512, 64
    got = kl.run(crs["dialect_enq"], 1, "dpar", {"x": np.arange(G, dtype=np.int32)}, ("x",), G, L, outputs=("x",))
    assert kl.mismatches(got, {"x": np.arange(G, dtype=np.int32) + 5}) == []
    assert crs["dialect_enq"].device_enqueue_errors() == 0


# ------------------------------------------------------------ part A: the paths

G_PATH, L_PATH = 4096, 256


def path_input():
    return np.random.default_rng(41).integers(-50, 50, G_PATH).astype(np.int32)


def check_path(cr, x, x0, ranges, launches, threads, before):
    want, want_errors = kl.lead_model(x0, ranges, L_PATH, launches, threads)
    rose = cr.device_enqueue_errors() - before
    print(f"ranges {list(ranges)}, {launches} launches: errors rose by {rose}, model {want_errors}")
    assert kl.mismatches({"x": x}, {"x": want}) == []
    assert rose == want_errors == 0


def test_path_two_logical_devices(crs, threads):
    cr = crs["path2"]
    x0 = path_input()
    x = ck.ClArray(x0.copy())
    before = cr.device_enqueue_errors()
    for call in range(3):                      # the balancer moves the split between calls
        x.compute(cr, 1, "lead", G_PATH, L_PATH)
        ranges = cr.ranges(1)
        assert len(ranges) == 2 and sum(ranges) == G_PATH
        check_path(cr, x.array, x0, ranges, call + 1, threads, before)


def test_path_enqueue_mode(crs, threads):
    cr = crs["path"]
    x0 = path_input()
    x = ck.ClArray(x0.copy())
    before = cr.device_enqueue_errors()
    x.compute(cr, 2, "lead", G_PATH, L_PATH)
    x.read = False                             # device-resident inside the batch
    cr.enqueue_mode = True
    for _ in range(3):
        x.compute(cr, 2, "lead", G_PATH, L_PATH)
    cr.enqueue_mode = False
    check_path(cr, x.array, x0, [G_PATH], 4, threads, before)


def test_path_async_enqueue_several_in_flight(crs, threads):
    """Queues are per stream: computes in flight on different streams do not
    share level counts."""
    cr = crs["path"]
    x0 = path_input()
    xs = [ck.ClArray(x0 + k) for k in range(4)]
    before = cr.device_enqueue_errors()
    cr.enqueue_mode = True
    cr.enqueue_mode_async_enable = True
    try:
        for k, x in enumerate(xs):
            x.compute(cr, 10 + k, "lead", G_PATH, L_PATH)
    finally:
        cr.enqueue_mode = False
        cr.enqueue_mode_async_enable = False
    for k, x in enumerate(xs):
        check_path(cr, x.array, x0 + k, [G_PATH], 1, threads, before)


@pytest.mark.parametrize("ptype", [ck.PIPELINE_EVENT, ck.PIPELINE_DRIVER])
def test_path_pipelines_with_four_blobs(crs, threads, ptype):
    cr = crs["path"]
    x0 = path_input()
    x = ck.ClArray(x0.copy())
    x.partial_read = True
    before = cr.device_enqueue_errors()
    x.compute(cr, 20 + int(ptype), "lead", G_PATH, L_PATH, pipeline=True, pipeline_type=ptype, pipeline_blobs=4)
    assert cr.last_record()["pipelined"]
    check_path(cr, x.array, x0, [G_PATH], 1, threads, before)


@pytest.mark.parametrize("threshold", [100, 2], ids=["below_graph_threshold", "above_graph_threshold"])
def test_path_repeat_count(crs, threads, threshold):
    cr = crs["path"]
    x0 = path_input()
    x = ck.ClArray(x0.copy())
    before = cr.device_enqueue_errors()
    x.compute(cr, 30, "lead", G_PATH, L_PATH)  # buffers and the stream's queue exist
    saved = cr.repeat_graph_threshold
    cr.repeat_count = 3
    cr.repeat_graph_threshold = threshold
    try:
        x.compute(cr, 30, "lead", G_PATH, L_PATH)
    finally:
        cr.repeat_count = 1
        cr.repeat_graph_threshold = saved
    check_path(cr, x.array, x0, [G_PATH], 4, threads, before)


def test_path_capture_and_replay(crs, threads):
    cr = crs["path"]
    x0 = path_input()
    x = ck.ClArray(x0.copy())
    before = cr.device_enqueue_errors()
    x.compute(cr, 31, "lead", G_PATH, L_PATH)
    x.read = x.write = False
    with cr.capture() as g:
        x.compute(cr, 31, "lead", G_PATH, L_PATH)
    g.replay(2)
    cr.download(x, 0)
    g.destroy()
    check_path(cr, x.array, x0, [G_PATH], 3, threads, before)


def test_path_record_kernel_times(crs, threads):
    """The hipExtModuleLaunchKernel branch of the parent launch."""
    cr = crs["path"]
    x0 = path_input()
    x = ck.ClArray(x0.copy())
    before = cr.device_enqueue_errors()
    cr.record_kernel_times = True
    try:
        x.compute(cr, 32, "lead", G_PATH, L_PATH)
        times = cr.kernel_times(0)
    finally:
        cr.record_kernel_times = False
    assert [k for k, _ in times] == ["lead"] and times[0][1] > 0
    check_path(cr, x.array, x0, [G_PATH], 1, threads, before)


def test_path_debug_checks_name_the_parent(gpu, threads):
    """A child that writes one element into the guard tail (memory the
    runtime owns) is reported under its parent's kernel name."""
    cr = ck.ClNumberCruncher(gpu[0], kl.PATH_SRC)
    assert cr.error_code() == 0, cr.error_message()
    cr.debug_checks = True
    x0 = path_input()
    x = ck.ClArray(x0.copy())
    x.compute(cr, 1, "lead", G_PATH, L_PATH)
    check_path(cr, x.array, x0, [G_PATH], 1, threads, 0)
    with pytest.raises(Exception, match=r"lead_oob.*wrote past the end of array #0 \(%d bytes\).*first at \+0"
                       % (4 * G_PATH)):
        x.compute(cr, 2, "lead_oob", G_PATH, L_PATH)
    assert cr.device_enqueue_errors() == 0
    cr.dispose()


# ------------------------------------------------------------------ part B

@pytest.mark.parametrize("L", kl.WG_LOCALS)
def test_rotation_and_loop_barriers(crs, L):
    G = kl.wg_range(L)
    a = kl.wg_input(G)
    got = kl.run(crs["wg"], 1, "rot", {"a": a, "b": np.zeros(G, np.int32)}, ("a", "b"), G, L, outputs=("b",))
    assert kl.mismatches(got, {"b": kl.rot_model(a, L)}) == []
    got = kl.run(crs["wg"], 2, "loopbar", {"a": a, "b": np.zeros(G, np.int32), "trips": np.array([5], np.int32)},
                 ("a", "b", "trips"), G, L, outputs=("b",))
    assert kl.mismatches(got, {"b": kl.loopbar_model(a, L, 5)}) == []


@pytest.mark.parametrize("L", (1, 48, 64, 256))
def test_atomics_global_and_shared(crs, L):
    kl.check_shared_atomics(crs["wg"], L)
    kl.check_global_atomics(crs["atom"], L)


@pytest.mark.parametrize("L", kl.SUM_LOCALS)
def test_block_sum_any_local_size(crs, L):
    kl.check_block_sum(crs["wg"], L)


# ------------------------------------------------------------------ part C

def test_dialect_builtins_exact(crs):
    kl.check_dialect_exact(crs["dialect"])


def test_native_functions_add_a_name_not_arithmetic(crs):
    """native_* on gfx950 are bit-identical to the HIP-dialect twin that calls
    the intrinsic the prelude maps them to.  The distance from float64 is
    printed, not asserted (profiles/kernel_lang.md)."""
    r = kl.run_native(crs["dialect"], "d_native", 14)
    twin = kl.run_native(crs["twin"], "t_native", 15)
    for row, name in enumerate(kl.NATIVE_NAMES):
        assert r[row].tobytes() == twin[row].tobytes(), name
    a, b = kl.native_inputs()
    print("\ngfx950 native_* worst ulp from float64:", kl.native_distance(r, a, b))


def test_rewriting_rules_and_printf_literal(crs, capfd):
    kl.check_rewrite_and_printf(crs["rewrite"], crs["dialect"], capfd)
    assert capfd.readouterr().out.count(kl.PRINT_LINE) == 1
