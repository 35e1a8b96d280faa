"""CPU tier of the kernel-string oracles (tests/kernel_lang.py): every corpus
source rewrites and cross-compiles for gfx950, parts B and C run on the CPU
device against their models, and the models themselves are shown to
discriminate (each wrong rule differs from the right one on a corpus case)."""
import numpy as np
import pytest

import cekirdekler_amd as ck
from cekirdekler_amd import cek

import kernel_lang as kl

THREADS = kl.dispatcher_threads(8)   # a small device: the model's rules do not depend on the size


# ------------------------------------------------------ rewrite + gfx950 build

@pytest.mark.parametrize("name", list(kl.SOURCES))
def test_corpus_source_cross_compiles_for_gfx950(name):
    src = kl.SOURCES[name]
    out = cek.gpu_rewrite(src)
    assert out.count("// ---- end prelude ----") == 1
    ok, code, log = cek.compile_gpu(src, [], "gfx950")
    assert ok, log
    assert code[:4] == b"\x7fELF"


def test_dialect_define_comes_before_the_prelude():
    for rewrite in (cek.gpu_rewrite, cek.cpu_rewrite):
        out = rewrite(kl.DIALECT_SRC)
        assert out.index("#define CEK_OPENCL_DIALECT 1") < out.index("#ifdef CEK_OPENCL_DIALECT")
        assert "CEK_OPENCL_DIALECT 1" not in rewrite(kl.TWIN_SRC)


def test_gpu_native_functions_do_not_carry_the_opencl_builtin_names():
    """A device function that is itself named native_sqrt mangles like the
    OpenCL builtin, and the AMDGPU backend then swaps in the full-precision
    function; the GPU prelude maps the names by macro onto __cek_native_*."""
    out = cek.gpu_rewrite(kl.DIALECT_SRC)
    for name in kl.NATIVE_NAMES:
        assert f"float {name}(" not in out and f"#define {name}(" in out, name


def test_dispatcher_locals_are_in_the_reserved_namespace():
    """Whatever the dispatcher declares starts with __cek_ (or is a parameter
    copied from the parent), so no parameter name can meet it."""
    out = cek.gpu_rewrite(kl.NAMES_SRC)
    body = out[out.index("// ---- dispatchers ----"):]
    assert "case 0: put(__cek_i, __cek_rec.param, q, cnt, stride, r, rec, i, __cek_q, __cek_level)" in body
    import re
    declared = re.findall(r"(?:const int|const long long|long long|int|__CekQueue\*|const __CekRec) (\w+) =", body)
    assert declared and all(d.startswith("__cek_") for d in declared), declared


def test_translation_leaves_literals_and_longer_identifiers_alone():
    out = cek.gpu_rewrite(kl.DIALECT_SRC)
    assert '"item %d: local global constant kernel barrier( end\\n"' in out
    out = cek.gpu_rewrite(kl.REWRITE_SRC)
    user = out[out.index("// ---- end prelude ----"):]
    assert "my_barrier(i)" in user and "do_mem_fence(v)" in user
    assert "my___syncthreads" not in user and "read___threadfence" not in user and "write___threadfence" not in user
    assert user.count("__syncthreads()") == 1 and user.count("__threadfence()") == 3
    assert "CLK_" not in user and "mem_fence(" not in user.replace("do_mem_fence(", "")


def test_cek_enqueue_on_cpu_device_is_refused(cpu):
    c = ck.ClNumberCruncher(cpu, kl.PATH_SRC)
    assert c.error_code() != 0
    assert "cek_enqueue (device-side enqueue) runs on GPU devices only" in c.error_message()


# --------------------------------------------------------------- CPU device

@pytest.fixture(scope="module")
def cpu():
    return ck.ClPlatforms.all().cpus(True)


@pytest.fixture(scope="module")
def crs(cpu):
    """One cruncher per corpus source that runs on the CPU device."""
    out = {}
    for name in kl.CPU_SOURCES:
        c = ck.ClNumberCruncher(cpu, kl.SOURCES[name])
        out[name] = c
    yield out
    for c in out.values():
        c.dispose()


def _cr(crs, name):
    c = crs[name]
    assert c.error_code() == 0, c.error_message()
    return c


@pytest.mark.parametrize("L", kl.WG_LOCALS)
def test_cpu_rotation_and_loop_barriers(crs, L):
    G = kl.wg_range(L)
    a = kl.wg_input(G)
    got = kl.run(_cr(crs, "wg"), 1, "rot", {"a": a, "b": np.zeros(G, np.int32)}, ("a", "b"), G, L, outputs=("b",))
    assert kl.mismatches(got, {"b": kl.rot_model(a, L)}) == []
    got = kl.run(_cr(crs, "wg"), 2, "loopbar", {"a": a, "b": np.zeros(G, np.int32), "trips": np.array([5], np.int32)},
                 ("a", "b", "trips"), G, L, outputs=("b",))
    assert kl.mismatches(got, {"b": kl.loopbar_model(a, L, 5)}) == []


@pytest.mark.parametrize("L", (1, 48, 64, 256))
def test_cpu_shared_word_atomics(crs, L):
    kl.check_shared_atomics(_cr(crs, "wg"), L)


@pytest.mark.parametrize("L", kl.SUM_LOCALS)
def test_cpu_block_sum_any_local_size(crs, L):
    kl.check_block_sum(_cr(crs, "wg"), L)


@pytest.mark.parametrize("L", (1, 48, 64, 256))
def test_cpu_global_atomics_every_type(crs, L):
    kl.check_global_atomics(_cr(crs, "atom"), L)


def test_comparisons_reject_a_dropped_element_and_a_lost_update(crs):
    """The wrong rules named: cek_block_sum's halving loop that truncates (at
    48 items scratch[2] is never added), and a histogram update that is not
    atomic (one increment lost)."""
    got = kl.check_block_sum(_cr(crs, "wg"), 48)
    xf = kl.block_sum_input(kl.wg_range(48))
    assert [m.split(":")[0] for m in kl.mismatches(got, {"bs": kl.block_sum_model(xf, 48, drop_odd=True)})] == ["bs"]
    # at a power of two the truncating loop is the right one: the summation tree did not move
    xp = kl.block_sum_input(kl.wg_range(64))
    assert np.array_equal(kl.block_sum_model(xp, 64, drop_odd=True), kl.block_sum_model(xp, 64))
    got, bins = kl.check_global_atomics(_cr(crs, "atom"), 48)
    assert [m.split(":")[0] for m in kl.mismatches(got, kl.hist_model(bins, lose_one=True))] == ["hi"]


# ------------------------------------------------------------------ part C

def test_cpu_dialect_builtins_exact(crs):
    kl.check_dialect_exact(_cr(crs, "dialect"))


def test_cpu_native_functions_add_a_name_not_arithmetic(crs):
    """native_* on the CPU device: bit-identical to numpy float32 where IEEE
    fixes the result (sqrt, 1/sqrt, /), and to the HIP-dialect twin kernel on
    the same device otherwise.  The distance from float64 is printed, not
    asserted (profiles/kernel_lang.md)."""
    r = kl.run_native(_cr(crs, "dialect"), "d_native", 14)
    twin = kl.run_native(_cr(crs, "twin"), "t_native", 15)
    a, b = kl.native_inputs()
    for row, want in kl.native_ieee(a, b).items():
        assert r[row].tobytes() == want.astype(np.float32).tobytes(), kl.NATIVE_NAMES[row]
    for row, name in enumerate(kl.NATIVE_NAMES):
        assert r[row].tobytes() == twin[row].tobytes(), name
    print("\nCPU device native_* worst ulp from float64:", kl.native_distance(r, a, b))


def test_cpu_rewriting_rules_and_printf_literal(crs, capfd):
    kl.check_rewrite_and_printf(_cr(crs, "rewrite"), _cr(crs, "dialect"), capfd)
    assert capfd.readouterr().out.count(kl.PRINT_LINE) == 1


# --------------------------------------------------- the queue model discriminates

def _table(model, name, levels=kl.K_LEVELS - 1):
    A, errors = kl.table_model(model, kl.table_case(name, THREADS), levels, THREADS)
    return {k: A[k] for k in kl.ENQ_OUTPUTS}, errors


def _differs(wrong, steps):
    """Right and wrong model over the same sequence of (case, levels)."""
    right, bad = kl.QueueModel(kl.ENQ_CHILDREN), kl.QueueModel(kl.ENQ_CHILDREN, wrong)
    diff = False
    for name, levels in steps:
        (ra, re_), (ba, be) = _table(right, name, levels), _table(bad, name, levels)
        diff = diff or re_ != be or kl.mismatches(ba, ra) != []
    return diff


def test_queue_model_right_rules_on_the_corpus():
    """The numbers the issue states, from the model alone."""
    m = kl.QueueModel(kl.ENQ_CHILDREN)
    A, e = _table(m, "levels")
    assert list(A["cnt"][:4]) == [0, 48, 96, 192] and A["cnt"][7] == 1024 and e == 192
    A, e = _table(m, "cap_exact")
    assert A["cnt"][0] == kl.K_CAP + 4 and e == 0
    A, e = _table(m, "cap_over")
    assert A["cnt"][0] == kl.K_CAP and e == 512
    A, e = _table(m, "few")
    assert A["cnt"][0] == 3 and e == 0
    A, e = _table(m, "tail")
    assert np.all(A["x"] == 1) and len(A["x"]) == THREADS + 257 and e == 0
    A, e = _table(m, "nvals")
    assert A["x"].sum() == 1 and A["x"][8] == 1 and e == 0
    A, e = _table(m, "param64")
    assert set(A["out"].tolist()) >= {(1 << 40) + 1, -(1 << 40) + 5, -(1 << 62) + 7, 1 << 31, -4} and e == 0
    for levels, cnt, err in ((0, [0, 0, 0], 0), (1, [48, 0, 0], 0), (2, [48, 96, 0], 0), (3, [48, 96, 192], 192)):
        A, e = _table(m, "levels", levels)
        assert list(A["cnt"][1:4]) == cnt and e == err


# wrong rule -> the (case, levels) sequence on which it must differ from the right rules
WRONG_CASES = [
    ("child_off_by_one", [("nvals", 3)]),
    ("no_reset", [("cap_over", 3), ("few", 3)]),
    ("param32", [("param64", 3)]),
    ("no_tail", [("tail", 3)]),
    ("nonpos_error", [("nvals", 3)]),
    ("cap_global", [("cap_exact", 3)]),
    ("levels_plus", [("levels", 1)]),
    ("levels_minus", [("levels", 2)]),
]


@pytest.mark.parametrize("wrong,steps", WRONG_CASES, ids=[w for w, _ in WRONG_CASES])
def test_queue_model_rejects_wrong_rule(wrong, steps):
    """Each wrong rule (kernel_lang.WRONG_RULES names them) gives another
    result than the right one on a corpus case, so a runtime that followed it
    would fail the GPU tier."""
    assert wrong in kl.WRONG_RULES
    assert _differs(wrong, steps), kl.WRONG_RULES[wrong]
    assert not _differs(None, steps)


def test_every_wrong_rule_has_a_discrimination_case():
    assert {w for w, _ in WRONG_CASES} == set(kl.WRONG_RULES)
