"""Corpus of JIT kernel strings and plain models of what each must leave in
its arrays (no GPU use; the CPU tier is tests/test_kernel_lang.py, the GPU
tier tests/test_gpu_kernel_lang.py).

The code under test is what the runtime generates around a user's kernel
string (csrc/jit.cpp: gpu_rewrite, cpu_rewrite, translate_opencl, the two
preludes, the fiber and simd runners, the ``__cek_dispatch_<kernel>``
dispatchers behind ``cek_enqueue``) and the ``cek_block_sum`` helper.

Every effect in the corpus is order-independent — integer atomics, ``+=`` of
small integers in fp32, or distinct elements per record — so the expected
arrays are exact and unique.

Part A  device-side enqueue against :class:`QueueModel`, an executable model
        of the queue.
Part B  work-group semantics (barriers, LDS, atomics, cek_block_sum), the same
        source on the CPU device and on gfx950.
Part C  the OpenCL dialect: builtins, typedefs and the rewriting rules.
"""
from __future__ import annotations

import ctypes

import numpy as np

import cekirdekler_amd as ck
from cekirdekler_amd import cek

# queue levels (the parent's included) and records per level, from the runtime
K_LEVELS = int(cek.DYN_LEVELS)
K_CAP = int(cek.DYN_CAP)


def dispatcher_threads(compute_units: int) -> int:
    """Work items of one dispatcher launch: 4 work-groups of 256 per CU."""
    return 4 * max(1, int(compute_units)) * 256


# ===================================================================== part A

WRONG_RULES = {
    "child_off_by_one": "the child index off by one",
    "no_reset": "counts not reset between launches",
    "param32": "param truncated to 32 bits",
    "no_tail": "no grid-stride tail",
    "nonpos_error": "n <= 0 counted as an error",
    "cap_global": "the cap applied across levels instead of per level",
    "levels_plus": "one level too many dispatched",
    "levels_minus": "one level too few dispatched",
}


class QueueModel:
    """The rules of ``cek_enqueue``, run level by level.

    ``children`` maps child names, in source order, to functions
    ``child(ids, param, A, enq)`` (``ids``: the record's ids as an array,
    ``A``: dict of arrays); a parent is ``parent(g, lid, L, A, enq)`` for one
    work item.  ``enq(name, n, param)`` is the model of ``cek_enqueue``.
    ``wrong`` selects one deliberately wrong rule (WRONG_RULES) for the
    discrimination tests."""

    def __init__(self, children: dict, wrong: str | None = None):
        assert wrong is None or wrong in WRONG_RULES
        self.names = list(children)
        self.children = list(children.values())
        self.wrong = wrong
        self.recs = [[] for _ in range(K_LEVELS)]

    def _enq(self, level: int):
        def enq(name, n, param):
            n, param = int(n), int(param)
            if n <= 0:                        # appends nothing, no error
                self.errors += self.wrong == "nonpos_error"
                return
            if level + 1 >= K_LEVELS:         # an enqueue from the last level
                self.errors += 1
                return
            held = sum(map(len, self.recs)) if self.wrong == "cap_global" else len(self.recs[level + 1])
            if held >= K_CAP:                 # the level is full
                self.errors += 1
                return
            k = self.names.index(name)
            if self.wrong == "child_off_by_one":
                k = (k + 1) % len(self.names)
            if self.wrong == "param32":
                param = ((param & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000
            self.recs[level + 1].append((k, n, param))
        return enq

    def launch(self, parent, A: dict, offset: int, count: int, local: int, levels: int, threads: int) -> int:
        """One parent launch over work items [offset, offset + count) of one
        device, then its child levels; returns the errors it counted."""
        self.errors = 0
        if self.wrong != "no_reset":          # level counts start fresh at every parent launch
            self.recs = [[] for _ in range(K_LEVELS)]
        enq = self._enq(0)
        for g in range(offset, offset + count):
            parent(g, (g - offset) % local, local, A, enq)
        last = levels + {"levels_plus": 1, "levels_minus": -1}.get(self.wrong, 0)
        for lvl in range(1, min(max(last, 0), K_LEVELS - 1) + 1):   # later records are left behind
            enq = self._enq(lvl)
            for k, n, param in list(self.recs[lvl]):
                m = min(n, threads) if self.wrong == "no_tail" else n
                self.children[k](np.arange(m, dtype=np.int64), param, A, enq)
        return int(self.errors)


# ---- the table-driven parent: work item g < ctl[0] enqueues child kind
# ctl[1+2g] with n = ctl[2+2g] and param = prm[g]

_P = ("const int* __restrict__ ctl, const long long* __restrict__ prm, int* cnt, long long* out, int* x, float* f")

ENQ_SRC = f"""
__cek_child__ void k_inc(long long id, long long param, {_P}) {{ x[param + id] += 1; }}
__cek_child__ void k_half(long long id, long long param, {_P}) {{ f[param + id] += 0.5f; }}
__cek_child__ void k_store(long long id, long long param, {_P}) {{ out[(param & 7) + id] = param; }}
__cek_child__ void k_chain(long long id, long long param, {_P}) {{
  atomicAdd(&cnt[param], 1);
  cek_enqueue(k_chain, 2, param + 1);
}}
__cek_child__ void k_count(long long id, long long param, {_P}) {{
  atomicAdd(&cnt[0], 1);
  if (param > 0) cek_enqueue(k_count, 1, param - 1);
}}
__global__ void table({_P}) {{
  const long long g = get_global_id(0);
  atomicAdd(&cnt[7], 1);
  if (g >= ctl[0]) return;
  const int kind = ctl[1 + 2 * g];
  const long long n = ctl[2 + 2 * g], p = prm[g];
  switch (kind) {{
    case 0: cek_enqueue(k_inc, n, p); break;
    case 1: cek_enqueue(k_half, n, p); break;
    case 2: cek_enqueue(k_store, n, p); break;
    case 3: cek_enqueue(k_chain, n, p); break;
    case 4: cek_enqueue(k_count, n, p); break;
    default: break;
  }}
}}
"""

ENQ_ARRAYS = ("ctl", "prm", "cnt", "out", "x", "f")
ENQ_OUTPUTS = ("cnt", "out", "x", "f")
_KINDS = ("k_inc", "k_half", "k_store", "k_chain", "k_count")


def _k_inc(ids, param, A, enq):
    A["x"][param + ids] += 1


def _k_half(ids, param, A, enq):
    A["f"][param + ids] += np.float32(0.5)


def _k_store(ids, param, A, enq):
    A["out"][(param & 7) + ids] = param


def _k_chain(ids, param, A, enq):
    A["cnt"][param] += len(ids)
    for _ in ids:
        enq("k_chain", 2, param + 1)


def _k_count(ids, param, A, enq):
    A["cnt"][0] += len(ids)
    if param > 0:
        for _ in ids:
            enq("k_count", 1, param - 1)


ENQ_CHILDREN = dict(zip(_KINDS, (_k_inc, _k_half, _k_store, _k_chain, _k_count)))


def table_parent(g, lid, L, A, enq):
    A["cnt"][7] += 1
    if g >= A["ctl"][0]:
        return
    kind, n, p = int(A["ctl"][1 + 2 * g]), int(A["ctl"][2 + 2 * g]), int(A["prm"][g])
    if 0 <= kind < len(_KINDS):
        enq(_KINDS[kind], n, p)


def table_case(name: str, threads: int) -> dict:
    """A command table ``[(kind, n, param)]`` and the launch it needs:
    ``{"cmds", "G", "L", "nx"}`` (``nx``: length of x and f)."""
    nx = 256
    G = 1024
    if name == "levels":        # three child levels and a fourth attempt
        cmds = [(3, 3, 1)] * 16
    elif name == "kinds":       # three child kinds chosen by data, effects pairwise different
        cmds, stores = [], 0
        for j, k in enumerate(np.random.default_rng(11).integers(0, 3, 24)):
            if k == 2 and stores < 8:       # a kind-2 record stores its param at out[param & 7]: one per slot
                cmds.append((2, 1, stores))
                stores += 1
            else:
                cmds.append((int(k) % 2, 4, 8 * j))
    elif name == "param64":     # param as a full 64-bit value, positive and negative
        cmds = [(2, 1, (1 << 40) + 1), (2, 1, -(1 << 40) + 5), (2, 1, (1 << 40) + 2), (2, 1, -(1 << 62) + 7),
                (2, 1, (1 << 31)), (2, 1, -4)]
    elif name == "nvals":       # n of 0, -5 and 1
        cmds = [(0, 0, 0), (0, -5, 4), (0, 1, 8)]
    elif name == "tail":        # the grid-stride tail: more ids than the dispatcher has threads
        cmds = [(0, threads + 257, 0)]
        nx = threads + 257
    elif name == "cap_exact":   # a full level, and four records one level deeper: no error
        cmds = [(4, 1, 1 if j < 4 else 0) for j in range(K_CAP)]
    elif name == "cap_over":    # 512 enqueues more than a level holds, all interchangeable
        cmds = [(4, 1, 0)] * (K_CAP + 512)
    elif name == "few":         # the compute after an overflow is exact again
        cmds = [(4, 1, 0)] * 3
    elif name == "nothing":     # a parent that enqueues nothing at run time
        cmds = []
    else:
        raise KeyError(name)
    G = max(G, -(-len(cmds) // 256) * 256)
    return {"cmds": cmds, "G": G, "L": 256, "nx": nx}


TABLE_CASES = ("levels", "kinds", "param64", "nvals", "tail", "cap_exact", "cap_over", "few", "nothing")


def table_arrays(case: dict) -> dict:
    cmds, G = case["cmds"], case["G"]
    ctl = np.full(1 + 2 * G, -1, np.int32)
    ctl[0] = len(cmds)
    prm = np.zeros(G, np.int64)
    for j, (k, n, p) in enumerate(cmds):
        ctl[1 + 2 * j], ctl[2 + 2 * j], prm[j] = k, n, p
    return {"ctl": ctl, "prm": prm, "cnt": np.zeros(8, np.int32), "out": np.zeros(8, np.int64),
            "x": np.zeros(case["nx"], np.int32), "f": np.zeros(case["nx"], np.float32)}


def table_model(model: QueueModel, case: dict, levels: int, threads: int):
    """(arrays, errors) of one ``table`` launch under ``model``."""
    A = table_arrays(case)
    errors = model.launch(table_parent, A, 0, case["G"], case["L"], levels, threads)
    return A, errors


# ---- parent parameter lists: names that are the dispatcher's own words, a
# const __restrict__ array, arrays of different element types, two parents
# sharing a child, a kernel that enqueues nothing

_N = "const float* __restrict__ q, float* cnt, int* stride, long long* r, unsigned* rec, int* i"

NAMES_SRC = f"""
__cek_child__ void put(long long id, long long param, {_N}) {{
  const long long e = param + id;
  cnt[e] = q[e] + 1.0f;
  stride[e] += 2;
  r[e] = -e - 1;
  rec[e] = 3000000000u + (unsigned)e;
  atomicAdd(&i[0], 1);
}}
__global__ void pa({_N}) {{
  if (get_local_id(0) == 0) cek_enqueue(put, get_local_size(0), get_global_id(0));
}}
__global__ void pb({_N}) {{
  const long long g = get_global_id(0);
  stride[g] += 100;
  if (get_local_id(0) == 1) cek_enqueue(put, 1, g);
}}
__global__ void plain({_N}) {{ stride[get_global_id(0)] += 1000; }}
"""

NAMES_ARRAYS = ("q", "cnt", "stride", "r", "rec", "i")


def names_arrays(G: int) -> dict:
    return {"q": np.arange(G, dtype=np.float32), "cnt": np.zeros(G, np.float32), "stride": np.zeros(G, np.int32),
            "r": np.zeros(G, np.int64), "rec": np.zeros(G, np.uint32), "i": np.zeros(1, np.int32)}


def _put(ids, param, A, enq):
    e = param + ids
    A["cnt"][e] = A["q"][e] + np.float32(1)
    A["stride"][e] += 2
    A["r"][e] = -e - 1
    A["rec"][e] = (3000000000 + e).astype(np.uint32)
    A["i"][0] += len(ids)


NAMES_CHILDREN = {"put": _put}


def _pa(g, lid, L, A, enq):
    if lid == 0:
        enq("put", L, g)


def _pb(g, lid, L, A, enq):
    A["stride"][g] += 100
    if lid == 1:
        enq("put", 1, g)


def _plain(g, lid, L, A, enq):
    A["stride"][g] += 1000


NAMES_PARENTS = {"pa": _pa, "pb": _pb, "plain": _plain}

# ---- a dialect parent

DIALECT_ENQ_SRC = """
__cek_child__ void dput(long long id, long long param, __global int* x) { x[param + id] += 5; }
__kernel void dpar(__global int* x) {
  if (get_local_id(0) == 0) cek_enqueue(dput, get_local_size(0), get_global_id(0));
}
"""

# ---- paths: the leader of each group enqueues a child over its own group's
# elements, so every write stays in its device's range and the result does
# not depend on the split

PATH_SRC = """
__cek_child__ void g_inc(long long id, long long param, int* x) { x[param + id] += 1; }
__cek_child__ void g_oob(long long id, long long param, int* x) { x[param + id] = 7; }
__global__ void lead(int* x) {
  const long long g = get_global_id(0);
  x[g] += 100;
  if (get_local_id(0) == 0) cek_enqueue(g_inc, get_local_size(0), g);
}
__global__ void lead_oob(int* x) {
  const long long g = get_global_id(0);
  x[g] += 100;
  if (g + 1 == get_global_size(0)) cek_enqueue(g_oob, 1, g + 1);
}
"""


def _g_inc(ids, param, A, enq):
    A["x"][param + ids] += 1


def _g_oob(ids, param, A, enq):
    A["x"][param + ids] = 7


PATH_CHILDREN = {"g_inc": _g_inc, "g_oob": _g_oob}


def lead_parent(g, lid, L, A, enq):
    A["x"][g] += 100
    if lid == 0:
        enq("g_inc", L, g)


def lead_model(x: np.ndarray, ranges, L: int, launches: int, threads: int):
    """``launches`` runs of ``lead`` with the global range split into the
    devices' ``ranges``; (x afterwards, errors)."""
    A = {"x": x.copy()}
    errors = 0
    for _ in range(launches):
        off = 0
        for r in ranges:                      # one queue and one model per device
            errors += QueueModel(PATH_CHILDREN).launch(lead_parent, A, off, int(r), L, K_LEVELS - 1, threads)
            off += int(r)
    return A["x"], errors


# ===================================================================== part B

WG_LOCALS = (1, 48, 64, 256, 1024)   # 48: neither a power of two nor a multiple of the wave
SUM_LOCALS = (1, 48, 64, 256)

_BLOCK_SUM = str(ck.ClBuiltInAuxilliaryFunctions(block_sum=True))

# barrier kernels: on the CPU device the whole program runs on the fiber runner
WG_SRC = _BLOCK_SUM + r"""
__global__ void rot(const int* a, int* b) {
  __shared__ int s0[1024];
  __shared__ int s1[1024];
  const int t = (int)get_local_id(0), L = (int)get_local_size(0);
  const long long g = get_global_id(0);
  s0[t] = a[g];
  __syncthreads();
  s1[t] = s0[(t + 1) % L] + 1;
  __syncthreads();
  s0[t] = s1[(t + 3) % L] * 2;
  __syncthreads();
  b[g] = s0[(t + 5) % L] - t;
}
__global__ void loopbar(const int* a, int* b, const int* trips) {
  __shared__ int s[1024];
  const int t = (int)get_local_id(0), L = (int)get_local_size(0);
  const long long g = get_global_id(0);
  int v = a[g];
  for (int k = 0; k < trips[0]; ++k) {   // uniform trip count
    s[t] = v;
    __syncthreads();
    v = s[(t + 1) % L] + k;
    __syncthreads();
  }
  b[g] = v;
}
__global__ void shatom(const int* a, int* tick, int* exo, int* gout, float* gf) {
  __shared__ int acc[4];
  __shared__ float fa[1];
  const int t = (int)get_local_id(0), L = (int)get_local_size(0);
  const long long g = get_global_id(0), grp = g / L;
  if (t == 0) { acc[0] = 0; acc[1] = -2147483647 - 1; acc[2] = 2147483647; acc[3] = 0; fa[0] = 0.0f; }
  __syncthreads();
  tick[g] = atomicAdd(&acc[0], 1);
  atomicMax(&acc[1], a[g]);
  atomicMin(&acc[2], a[g]);
  exo[g] = atomicExch(&acc[3], t + 1);
  atomicAdd(&fa[0], (float)(a[g] & 3));
  __syncthreads();
  if (t == 0) {
    gout[4 * grp + 0] = acc[0]; gout[4 * grp + 1] = acc[1]; gout[4 * grp + 2] = acc[2]; gout[4 * grp + 3] = acc[3];
    gf[grp] = fa[0];
  }
}
__global__ void bsum(const float* xf, float* bs) {
  __shared__ float scratch[256];
  const long long g = get_global_id(0);
  bs[g] = cek_block_sum(xf[g], scratch);
}
"""

# no barrier: the CPU device's simd runner
ATOM_SRC = r"""
__global__ void hist(const int* bin, int* hi, unsigned* hu, long long* hl, unsigned long long* hq, float* hf,
                     double* hd) {
  const long long g = get_global_id(0);
  const int b = bin[g];
  atomicAdd(&hi[b], 1);
  atomicAdd(&hu[b], 3);                       // integer literals for every type
  atomicAdd(&hl[b], (1ll << 33) - g);
  atomicAdd(&hq[b], 1);
  atomicAdd(&hq[8 + b], (unsigned long long)g << 32);
  atomicAdd(&hf[b], 1);
  atomicAdd(&hd[b], 0.5);
}
__global__ void ticket(int* c, int* old, unsigned long long* cq, unsigned long long* oldq) {
  const long long g = get_global_id(0);
  old[g] = atomicAdd(&c[0], 1);
  oldq[g] = atomicAdd(&cq[0], 1);
}
__global__ void maxmin(const int* v, int* mi, unsigned* mu, long long* ml, unsigned long long* mq) {
  const long long g = get_global_id(0);
  atomicMax(&mi[0], v[g]);                     atomicMin(&mi[1], v[g]);
  atomicMax(&mu[0], (unsigned)v[g] * 3u);      atomicMin(&mu[1], (unsigned)v[g] * 3u);
  atomicMax(&ml[0], (long long)v[g] << 20);    atomicMin(&ml[1], (long long)v[g] << 20);
  atomicMax(&mq[0], (unsigned long long)g << 34);
  atomicMin(&mq[1], ((unsigned long long)g << 34) + 9);
  atomicMax(&mi[2], 5);                        // literals
  atomicMin(&mu[2], 7);
}
__global__ void exch(int* w, int* old, float* ef, float* oldf, unsigned long long* eq, unsigned long long* oldq) {
  const long long g = get_global_id(0);
  old[g] = atomicExch(&w[0], (int)g + 1);      // one word passed through every work item
  oldf[g] = atomicExch(&ef[g], (float)g + 0.5f);
  oldq[g] = atomicExch(&eq[g], ((unsigned long long)g << 40) + 1);
}
"""


def wg_range(L: int) -> int:
    """More than one group at every local size."""
    return 2 * L if L >= 1024 else 3 * L


def wg_input(G: int) -> np.ndarray:
    return np.random.default_rng(21).integers(-1000, 1000, G).astype(np.int32)


def rot_model(a: np.ndarray, L: int) -> np.ndarray:
    s0 = a.reshape(-1, L).astype(np.int32)
    s1 = np.roll(s0, -1, axis=1) + 1
    s0 = np.roll(s1, -3, axis=1) * 2
    return (np.roll(s0, -5, axis=1) - np.arange(L, dtype=np.int32)).reshape(-1)


def loopbar_model(a: np.ndarray, L: int, trips: int) -> np.ndarray:
    v = a.reshape(-1, L).astype(np.int32)
    for k in range(trips):
        v = np.roll(v, -1, axis=1) + k
    return v.reshape(-1)


def shatom_model(a: np.ndarray, L: int) -> dict:
    """What is unique: the per-group words.  ``tick`` and ``exo`` hold the
    returned old values, checked by :func:`is_ticket_order` / :func:`is_exchange_chain`."""
    v = a.reshape(-1, L)
    gout = np.stack([np.full(len(v), L), v.max(1), v.min(1)], axis=1).astype(np.int32)
    return {"gout3": gout, "gf": (v & 3).sum(1).astype(np.float32)}


def is_ticket_order(old: np.ndarray, n: int) -> bool:
    """The old values of n increments by 1 from 0 sort to arange(n)."""
    return np.array_equal(np.sort(np.asarray(old).astype(np.int64)), np.arange(n))


def is_exchange_chain(old: np.ndarray, final: int, n: int) -> bool:
    """A word that starts at 0 and is exchanged with 1..n: the returned old
    values and the word's final value are 0..n, each once."""
    return np.array_equal(np.sort(np.append(np.asarray(old).astype(np.int64), int(final))), np.arange(n + 1))


def block_sum_input(G: int) -> np.ndarray:
    """Integer-valued floats: every partial sum is exact in fp32."""
    return np.random.default_rng(22).integers(-64, 64, G).astype(np.float32)


def block_sum_model(xf: np.ndarray, L: int, drop_odd: bool = False) -> np.ndarray:
    """Every work item gets its group's sum.  ``drop_odd``: the wrong model
    of a halving loop that truncates (at 48 items scratch[2] is never added)."""
    v = xf.reshape(-1, L).astype(np.float64).copy()
    if drop_odd:
        n = L
        while n > 1:
            s = n // 2
            v[:, :s] += v[:, s:2 * s]
            n = s
        tot = v[:, 0]
    else:
        tot = v.sum(1)
    return np.repeat(tot.astype(np.float32), L)


HIST_BINS = 8


def hist_input(G: int) -> np.ndarray:
    return np.random.default_rng(23).integers(0, HIST_BINS, G).astype(np.int32)


def hist_arrays() -> dict:
    return {"hi": np.zeros(8, np.int32), "hu": np.zeros(8, np.uint32), "hl": np.zeros(8, np.int64),
            "hq": np.zeros(16, np.uint64), "hf": np.zeros(8, np.float32), "hd": np.zeros(8, np.float64)}


def hist_model(bins: np.ndarray, lose_one: bool = False) -> dict:
    """``lose_one``: the wrong model of a non-atomic update (one increment lost)."""
    A = hist_arrays()
    g = np.arange(len(bins), dtype=np.int64)
    np.add.at(A["hi"], bins, 1)
    np.add.at(A["hu"], bins, np.uint32(3))
    np.add.at(A["hl"], bins, (1 << 33) - g)
    np.add.at(A["hq"], bins, np.uint64(1))
    np.add.at(A["hq"], 8 + bins, g.astype(np.uint64) << np.uint64(32))
    np.add.at(A["hf"], bins, np.float32(1))
    np.add.at(A["hd"], bins, 0.5)
    if lose_one:
        A["hi"][bins[0]] -= 1
    return A


def maxmin_arrays() -> dict:
    return {"mi": np.array([-2**31, 2**31 - 1, 0], np.int32), "mu": np.array([0, 2**32 - 1, 2**32 - 1], np.uint32),
            "ml": np.array([-2**63, 2**63 - 1], np.int64), "mq": np.array([0, 2**64 - 1], np.uint64)}


def maxmin_model(v: np.ndarray) -> dict:
    g = np.arange(len(v), dtype=np.uint64)
    u = (v.astype(np.int64) * 3 & 0xFFFFFFFF).astype(np.uint32)
    sh = v.astype(np.int64) << 20
    return {"mi": np.array([v.max(), v.min(), 5], np.int32), "mu": np.array([u.max(), u.min(), 7], np.uint32),
            "ml": np.array([sh.max(), sh.min()], np.int64),
            "mq": np.array([(g << np.uint64(34)).max(), ((g << np.uint64(34)) + np.uint64(9)).min()], np.uint64)}


# ===================================================================== part C

# every name the preludes declare under CEK_OPENCL_DIALECT has a kernel here
DIALECT_SRC = r"""
__constant float TAB[4] = {1.0f, 2.0f, 4.0f, 8.0f};
__kernel void d_mad(__global const float* a, __global float* y) {
  int i = get_global_id(0);
  y[i] = mad(a[i], 2.0f, TAB[i & 3]);
}
__kernel void d_clamp(__global const float* a, __global float* y) {
  int i = get_global_id(0);
  y[i] = clamp(a[i], -2.0f, 3.0f);
}
kernel void d_atomic(global const int* bin, global int* h, global int* c) {
  int i = get_global_id(0);
  atomic_add(&h[bin[i]], 3);
  atomic_inc(&c[0]);
}
__kernel void d_types(__global uchar* a, __global ushort* b, __global uint* c, __global ulong* d) {
  uint i = (uint)get_global_id(0);
  a[i] = (uchar)(i * 7u);
  b[i] = (ushort)(i * 1001u);
  c[i] = i * 70001u;
  d[i] = (ulong)i << 33;
}
__kernel void d_native(__global const float* a, __global const float* b, __global float* r) {
  int i = get_global_id(0), n = get_global_size(0);
  r[0 * n + i] = native_sqrt(a[i]);
  r[1 * n + i] = native_rsqrt(a[i]);
  r[2 * n + i] = native_exp(b[i]);
  r[3 * n + i] = native_sin(b[i]);
  r[4 * n + i] = native_cos(b[i]);
  r[5 * n + i] = native_divide(b[i], a[i]);
}
__kernel void d_print(__global int* y) {
  int i = get_global_id(0);
  if (i == 3) printf("item %d: local global constant kernel barrier( end\n", i);
  y[i] = i;
}
"""

# the rewriting rules around barrier / mem_fence (a barrier: the fiber runner on the CPU device)
REWRITE_SRC = r"""
__device__ int my_barrier(int v) { return v + 1; }       // user functions whose names end in a keyword
__device__ int do_mem_fence(int v) { return v * 2; }
__kernel void d_rewrite(__global int* y) {
  __local int s[64];
  int t = get_local_id(0), i = get_global_id(0);
  s[t] = my_barrier(i);
  barrier(CLK_LOCAL_MEM_FENCE | (CLK_GLOBAL_MEM_FENCE));
  read_mem_fence(CLK_LOCAL_MEM_FENCE);
  int v = s[(t + 1) % (int)get_local_size(0)];
  write_mem_fence((CLK_GLOBAL_MEM_FENCE));
  mem_fence(CLK_LOCAL_MEM_FENCE);
  y[i] = do_mem_fence(v);
}
"""

PRINT_LINE = "item 3: local global constant kernel barrier( end"

# the HIP-dialect twin of d_native: the functions the prelude maps native_* to
TWIN_SRC = r"""
#ifdef CEK_GPU
#define T_SQRT(x) __fsqrt_rn(x)
#define T_RSQRT(x) rsqrtf(x)
#define T_EXP(x) __expf(x)
#define T_SIN(x) __sinf(x)
#define T_COS(x) __cosf(x)
#define T_DIV(a, b) __fdividef(a, b)
#else
#define T_SQRT(x) sqrtf(x)
#define T_RSQRT(x) (1.0f / sqrtf(x))
#define T_EXP(x) expf(x)
#define T_SIN(x) sinf(x)
#define T_COS(x) cosf(x)
#define T_DIV(a, b) ((a) / (b))
#endif
__global__ void t_native(const float* a, const float* b, float* r) {
  int i = get_global_id(0), n = get_global_size(0);
  r[0 * n + i] = T_SQRT(a[i]);
  r[1 * n + i] = T_RSQRT(a[i]);
  r[2 * n + i] = T_EXP(b[i]);
  r[3 * n + i] = T_SIN(b[i]);
  r[4 * n + i] = T_COS(b[i]);
  r[5 * n + i] = T_DIV(b[i], a[i]);
}
"""

NATIVE_NAMES = ("native_sqrt", "native_rsqrt", "native_exp", "native_sin", "native_cos", "native_divide")
NATIVE_N = 256


def native_inputs():
    """A fixed grid inside each function's ordinary domain: a in [0.25, 64]
    (sqrt, rsqrt, the divisor), b in [-3.14, 3.14] (exp, sin, cos, the dividend)."""
    a = np.linspace(0.25, 64.0, NATIVE_N).astype(np.float32)
    b = np.linspace(-3.14, 3.14, NATIVE_N).astype(np.float32)
    return a, b


def native_float64(a, b) -> np.ndarray:
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.stack([np.sqrt(a), 1.0 / np.sqrt(a), np.exp(b), np.sin(b), np.cos(b), b / a])


def native_ieee(a, b) -> dict:
    """The rows IEEE fixes, as the CPU prelude writes them, in numpy float32."""
    one = np.float32(1)
    return {0: np.sqrt(a), 1: one / np.sqrt(a), 5: b / a}


def native_distance(r: np.ndarray, a, b) -> dict:
    """Worst distance of each function from its float64 evaluation, in ulps
    of the float32 result (recorded in profiles/kernel_lang.md, not asserted)."""
    ref = native_float64(a, b)
    got = r.reshape(6, -1).astype(np.float64)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return {nm: float(np.max(np.abs(got[k] - ref[k]) / ulp[k])) for k, nm in enumerate(NATIVE_NAMES)}


def mad_input(n: int) -> np.ndarray:
    """Integer-valued: a*b + c is exact, fused or not."""
    return np.random.default_rng(31).integers(-100, 100, n).astype(np.float32)


def mad_model(a):
    return a * np.float32(2) + np.array([1, 2, 4, 8], np.float32)[np.arange(len(a)) & 3]


def clamp_input(n: int) -> np.ndarray:
    return np.linspace(-6.0, 6.0, n).astype(np.float32)


def clamp_model(a):
    return np.minimum(np.maximum(a, np.float32(-2)), np.float32(3))


def types_model(n: int) -> dict:
    i = np.arange(n, dtype=np.uint64)
    return {"a": (i * 7).astype(np.uint8), "b": (i * 1001).astype(np.uint16), "c": (i * 70001).astype(np.uint32),
            "d": i << np.uint64(33)}


def rewrite_model(G: int, L: int) -> np.ndarray:
    s = (np.arange(G, dtype=np.int32) + 1).reshape(-1, L)
    return (np.roll(s, -1, axis=1) * 2).reshape(-1)


# every corpus source: all of them must rewrite and cross-compile for gfx950
SOURCES = {"enq": ENQ_SRC, "names": NAMES_SRC, "dialect_enq": DIALECT_ENQ_SRC, "path": PATH_SRC, "wg": WG_SRC,
           "atom": ATOM_SRC, "dialect": DIALECT_SRC, "rewrite": REWRITE_SRC, "twin": TWIN_SRC}
# the sources that also build and run on the CPU device (no cek_enqueue there)
CPU_SOURCES = ("wg", "atom", "dialect", "rewrite", "twin")


# ==================================================================== running

def mismatches(got: dict, want: dict) -> list:
    """One line per array of ``want`` that ``got`` does not equal bit for bit:
    its name, how many elements differ and the first of them."""
    bad = []
    for k, w in want.items():
        g = np.asarray(got[k])
        w = np.asarray(w)
        if g.shape != w.shape or g.dtype != w.dtype:
            bad.append(f"{k}: {g.dtype}{g.shape} for {w.dtype}{w.shape}")
        elif g.tobytes() != w.tobytes():
            d = np.flatnonzero(g.view(np.uint8).reshape(len(g), -1) != w.view(np.uint8).reshape(len(w), -1))
            i = int(d[0]) // g.itemsize
            bad.append(f"{k}: {len(set((d // g.itemsize).tolist()))} of {len(g)} differ, first [{i}] = {g[i]!r}, "
                       f"model {w[i]!r}")
    return bad


def run(cr, cid: int, kernel: str, arrays: dict, order, G: int, L: int, outputs=(), **kw) -> dict:
    """One compute on a one-device cruncher: arrays in ``order``, inputs read
    whole and not written back, ``outputs`` read and written back whole.
    Returns the host arrays afterwards."""
    cl = []
    for name in order:
        a = ck.ClArray(arrays[name])
        if name in outputs:
            a.write_all = True
        else:
            a.write = False
        cl.append(a)
    ck.ClParameterGroup(cl).compute(cr, cid, kernel, G, L, **kw)
    return {name: a.array.copy() for name, a in zip(order, cl)}


# ===================================================== checks both tiers share
# (one cruncher per source, built by the caller for its device)

def check_shared_atomics(cr, L):
    G = wg_range(L)
    a = wg_input(G)
    arrays = {"a": a, "tick": np.full(G, -1, np.int32), "exo": np.full(G, -1, np.int32),
              "gout": np.zeros(4 * (G // L), np.int32), "gf": np.zeros(G // L, np.float32)}
    got = run(cr, 3, "shatom", arrays, ("a", "tick", "exo", "gout", "gf"), G, L,
                 outputs=("tick", "exo", "gout", "gf"))
    want = shatom_model(a, L)
    gout = got["gout"].reshape(-1, 4)
    assert mismatches({"gout3": np.ascontiguousarray(gout[:, :3]), "gf": got["gf"]}, want) == []
    for grp in range(G // L):
        assert is_ticket_order(got["tick"][grp * L:(grp + 1) * L], L)
        assert is_exchange_chain(got["exo"][grp * L:(grp + 1) * L], gout[grp, 3], L)


def check_block_sum(cr, L):
    G = wg_range(L)
    xf = block_sum_input(G)
    got = run(cr, 4, "bsum", {"xf": xf, "bs": np.zeros(G, np.float32)}, ("xf", "bs"), G, L, outputs=("bs",))
    assert mismatches(got, {"bs": block_sum_model(xf, L)}) == []
    return got


def check_global_atomics(cr, L):
    G = wg_range(L) if L > 1 else 64
    bins = hist_input(G)
    order = ("bin", "hi", "hu", "hl", "hq", "hf", "hd")
    got = run(cr, 5, "hist", {"bin": bins, **hist_arrays()}, order, G, L, outputs=order[1:])
    assert mismatches(got, hist_model(bins)) == []
    arrays = {"c": np.zeros(1, np.int32), "old": np.full(G, -1, np.int32), "cq": np.zeros(1, np.uint64),
              "oldq": np.zeros(G, np.uint64)}
    t = run(cr, 6, "ticket", arrays, ("c", "old", "cq", "oldq"), G, L, outputs=("c", "old", "cq", "oldq"))
    assert t["c"][0] == G and t["cq"][0] == G
    assert is_ticket_order(t["old"], G) and is_ticket_order(t["oldq"], G)
    v = wg_input(G)
    order = ("v", "mi", "mu", "ml", "mq")
    m = run(cr, 7, "maxmin", {"v": v, **maxmin_arrays()}, order, G, L, outputs=order[1:])
    assert mismatches(m, maxmin_model(v)) == []
    arrays = {"w": np.zeros(1, np.int32), "old": np.full(G, -1, np.int32), "ef": np.full(G, -1.0, np.float32),
              "oldf": np.zeros(G, np.float32), "eq": np.full(G, 5, np.uint64), "oldq": np.zeros(G, np.uint64)}
    order = ("w", "old", "ef", "oldf", "eq", "oldq")
    e = run(cr, 8, "exch", arrays, order, G, L, outputs=order)
    g = np.arange(G)
    assert is_exchange_chain(e["old"], e["w"][0], G)
    want = {"ef": (g + 0.5).astype(np.float32), "oldf": np.full(G, -1.0, np.float32),
            "eq": (g.astype(np.uint64) << np.uint64(40)) + np.uint64(1), "oldq": np.full(G, 5, np.uint64)}
    assert mismatches(e, want) == []
    return got, bins


def check_dialect_exact(cr):
    n = 256
    a = mad_input(n)
    got = run(cr, 10, "d_mad", {"a": a, "y": np.zeros(n, np.float32)}, ("a", "y"), n, 64, outputs=("y",))
    assert mismatches(got, {"y": mad_model(a)}) == []
    a = clamp_input(n)
    got = run(cr, 11, "d_clamp", {"a": a, "y": np.zeros(n, np.float32)}, ("a", "y"), n, 64, outputs=("y",))
    assert mismatches(got, {"y": clamp_model(a)}) == []
    bins = hist_input(n)
    got = run(cr, 12, "d_atomic", {"bin": bins, "h": np.zeros(8, np.int32), "c": np.zeros(1, np.int32)},
                 ("bin", "h", "c"), n, 64, outputs=("h", "c"))
    want = {"h": (3 * np.bincount(bins, minlength=8)).astype(np.int32), "c": np.array([n], np.int32)}
    assert mismatches(got, want) == []
    arrays = {"a": np.zeros(n, np.uint8), "b": np.zeros(n, np.uint16), "c": np.zeros(n, np.uint32),
              "d": np.zeros(n, np.uint64)}
    got = run(cr, 13, "d_types", arrays, ("a", "b", "c", "d"), n, 64, outputs=("a", "b", "c", "d"))
    assert mismatches(got, types_model(n)) == []


def run_native(cr, kernel, cid):
    a, b = native_inputs()
    n = NATIVE_N
    got = run(cr, cid, kernel, {"a": a, "b": b, "r": np.zeros(6 * n, np.float32)}, ("a", "b", "r"), n, 64,
                 outputs=("r",))
    return got["r"].reshape(6, n)


def check_rewrite_and_printf(cr_rewrite, cr_dialect, capfd):
    G, L = 192, 48
    got = run(cr_rewrite, 16, "d_rewrite", {"y": np.zeros(G, np.int32)}, ("y",), G, L, outputs=("y",))
    assert mismatches(got, {"y": rewrite_model(G, L)}) == []
    capfd.readouterr()
    got = run(cr_dialect, 17, "d_print", {"y": np.zeros(64, np.int32)}, ("y",), 64, 64, outputs=("y",))
    cr_dialect.sync()
    ctypes.CDLL(None).fflush(None)      # the CPU device prints through the process's own stdio
    assert mismatches(got, {"y": np.arange(64, dtype=np.int32)}) == []
