"""Executable model of the stage pipelines (cekirdekler_amd/parallel/
pipeline.py): a push-by-push numpy emulator of ``ClPipeline`` and a
feed-by-feed emulator of ``DevicePipeline``, their stage kernels (once as JIT
kernel strings, once as numpy callables), the cases and the harness that runs
one case on the real pipelines.  tests/test_pipeline_model.py is the CPU tier,
tests/test_gpu_pipeline_model.py the GPU tier; docs/API.md states the same
rules in prose.

``ClPipeline``.  Per stage the model holds the current and spare input and
output buffers and the hidden buffers, and per (device, buffer) one replica: a
GPU-kind device has a replica of its own, a CPU-kind device uses the stage's
host array (Replicas::buffer).  One push runs every stage's kernels in
order on its current buffers, each device over its range; after every kernel
of a multi-device stage each device's slice of every output and of every
hidden buffer that is not read_only goes into every other replica (the
coherence rule).  Then the transfers of the spare buffers run (host data into
stage 0, each stage's previous outputs into the next stage, the last stage's
previous outputs to the results), then the swaps, the owner snapshot and the
ready-counter rule of ``push_data``.  The ranges of every kernel of every push
are given to the model (the real pipeline's ``ranges(cid)`` / ``references
(cid)`` read after the push, or ``synthetic_splits``): the model never
predicts the balancer.

The oracle is the model with ``coherent=True``: every stage on one device.
What it returns for push ``p`` is a pure function of the pushed data and the
initial buffer contents.  The per-device-replica mode exists to count the
bytes each path moves and to express the faults.

Everything is integer (wrap-around arithmetic is exact) and every comparison
is ``==``.  ``faults=`` switches single rules to a wrong version; the CPU
tier shows that each is caught by a named case (FAULT_CASES, DP_FAULT_CASES).
The coherence rule makes every replica whole, and a transfer that takes a
wrong but covering slice from a whole replica still moves the right values.
The ownership faults and ``slice_epg_as_epw`` are therefore stated for the
variant that keeps outputs per device with one owner split per output
(``PER_DEVICE_OUTPUTS``), where slices must be exact; the fault-free model of
that variant equals the oracle too.
"""
from __future__ import annotations

import dataclasses
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from transfer_model import TYPES, stamp

L = 64                # local range of every kernel
N = 1536              # work items of every stage: 24 groups
GROUPS = N // L
TAIL = 7              # elements past range * epw in the "tail" outputs
EPG = 7               # the per-group record: odd, so that uchar slices are unaligned
U = np.uint64

FAULTS = (
    "hidden_per_device",              # no coherence of hidden state across a moved split
    "owner_last_kernel_only",         # every output is owned by the last kernel's split
    "owner_one_push_late",            # the owner split is the previous push's
    "slice_no_epw",                   # slices are taken without the epw factor
    "slice_epg_as_epw",               # elements_per_group is treated as elements per work item
    "slice_ignores_item_size",        # slices are counted in elements where bytes are meant
    "tail_dropped",                   # elements past range * epw never move
    "swap_inputs_skipped",            # a later stage's inputs are not swapped on a push without data
    "swap_outputs_without_results",   # the last stage's outputs are swapped on a push without results
    "ready_counter_off_by_one",       # results are announced one push early
    "transfer_to_device0_only",       # a transition fills only the first device of the next stage
    "initializer_on_one_buffer_set",  # the initializer runs on the current buffers only
)
PER_DEVICE_OUTPUTS = ("owner_last_kernel_only", "owner_one_push_late", "slice_epg_as_epw")

DP_FAULTS = (
    "transition_same_parity",    # the consumer reads the buffer the producer writes in the same feed
    "output_wrong_parity",       # output_buffer() hands out the buffer being written next
    "internal_double_buffered",  # an INTERNAL array alternates between two buffers
    "stop_still_uploads",        # stop_host_device_transmission does not stop the uploads
)


def _u(x) -> np.ndarray:
    """The C conversion (unsigned long long)x: signed types sign-extend."""
    return np.asarray(x).astype(U)


def perm(i):
    return (i * 31 + 7) % N


# ------------------------------------------------------------------ stage kinds


@dataclasses.dataclass(frozen=True)
class StageSpec:
    """One stage of a case.  ``devices`` names its devices, one letter each:
    ``g`` a (logical) GPU, ``c`` the CPU device.  ``xn`` is the length of the
    first input (N, or longer to take a whole longer output)."""
    kind: str            # "acc", "two", "join" or "init"
    devices: str = "g"
    E: int = 1           # elements per work item of the acc kind's output
    tail: int = 0        # elements past N * E in the acc kind's output
    xn: int = N


@dataclasses.dataclass(frozen=True)
class BufSpec:
    role: str            # "in", "hid" or "out"
    n: int
    epw: int = 1
    epg: int = 0
    read_only: bool = False


def buffers_of(s: StageSpec) -> List[BufSpec]:
    """The stage's parameter list: inputs, hidden buffers, outputs."""
    if s.kind == "acc":     # x, acc (state), y
        return [BufSpec("in", s.xn), BufSpec("hid", N), BufSpec("out", N * s.E + s.tail, epw=s.E)]
    if s.kind == "two":     # x, h (kernel 1 -> kernel 2), y (kernel 2), g (kernel 1 alone, per group)
        return [BufSpec("in", s.xn), BufSpec("hid", N), BufSpec("out", N), BufSpec("out", GROUPS * EPG, epg=EPG)]
    if s.kind == "join":    # x, gin, w (a read_only constant with a tail), y
        return [BufSpec("in", s.xn), BufSpec("in", GROUPS * EPG, epg=EPG), BufSpec("hid", N + TAIL, read_only=True),
                BufSpec("out", N)]
    if s.kind == "init":    # x, c (written by the initializer), y
        return [BufSpec("in", s.xn), BufSpec("hid", N), BufSpec("out", N)]
    raise KeyError(s.kind)


def kernels_of(s: StageSpec) -> Tuple[List[str], List[str]]:
    """(kernel names, initializer names)."""
    return {"acc": ([f"acc_{s.E}"], []), "two": (["two_a", "two_b"], []), "join": (["join"], []),
            "init": (["use_c"], ["init_c"])}[s.kind]


def writer_of(s: StageSpec) -> List[int]:
    """For every output, the index of the stage kernel that writes it."""
    return {"acc": [0], "two": [1, 0], "join": [0], "init": [0]}[s.kind]


def stage_source(s: StageSpec, ctype: str) -> str:
    """The stage's kernels in the project's kernel dialect.  Every index is
    inside its array whatever the split: a work item outside [0, PM_N)
    returns, and every other index is reduced into its array."""
    head = (f"typedef {ctype} T;\ntypedef unsigned long long U;\n#define PM_N {N}LL\n#define PM_XN {s.xn}LL\n"
            f"#define PM_L {L}LL\n#define PM_EPG {EPG}LL\n#define PM_PERM(i) (((i) * 31 + 7) % PM_N)\n")
    if s.kind == "acc":
        return head + f"""
__global__ void acc_{s.E}(const T* x, T* acc, T* y) {{
  const long long i = get_global_id(0);
  if (i < 0 || i >= PM_N) return;
  const T a = (T)((U)acc[i] + 3ull * (U)x[i] + (U)i + 1ull);
  acc[i] = a;
  for (long long e = 0; e < {s.E}; ++e)
    y[i * {s.E} + e] = (T)((U)a + (U)x[PM_PERM(i)] + (U)x[PM_XN - 1 - i % 7] + 5ull * (U)e + 11ull * (U)i);
}}
"""
    if s.kind == "two":
        return head + """
__global__ void two_a(const T* x, T* h, T* y, T* g) {
  const long long i = get_global_id(0);
  if (i < 0 || i >= PM_N) return;
  h[i] = (T)(7ull * (U)x[i] + (U)i + 3ull);
  if (i % PM_L == 0)
    for (long long j = 0; j < PM_EPG; ++j) g[i / PM_L * PM_EPG + j] = (T)((U)x[i] + 13ull * (U)j + (U)(i / PM_L));
}
__global__ void two_b(const T* x, T* h, T* y, T* g) {
  const long long i = get_global_id(0);
  if (i < 0 || i >= PM_N) return;
  y[i] = (T)((U)h[PM_PERM(i)] + (U)x[i] + (U)x[PM_XN - 1 - i % 7] + 2ull * (U)i);
}
"""
    if s.kind == "join":
        return head + f"""
__global__ void join(const T* x, const T* gin, const T* w, T* y) {{
  const long long i = get_global_id(0);
  if (i < 0 || i >= PM_N) return;
  y[i] = (T)((U)x[PM_PERM(i)] + (U)gin[(i * 5 + 3) % {GROUPS * EPG}LL] + (U)w[PM_N + {TAIL - 1}LL - i % 7] +
             (U)w[PM_PERM(i)] + 3ull * (U)i);
}}
"""
    return head + """
__global__ void init_c(const T* x, T* c, T* y) {
  const long long i = get_global_id(0);
  if (i < 0 || i >= PM_N) return;
  c[i] = (T)(13ull * (U)i + 1ull);
  y[i] = (T)(1000ull + 3ull * (U)i);
}
__global__ void use_c(const T* x, T* c, T* y) {
  const long long i = get_global_id(0);
  if (i < 0 || i >= PM_N) return;
  y[i] = (T)((U)x[i] + 2ull * (U)x[PM_PERM(i)] + (U)c[PM_PERM(i)] + (U)i);
}
"""


def numpy_kernel(s: StageSpec, name: str) -> Callable:
    """``k(bufs, i)``: the kernel ``name`` on the work items ``i`` (int64),
    ``bufs`` in parameter order."""
    E, xn = s.E, s.xn

    def acc(b, i):
        x, a, y = b
        new = (_u(a[i]) + U(3) * _u(x[i]) + _u(i) + U(1)).astype(a.dtype)
        a[i] = new
        for e in range(E):
            y[i * E + e] = (_u(new) + _u(x[perm(i)]) + _u(x[xn - 1 - i % 7]) + U(5 * e) + U(11) * _u(i)).astype(y.dtype)

    def two_a(b, i):
        x, h, y, g = b
        h[i] = (U(7) * _u(x[i]) + _u(i) + U(3)).astype(h.dtype)
        heads = i[i % L == 0]
        for j in range(EPG):
            g[heads // L * EPG + j] = (_u(x[heads]) + U(13 * j) + _u(heads // L)).astype(g.dtype)

    def two_b(b, i):
        x, h, y, g = b
        y[i] = (_u(h[perm(i)]) + _u(x[i]) + _u(x[xn - 1 - i % 7]) + U(2) * _u(i)).astype(y.dtype)

    def join(b, i):
        x, gin, w, y = b
        y[i] = (_u(x[perm(i)]) + _u(gin[(i * 5 + 3) % (GROUPS * EPG)]) + _u(w[N + TAIL - 1 - i % 7]) + _u(w[perm(i)]) +
                U(3) * _u(i)).astype(y.dtype)

    def init_c(b, i):
        x, c, y = b
        c[i] = (U(13) * _u(i) + U(1)).astype(c.dtype)
        y[i] = (U(1000) + U(3) * _u(i)).astype(y.dtype)

    def use_c(b, i):
        x, c, y = b
        y[i] = (_u(x[i]) + U(2) * _u(x[perm(i)]) + _u(c[perm(i)]) + _u(i)).astype(y.dtype)

    return {"two_a": two_a, "two_b": two_b, "join": join, "init_c": init_c, "use_c": use_c}.get(name, acc)


# ------------------------------------------------------------------ cases


@dataclasses.dataclass(frozen=True)
class Case:
    """A pipeline layout, its element type, how it is pushed and in which form
    the data is handed over; ``2 * stages + 6`` pushes."""
    name: str
    type_name: str
    stages: Tuple[StageSpec, ...]
    mode: str = "both"       # "both", "drain" or "gaps": see push_plan()
    data_form: str = "array"  # "array", "list" (llong only: a list becomes int64) or "strided" (x[::2])

    def __str__(self) -> str:
        return self.name

    @property
    def pushes(self) -> int:
        return 2 * len(self.stages) + 6

    @property
    def dtype(self):
        return np.dtype(TYPES[self.type_name][1])

    def single(self) -> "Case":
        """The same pipeline with every stage on one GPU-kind device."""
        return dataclasses.replace(self, stages=tuple(dataclasses.replace(s, devices="g") for s in self.stages))

    def on_cpu(self) -> "Case":
        """The same pipeline on CPU devices: a stage of several devices
        becomes cpu + cpu."""
        return dataclasses.replace(self, stages=tuple(
            dataclasses.replace(s, devices="c" if len(s.devices) == 1 else "cc") for s in self.stages))


def push_plan(case: Case) -> List[Tuple[bool, bool]]:
    """(data given, results given) of every push.  "both": every push has
    both.  "drain": data without results, then results without data.
    "gaps": both, with a push of neither and a push of each alone in between,
    so that every branch of the swap and counter rules runs after results
    flow."""
    P = case.pushes
    if case.mode == "both":
        return [(True, True)] * P
    if case.mode == "drain":
        return [(True, False)] * (P // 2) + [(False, True)] * (P - P // 2)
    odd = {2: (False, False), 5: (True, False), 7: (False, True), P - 2: (False, False)}
    return [odd.get(p, (True, True)) for p in range(P)]


A = StageSpec


def cases() -> List[Case]:
    """Stage shapes (stateful hidden, two kernels with a permuted hand-over,
    an output that only kernel 1 writes, an initializer), slice geometry (epw
    1 and 3, a per-group record of 7, a tail of 7, an input shorter than the
    output that feeds it), 1, 2 and 3 devices per stage and GPU + CPU, the
    transitions 3->1, 1->2, 2->3 (and 3->2, 2->1), the three push modes, the
    three data forms and the four element types."""
    return [
        Case("stateful-3-1-2", "int", (A("acc", "ggg"), A("acc", "g", E=3, tail=TAIL), A("acc", "gg"))),
        Case("epw3-tail-2-3", "ushort",
             (A("acc", "gg", E=3, tail=TAIL), A("acc", "ggg", E=3, tail=TAIL, xn=3 * N + TAIL)), mode="drain"),
        Case("two-kernel-3-1-2", "uchar", (A("two", "ggg"), A("join", "g"), A("two", "gg"))),
        Case("two-kernel-2-3", "llong", (A("two", "gg"), A("join", "ggg")), mode="gaps", data_form="list"),
        Case("init-2-3", "int", (A("init", "gg"), A("acc", "ggg", E=3)), data_form="strided"),
        Case("mixed-gc-1", "ushort", (A("acc", "gc"), A("two", "g")), mode="gaps"),
        Case("stateful-epw3-3", "uchar", (A("acc", "ggg", E=3, tail=TAIL),), mode="drain"),
    ]


def case_named(name: str) -> Case:
    return {c.name: c for c in cases()}[name]


FAULT_CASES = {
    "hidden_per_device": "stateful-3-1-2",
    "owner_last_kernel_only": "two-kernel-3-1-2",
    "owner_one_push_late": "stateful-3-1-2",
    "slice_no_epw": "epw3-tail-2-3",
    "slice_epg_as_epw": "two-kernel-3-1-2",
    "slice_ignores_item_size": "stateful-3-1-2",
    "tail_dropped": "epw3-tail-2-3",
    "swap_inputs_skipped": "two-kernel-2-3",
    "swap_outputs_without_results": "two-kernel-2-3",
    "ready_counter_off_by_one": "stateful-3-1-2",
    "transfer_to_device0_only": "stateful-3-1-2",
    "initializer_on_one_buffer_set": "init-2-3",
}


def initial(case: Case, stage: int, index: int, spec: BufSpec) -> np.ndarray:
    """Initial contents of buffer ``index`` of ``stage``: different in every
    buffer, so that stale or misplaced data differs from fresh data."""
    return stamp(case.dtype, spec.n, 0, 10 * stage + index + 1)


def push_values(case: Case, p: int) -> np.ndarray:
    """The values push ``p`` feeds into stage 0's first input."""
    return stamp(case.dtype, case.stages[0].xn, p + 1, 77)


def make_data(case: Case, p: int):
    """Push ``p``'s data in the case's form, and the object that must stay
    alive in the caller (none: the pipeline keeps what it copies)."""
    v = push_values(case, p)
    if case.data_form == "list":
        assert case.type_name == "llong", "a list is taken as int64"
        return [v.tolist()]
    if case.data_form == "strided":
        wide = np.zeros(2 * len(v), v.dtype)
        wide[::2] = v
        wide[1::2] = ~v
        return [wide[::2]]
    return [v]


def synthetic_splits(case: Case, p: int) -> List[List[Tuple[List[int], List[int]]]]:
    """Per stage, per kernel, (ranges, references) for push ``p`` of an
    emulated runtime: the split moves from push to push, the kernels of one
    stage split differently, and every device gets a slice."""
    out = []
    for si, s in enumerate(case.stages):
        D = len(s.devices)
        per_kernel = []
        for k in range(len(kernels_of(s)[0])):
            r = [N // D // L * L] * D
            r[0] += N - sum(r)
            if D > 1:
                shift = L * (1 + (p + 2 * k + si) % 4)
                a, b = (p + k) % D, (p + k + 1) % D
                r[a] -= shift
                r[b] += shift
            per_kernel.append((r, [sum(r[:d]) for d in range(D)]))
        out.append(per_kernel)
    return out


# ------------------------------------------------------------------ the ClPipeline emulator


class _Buf:
    """One buffer of a stage: the host array and the GPU-kind devices' replicas."""

    def __init__(self, spec: BufSpec, host: np.ndarray, kinds: Sequence[str]):
        self.spec, self.host = spec, host
        self.reps = [host.copy() if k == "gpu" else host for k in kinds]  # _setup uploads the host contents

    def clone(self, kinds) -> "_Buf":
        return _Buf(self.spec, self.host.copy(), kinds)


class _Stage:
    def __init__(self, case: Case, index: int, spec: StageSpec, kinds: List[str]):
        self.spec, self.kinds, self.D = spec, kinds, len(kinds)
        bufs = [_Buf(b, initial(case, index, j, b), kinds) for j, b in enumerate(buffers_of(spec))]
        self.ins = [b for b in bufs if b.spec.role == "in"]
        self.hids = [b for b in bufs if b.spec.role == "hid"]
        self.outs = [b for b in bufs if b.spec.role == "out"]
        self.in_dup = [b.clone(kinds) for b in self.ins]
        self.out_dup = [b.clone(kinds) for b in self.outs]
        self.names, self.init_names = kernels_of(spec)
        self.owner = None        # per output: (references, ranges) of its slices, or None: whole on device 0
        self.owner_next = None
        self.owner_prev = None


class Emulator:
    """``ClPipeline`` for one case.  ``coherent=True``: every stage on one
    device (the oracle).  Otherwise the stages' devices are the case's."""

    def __init__(self, case: Case, faults: Sequence[str] = (), coherent: bool = False,
                 per_device_outputs: bool = False, init_splits=None):
        unknown = set(faults) - set(FAULTS)
        if unknown:
            raise KeyError(f"unknown faults {sorted(unknown)}")
        self.case, self.faults, self.coherent = case, frozenset(faults), coherent
        self.per_device_outputs = per_device_outputs or bool(self.faults & set(PER_DEVICE_OUTPUTS))
        self.stages = []
        for i, s in enumerate(case.stages):
            kinds = ["gpu"] if coherent else ["gpu" if ch == "g" else "cpu" for ch in s.devices]
            self.stages.append(_Stage(case, i, s, kinds))
        self.counter = 0
        self.stats = {"p2p": 0, "h2d": 0, "d2h": 0, "host": 0}
        for i, st in enumerate(self.stages):  # make_pipeline: the initializers, on both buffer sets
            for dup in ((False,) if "initializer_on_one_buffer_set" in self.faults else (False, True)):
                for name in st.init_names:
                    split = init_splits[i] if init_splits else self._equal(st.D)
                    self._kernel(st, name, split, dup)

    @staticmethod
    def _equal(D: int):
        r = [N // D // L * L] * D
        r[0] += N - sum(r)
        return r, [sum(r[:d]) for d in range(D)]

    # ---- slices
    def _slice(self, spec: BufSpec, ref: int, rng: int, item: int, transfer: bool) -> Tuple[int, int]:
        """(byte offset, bytes) of the work items [ref, ref + rng) in a buffer,
        clamped to it.  ``transfer``: for a stage transition (the faults of
        ClPipelineStage._slices apply), else for the coherence gather."""
        f = self.faults if transfer else frozenset()
        nbytes = spec.n * item
        if spec.epg and "slice_epg_as_epw" not in f:
            b, c = ref // L * spec.epg, rng // L * spec.epg
        else:
            e = spec.epg if spec.epg else (1 if "slice_no_epw" in f else spec.epw)
            b, c = ref * e, rng * e
        if "slice_ignores_item_size" in f:
            item = 1
        b, c = min(b * item, nbytes), c * item
        return b, max(0, min(c, nbytes - b))

    def _slices(self, st: _Stage, k: int, buf: _Buf) -> List[Tuple[int, int, int]]:
        owner = None if st.owner is None else st.owner[k]
        nbytes = buf.host.nbytes
        if owner is None:
            return [(0, 0, nbytes)]
        refs, ranges = owner
        out = []
        for d, (r, n) in enumerate(zip(refs, ranges)):
            b, c = self._slice(buf.spec, r, n, buf.host.itemsize, True)
            if c:
                out.append((d, b, c))
        spec = buf.spec  # the tail: what no work item of the range owns
        end = (sum(ranges) // L * spec.epg if spec.epg else sum(ranges) * spec.epw) * buf.host.itemsize
        if end < nbytes and "tail_dropped" not in self.faults:
            out.append((0, end, nbytes - end))
        return out

    # ---- one kernel on one stage
    def _kernel(self, st: _Stage, name: str, split, dup: bool) -> None:
        ranges, refs = split if st.D > 1 else ([N], [0])
        bufs = (st.in_dup if dup else st.ins) + st.hids + (st.out_dup if dup else st.outs)
        k = numpy_kernel(st.spec, name)
        done = set()
        for d in range(st.D):
            reps = [b.reps[d] for b in bufs]
            k(reps, np.arange(refs[d], refs[d] + ranges[d], dtype=np.int64))
        if st.D == 1:
            return
        for b in bufs:  # the coherence rule
            if b.spec.role == "in" or b.spec.read_only or id(b) in done:
                continue
            if b.spec.role == "hid" and "hidden_per_device" in self.faults:
                continue
            if b.spec.role == "out" and self.per_device_outputs:
                continue
            done.add(id(b))
            for s in range(st.D):
                o, c = self._slice(b.spec, refs[s], ranges[s], b.host.itemsize, False)
                src = b.reps[s].view(np.uint8)
                for d in range(st.D):
                    if d != s and b.reps[d] is not b.reps[s]:
                        b.reps[d].view(np.uint8)[o:o + c] = src[o:o + c]

    # ---- transfers
    def _transfer(self, dst_st: Optional[_Stage], dst, src_st: Optional[_Stage], k: int, src) -> None:
        """ClPipeline's _transfer: ``dst`` / ``src`` are _Bufs on the stage
        sides and numpy arrays on the host side."""
        sbytes = src.host.nbytes if src_st else src.nbytes
        dbytes = dst.host.nbytes if dst_st else dst.nbytes
        n = min(sbytes, dbytes)
        if src_st is None:
            srcs = [("cpu", src, 0, n)]
        else:
            srcs = [(src_st.kinds[d], src.reps[d], b, min(c, n - b)) for d, b, c in self._slices(src_st, k, src)
                    if b < n]
        if dst_st is None:
            dsts = [("cpu", dst)]
        else:
            devs = [0] if "transfer_to_device0_only" in self.faults else range(dst_st.D)
            dsts = [(dst_st.kinds[d], dst.reps[d]) for d in devs]
        for dk, da in dsts:
            for sk, sa, b, c in srcs:
                if c <= 0 or da is sa:
                    continue
                da.view(np.uint8)[b:b + c] = sa.view(np.uint8)[b:b + c]
                path = "p2p" if dk == sk == "gpu" else "h2d" if dk == "gpu" else "d2h" if sk == "gpu" else "host"
                self.stats[path] += c

    # ---- one push
    def push(self, data: Optional[Sequence[np.ndarray]], results: Optional[Sequence[np.ndarray]], splits=None) -> bool:
        f = self.faults
        S = len(self.stages)
        splits = splits if splits is not None else [[self._equal(st.D)] * len(st.names) for st in self.stages]
        for st, per_kernel in zip(self.stages, splits):
            for ki, name in enumerate(st.names):
                self._kernel(st, name, per_kernel[ki], False)
        if data is not None:
            st = self.stages[0]
            for dst, d in zip(st.in_dup, data):
                self._transfer(st, dst, None, 0, np.ascontiguousarray(d).reshape(-1))
        for i in range(S - 1):
            st, nxt = self.stages[i], self.stages[i + 1]
            for k, (dst, src) in enumerate(zip(nxt.in_dup, st.out_dup)):
                self._transfer(nxt, dst, st, k, src)
        if results is not None:
            st = self.stages[S - 1]
            for k, (r, src) in enumerate(zip(results, st.out_dup)):
                self._transfer(None, r, st, k, src)
        for i, (st, per_kernel) in enumerate(zip(self.stages, splits)):
            if st.D == 1:
                st.owner_next = None
            else:
                writers = writer_of(st.spec)
                if not self.per_device_outputs or "owner_last_kernel_only" in f:
                    writers = [len(st.names) - 1] * len(writers)
                st.owner_next = [(list(per_kernel[w][1]), list(per_kernel[w][0])) for w in writers]
            later_input = i != 0 and "swap_inputs_skipped" not in f
            if data is not None or later_input:
                st.ins, st.in_dup = st.in_dup, st.ins
            if results is not None or i != S - 1 or "swap_outputs_without_results" in f:
                st.outs, st.out_dup = st.out_dup, st.outs
                st.owner = st.owner_prev if "owner_one_push_late" in f else st.owner_next
                st.owner_prev = st.owner_next
        self.counter += 1
        c = self.counter + (1 if "ready_counter_off_by_one" in f else 0)
        if data is None and results is None:
            return c > 2 * S - 2
        if data is not None and results is not None:
            return c > 2 * S
        return c > 2 * S - 1


def result_arrays(case: Case) -> List[np.ndarray]:
    """Zeroed arrays as long as the last stage's outputs."""
    return [np.zeros(b.n, case.dtype) for b in buffers_of(case.stages[-1]) if b.role == "out"]


def run_model(case: Case, faults: Sequence[str] = (), coherent: bool = False, per_device_outputs: bool = False,
              splits_of: Optional[Callable] = None) -> List[tuple]:
    """Every push of the case on an Emulator: per push (ready, results, bytes
    moved so far by path)."""
    emu = Emulator(case, faults, coherent, per_device_outputs)
    results = result_arrays(case)
    seen = []
    for p, (has_data, has_results) in enumerate(push_plan(case)):
        data = [np.asarray(d) for d in make_data(case, p)] if has_data else None
        splits = (splits_of or synthetic_splits)(case, p)
        ready = emu.push(data, results if has_results else None, splits)
        seen.append((ready, [r.copy() for r in results], dict(emu.stats)))
    return seen


def first_difference(a: List[tuple], b: List[tuple]) -> Optional[str]:
    """The first push at which two runs differ in the ready flag or in an
    element of the results, as text; None if they never do."""
    for p, ((ra, xa, _), (rb, xb, _)) in enumerate(zip(a, b)):
        if ra != rb:
            return f"push {p}: ready {ra} / {rb}"
        for k, (x, y) in enumerate(zip(xa, xb)):
            bad = np.flatnonzero(x != y)
            if len(bad):
                return f"push {p}, result {k}, element {bad[0]}: got {x[bad[0]]}, want {y[bad[0]]} ({len(bad)} differ)"
    return None


# ------------------------------------------------------------------ the real ClPipeline


class Mismatch(AssertionError):
    pass


def build_pipeline(case: Case, device_of: Callable[[str], object]):
    """The case as a real ClPipeline.  ``device_of(letter)`` gives the
    ClDevices for ``g`` and ``c``.  Returns (pipeline, stages)."""
    import cekirdekler_amd as ck
    from cekirdekler_amd.parallel.pipeline import ClPipelineStage

    ctype = TYPES[case.type_name][0]
    stages = []
    for i, s in enumerate(case.stages):
        st = ClPipelineStage()
        for ch in s.devices:
            st.add_devices(device_of(ch))
        names, inits = kernels_of(s)
        st.add_kernels(stage_source(s, ctype), " ".join(names), [N] * len(names), [L] * len(names))
        if inits:
            st.initializer_kernel(" ".join(inits), [N] * len(inits), [L] * len(inits))
        for j, b in enumerate(buffers_of(s)):
            a = ck.ClArray(initial(case, i, j, b))
            a.elements_per_work_item, a.elements_per_group = b.epw, b.epg
            if b.read_only:
                a.read_only = True
            {"in": st.add_input_buffers, "hid": st.add_hidden_buffers, "out": st.add_output_buffers}[b.role](a)
        if stages:
            st.append_to_stage(stages[-1])
        stages.append(st)
    return stages[0].make_pipeline(), stages


def run_pipeline(case: Case, pipe, stages, before_push: Optional[Callable] = None) -> dict:
    """Pushes the case through the real pipeline.  Returns ``seen`` (per push:
    ready, results, transfer_stats) and ``splits`` (per push, per stage, per
    kernel: (ranges, references) as the stage's cruncher reported them)."""
    results = result_arrays(case)
    seen, splits, gathers = [], [], []
    for p, (has_data, has_results) in enumerate(push_plan(case)):
        if before_push:
            before_push(p, stages)
        data = make_data(case, p) if has_data else None
        ready = pipe.push_data(data, results if has_results else None)
        del data
        st = pipe.transfer_stats()
        seen.append((bool(ready), [r.copy() for r in results], {k: st[k] for k in ("p2p", "h2d", "d2h", "host")}))
        splits.append([[(s.cruncher.ranges(1 + k), s.cruncher.references(1 + k)) for k in range(len(s.kernel_names))]
                       for s in stages])
        gathers.append([s.cruncher.last_record()["gather_bytes"] for s in stages])
    return {"seen": seen, "splits": splits, "gather_bytes": gathers}


def check_against_oracle(case: Case, seen: List[tuple], what: str) -> None:
    """Every push of a real run against the coherent emulator: the ready flag
    and every element of every result."""
    diff = first_difference(seen, run_model(case, coherent=True))
    if diff:
        raise Mismatch(f"{case.name}, {what}: {diff}")


# ------------------------------------------------------------------ DevicePipeline

DP_FEEDS = 8
DP_MODES = ("parallel", "serial", "callback", "begin_end")
DP_STOP_AFTER = 3   # stop_host_device_transmission is set on the first stage after this feed


def dp_source(ctype: str) -> str:
    """Three stages: a (inp -> t1), b = "dp_b1 dp_b2" (t1 -> acc -> t2, t1 and
    acc read at permuted indices), c (t2 at permuted indices -> out)."""
    return f"""typedef {ctype} T;
typedef unsigned long long U;
#define PM_N {N}LL
#define PM_PERM(i) (((i) * 31 + 7) % PM_N)
__global__ void dp_a(const T* inp, T* t1) {{
  const long long i = get_global_id(0);
  if (i < 0 || i >= PM_N) return;
  t1[i] = (T)(3ull * (U)inp[i] + (U)i);
}}
__global__ void dp_b1(const T* t1, T* acc, T* t2) {{
  const long long i = get_global_id(0);
  if (i < 0 || i >= PM_N) return;
  acc[i] = (T)((U)acc[i] + (U)t1[PM_PERM(i)] + 1ull);
}}
__global__ void dp_b2(const T* t1, T* acc, T* t2) {{
  const long long i = get_global_id(0);
  if (i < 0 || i >= PM_N) return;
  t2[i] = (T)((U)acc[PM_PERM(i)] + 2ull * (U)t1[i] + (U)i);
}}
__global__ void dp_c(const T* t2, T* out) {{
  const long long i = get_global_id(0);
  if (i < 0 || i >= PM_N) return;
  out[i] = (T)((U)t2[PM_PERM(i)] + 7ull * (U)i);
}}
"""


DP_ARRAYS = ("inp", "t1", "acc", "t2", "out")
DP_TYPES = {"inp": "INPUT", "t1": "TRANSITION", "acc": "INTERNAL", "t2": "TRANSITION", "out": "OUTPUT"}
DP_STAGES = (("dp_a", ("inp", "t1")), ("dp_b1 dp_b2", ("t1", "acc", "t2")), ("dp_c", ("t2", "out")))


DP_FAULT_CASES = {  # the layout is one; a case is the element type it runs with
    "transition_same_parity": "int",
    "output_wrong_parity": "uchar",
    "internal_double_buffered": "llong",
    "stop_still_uploads": "ushort",
}


def dp_initial(dtype, name: str) -> np.ndarray:
    return stamp(dtype, N, 0, 200 + DP_ARRAYS.index(name))


def dp_values(dtype, f: int) -> np.ndarray:
    """What the host writes into input_buffer() for feed ``f``: position- and
    feed-dependent."""
    return stamp(dtype, N, f + 1, 99)


def _dp_kernels():
    i = np.arange(N, dtype=np.int64)

    def a(inp, t1):
        t1[:] = (U(3) * _u(inp) + _u(i)).astype(t1.dtype)

    def b(t1, acc, t2):
        acc[:] = (_u(acc) + _u(t1[perm(i)]) + U(1)).astype(acc.dtype)
        t2[:] = (_u(acc[perm(i)]) + U(2) * _u(t1) + _u(i)).astype(t2.dtype)

    def c(t2, out):
        out[:] = (_u(t2[perm(i)]) + U(7) * _u(i)).astype(out.dtype)

    return (a, b, c)


class DpEmulator:
    """Parity emulator of DevicePipeline._args / feed / _finish on one device
    of ``kind``: per array two buffers (one for INTERNAL), each with a host
    side and, on a GPU, a device side that only uploads and downloads
    connect (the test uploads every buffer once before the first feed)."""

    def __init__(self, dtype, kind: str = "gpu", faults: Sequence[str] = ()):
        unknown = set(faults) - set(DP_FAULTS)
        if unknown:
            raise KeyError(f"unknown faults {sorted(unknown)}")
        self.faults, self.kind = frozenset(faults), kind
        self.host = {n: [dp_initial(dtype, n), dp_initial(dtype, n)] for n in DP_ARRAYS}
        self.dev = {n: [h.copy() if kind == "gpu" else h for h in self.host[n]] for n in DP_ARRAYS}
        self.parity = 0
        self.stop_first = False

    def input_buffer(self) -> np.ndarray:
        return self.host["inp"][1 - self.parity]

    def output_buffer(self) -> np.ndarray:
        return self.host["out"][self.parity if "output_wrong_parity" in self.faults else 1 - self.parity]

    def feed(self) -> None:
        p, f = self.parity, self.faults
        for si, ((_, names), k) in enumerate(zip(DP_STAGES, _dp_kernels())):
            stopped = si == 0 and self.stop_first
            args = []
            for n in names:
                t = DP_TYPES[n]
                if t == "INTERNAL":
                    q = p if "internal_double_buffered" in f else 0
                elif t == "TRANSITION":
                    producer = [s for s, (_, ns) in enumerate(DP_STAGES) if n in ns][0] == si
                    q = p if producer or "transition_same_parity" in f else 1 - p
                else:
                    q = p
                if t == "INPUT" and (not stopped or "stop_still_uploads" in f) and self.kind == "gpu":
                    self.dev[n][q][:] = self.host[n][q]
                args.append((n, q))
            k(*[self.dev[n][q] for n, q in args])
            for n, q in args:
                if DP_TYPES[n] == "OUTPUT" and not stopped and self.kind == "gpu":
                    self.host[n][q][:] = self.dev[n][q]
        self.parity ^= 1


def run_dp_model(dtype, kind: str = "gpu", faults: Sequence[str] = (), stop: bool = True) -> List[np.ndarray]:
    """output_buffer() after each of DP_FEEDS feeds."""
    emu = DpEmulator(dtype, kind, faults)
    outs = []
    for f in range(DP_FEEDS):
        emu.input_buffer()[:] = dp_values(dtype, f)
        emu.feed()
        outs.append(emu.output_buffer().copy())
        if stop and f == DP_STOP_AFTER:
            emu.stop_first = True
    return outs


def run_dp_real(device, type_name: str, mode: str, stop: bool = True) -> List[np.ndarray]:
    """The same feeds on a real DevicePipeline over ``device`` (one
    ClDevices), in one of DP_MODES."""
    import cekirdekler_amd as ck
    from cekirdekler_amd.parallel.pipeline import (DevicePipeline, DevicePipelineArray, DevicePipelineArrayType,
                                                   DevicePipelineStage)

    ctype, dtype = TYPES[type_name]
    dp = DevicePipeline(device, dp_source(ctype))
    try:
        arrays = {n: DevicePipelineArray(DevicePipelineArrayType[DP_TYPES[n]], ck.ClArray(dp_initial(dtype, n)))
                  for n in DP_ARRAYS}
        for a in arrays.values():  # device buffers start undefined: define every one once
            for buf in a.buffers():
                if buf is not None:
                    dp.cruncher.upload(buf, 0)
        stages = []
        for names, bound in DP_STAGES:
            st = DevicePipelineStage(names, N, L)
            for n in bound:
                st.bind_array(arrays[n])
            dp.add_stage(st)
            stages.append(st)
        if mode == "serial":
            dp.enable_serial_mode()
        outs = []
        inp, out = arrays["inp"], arrays["out"]
        for f in range(DP_FEEDS):
            # input_buffer() is the buffer this feed does not read: filling it
            # before the feed, in the callback or between begin and end is the
            # same write; the next feed consumes it

            def fill(f=f):
                dp.input_buffer(inp).array[:] = dp_values(dtype, f)

            if mode == "callback":
                dp.feed_async(fill)
            elif mode == "begin_end":
                dp.feed_async_begin()
                fill()
                dp.feed_async_end()
            else:
                fill()
                dp.feed()
            outs.append(dp.output_buffer(out).array.copy())
            if stop and f == DP_STOP_AFTER:
                stages[0].stop_host_device_transmission = True
        return outs
    finally:
        dp.dispose()
