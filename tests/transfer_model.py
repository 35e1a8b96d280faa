"""Executable model of compute()'s data movement (csrc/cores_run.cpp, csrc/peer.cpp), its probe
kernels, its case generators and the harness that runs one case against a
backend.  tests/test_transfer_model.py is the CPU tier, tests/
test_gpu_transfer_model.py the GPU tier; docs/API.md states the same rules
in prose.

The model is a numpy emulator of one cruncher: the host arrays and, per
(device, array), one replica.  A GPU-kind device has a buffer of its own; a
CPU-kind device, and a zero-copy array on any device, uses the host array
itself (Replicas::buffer).  One call applies, in order: the uploads (from
the host as it was before the call), the kernel on every device's work items,
the downloads, the keep-resident gather; and it counts the bytes the runtime
reports as h2d_bytes / d2h_bytes.  The ranges and references are the ones the
real call reported (last_record()), so the model never predicts the balancer.
A pipelined call uploads partial_read arrays blob by blob; run_case bounds what
a kernel may see of the device's other blobs with a second emulator
(``lazy_blobs``) and accepts either, element by element.

Everything is integer and every comparison exact.  ``faults=`` switches single
rules to a wrong version: the CPU tier shows that each such runtime would be
caught by a named case (FAULT_CASES).
"""
from __future__ import annotations

import dataclasses
import itertools
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

# ------------------------------------------------------------------ constants

L = 64          # local range of every case
BLOBS = 4       # pipeline blobs
TAIL = 7        # elements past the last work item's own ones in the "tail" cases
IDS_EPW = 10    # the ids kernel's record per work item
IDS_CAP = 3 * L * 4 * 2 + 2 * L   # most work items any case addresses (offset + G at D = 3)

TYPES = {  # name -> (C type, numpy dtype)
    "uchar": ("unsigned char", np.uint8),
    "ushort": ("unsigned short", np.uint16),
    "int": ("int", np.int32),
    "llong": ("long long", np.int64),
}

FAULTS = (
    "partial_uploads_all",        # partial_read uploads everything
    "partial_no_epw",             # the partial slice is taken without the epw factor
    "partial_prev_ranges",        # the partial slice uses the previous call's ranges
    "partial_shift_group",        # the partial slice is shifted by one work-group
    "read_skipped",               # read is skipped
    "read_when_off",              # read is done although the flag is off
    "read_wins_over_partial",     # read wins over partial_read
    "write_whole_replica",        # write downloads the whole replica from each device
    "write_no_epw",               # the write slice is taken without epw
    "download_without_write",     # a download happens with write off
    "write_all_owner0",           # the write_all owner is always device 0
    "write_all_without_write",    # write_all downloads without write
    "write_all_slices",           # write_all downloads only slices
    "epg_as_epw",                 # elements_per_group is treated as epw
    "epg_from_ref",               # the epg slice is taken from ref*g
    "offset_dropped_slices",      # the global offset is dropped from the slices
    "offset_dropped_ids",         # the global offset is dropped from the kernel's ids
    "zero_copy_copied",           # a zero-copy array is a copied array with its flags
    "no_phase_separation",        # device d uploads after device d-1 has downloaded
    "gather_missing",             # the gather is missing
    "gather_dev0_only",           # the gather goes only to device 0
    "zero_range_transfers",       # a device with range 0 still transfers
    "repeat_reuploads",           # repeat re-uploads between repetitions
    "bytes_by_epw",               # byte counts are off by the epw factor
    "gather_before_downloads",    # the gather runs before the downloads (a write_all owner would bring it back)
)

PATHS = ("plain", "event", "driver", "repeat", "enqueue", "async", "graph")
REPEATS = 3

# ------------------------------------------------------------------ stamping


def stamp(dtype, n: int, version: int, tag: int) -> np.ndarray:
    """Host contents of array ``tag`` at ``version``: (version, index) through
    an odd multiplier, so that at one index two versions less than 2^bits/4099
    apart never agree (8-bit elements alias across indices; the wider types
    carry the proof)."""
    k = np.arange(n, dtype=np.uint64)
    v = (np.uint64(version * 4099 + tag * 1000003 + 1) + k) * np.uint64(2654435761)
    return v.astype(dtype)


# ------------------------------------------------------------------ arrays and flags

SRC_FLAGS = ("read", "partial", "both", "neither", "read_only", "zero_copy")
DST_FLAGS = ("write", "write_all", "all_alone", "neither", "write_only", "inplace", "zero_copy", "gather",
             "all_gather")


def user_settings(role: str, name: str) -> List[Tuple[str, bool]]:
    """The attribute assignments a user makes, in order, on a fresh ClArray
    (defaults: read and write on) to get flag set ``name``."""
    if role == "src":
        return {
            "read": [("write", False)],
            "partial": [("write", False), ("read", False), ("partial_read", True)],
            "both": [("write", False), ("partial_read", True)],
            "neither": [("write", False), ("read", False)],
            "read_only": [("read_only", True)],
            "zero_copy": [("write", False), ("zero_copy", True)],
        }[name]
    return {
        "write": [("read", False)],
        "write_all": [("read", False), ("write_all", True)],
        "all_alone": [("read", False), ("write", False), ("write_all", True)],
        "neither": [("read", False), ("write", False)],
        "write_only": [("write_only", True)],
        "inplace": [],
        "zero_copy": [("read", False), ("zero_copy", True)],
        "gather": [("read", False), ("gather_resident", True)],
        "all_gather": [("read", False), ("write_all", True), ("gather_resident", True)],
        "observe": [("read", False)],
        "const": [("read_only", True)],
    }[name]


@dataclasses.dataclass
class Flags:
    """What the native layer sees of one array (arrays.py's exclusion rules
    applied): read_only clears write and write_all and then refuses them,
    write_only clears read and partial_read and then refuses them, and each
    of the two is refused while the other is on."""
    read: bool = True
    partial: bool = False
    write: bool = True
    write_all: bool = False
    ro: bool = False
    wo: bool = False
    zc: bool = False
    gather: bool = False

    def assign(self, attr: str, v: bool) -> None:
        if attr == "read":
            if not self.wo:
                self.read = v
        elif attr == "partial_read":
            if not self.wo:
                self.partial = v
        elif attr == "write":
            if not self.ro:
                self.write = v
        elif attr == "write_all":
            if not self.ro:
                self.write_all = v
        elif attr == "read_only":
            if v and not self.wo:
                self.write = self.write_all = False
                self.ro = True
            elif not v:
                self.ro = False
        elif attr == "write_only":
            if v and not self.ro:
                self.read = self.partial = False
                self.wo = True
            elif not v:
                self.wo = False
        elif attr == "zero_copy":
            self.zc = v
        elif attr == "gather_resident":
            self.gather = v
        else:
            raise KeyError(attr)

    def primed(self) -> "Flags":
        """The first call of every sequence: plain read, nothing back."""
        return Flags(read=True, partial=False, write=False, write_all=False, zc=self.zc)

    def resident(self) -> "Flags":
        """No host transfer at all (the chained calls of an enqueued batch)."""
        return Flags(read=False, partial=False, write=False, write_all=False, zc=self.zc)


def flags_of(role: str, name: str) -> Flags:
    f = Flags()
    for attr, v in user_settings(role, name):
        f.assign(attr, v)
    return f


@dataclasses.dataclass
class Arr:
    """One kernel parameter as the model sees it."""
    host: np.ndarray
    flags: Flags
    epw: int = 1
    epg: int = 0


# ------------------------------------------------------------------ launches


def launch_plan(path: str, ref: int, rng: int, pipelined: bool) -> List[Tuple[int, int]]:
    """(offset, count) of every kernel launch one device makes for its range.
    The plain path launches once; a pipelined call launches once per blob:
    the driver pipeline in order, the event pipeline alternating between its
    two half-pipelines (Cores::run_event_pipeline / run_driver_pipeline)."""
    if rng <= 0:
        return []
    if not pipelined:
        return [(ref, rng)]
    chunk = rng // BLOBS
    if path == "driver":
        return [(ref + k * chunk, chunk) for k in range(BLOBS)]
    halves = 2 if BLOBS % 2 == 0 else 1
    return [(ref + (q % halves) * (rng // halves) + (q // halves) * chunk, chunk) for q in range(BLOBS)]


def expect_pipelined(path: str, arrs: Sequence[Arr], ranges: Sequence[int], D: int) -> bool:
    """Cores::compute_once: a pipeline is taken unless an array is read whole
    and written back on several devices (phase separation), an array gathers,
    or a range is not a whole number of blobs."""
    if path not in ("event", "driver"):
        return False
    for a in arrs:
        f = a.flags
        if not f.zc and f.gather:
            return False
        if D > 1 and not f.zc and f.read and not f.partial and f.write:
            return False
    return all(r == 0 or (r % (BLOBS * L) == 0) for r in ranges)


# ------------------------------------------------------------------ kernels (model side)

U = np.uint64


def _u(x) -> np.ndarray:
    """The C conversion (unsigned long long)x: signed types sign-extend."""
    return np.asarray(x).astype(U)


def probe_kernel(E: int, F: int) -> Callable:
    """probe_E_F(src, dst, seen, par): see probe_source()."""

    def k(reps: List[np.ndarray], items: np.ndarray, launch_off: int, G: int, *launch) -> None:
        src, dst, seen, par = reps
        c, lim = int(par[0]), int(par[1])
        i = items[(items >= 0) & (items < lim)]
        if not len(i):
            return
        own = i * E + (i + c) % E
        mir = G * E - 1 - own % (G * E)
        ks = [i * E + e for e in range(E)]
        olds = [_u(dst[kk]) for kk in ks]
        for e, kk in enumerate(ks):
            new = _u(src[kk]) + U(3) * olds[e] + U(5) * i.astype(U) + U(7) * U(c) + U(e)
            dst[kk] = new.astype(dst.dtype)
        last = np.select([own == kk for kk in ks], olds)
        for j in range(F):
            kind = (i + c + j) & 3
            v = np.select([kind == 0, kind == 1, kind == 2],
                          [_u(src[own]), _u(src[mir]), _u(src[np.zeros_like(i)])], last)
            seen[i * F + j] = (v + kind.astype(U)).astype(seen.dtype)

    return k


def group_kernel(E: int, g: int) -> Callable:
    """probeg_E_g(src, dst, grp, par): dst as in probe; the first work item of
    every work-group writes the group's ``g`` elements of ``grp``."""
    base = probe_kernel(E, 1)

    def k(reps: List[np.ndarray], items: np.ndarray, launch_off: int, G: int, *launch) -> None:
        src, dst, grp, par = reps
        c, lim = int(par[0]), int(par[1])
        i = items[(items >= 0) & (items < lim)]
        heads = i[(i - launch_off) % L == 0]
        vals = {}
        for j in range(g):
            vals[j] = (_u(src[heads * E]) + U(13) * U(j) + U(c) + (heads // L).astype(U))
        scratch = np.zeros(int(lim) + 1, grp.dtype)  # probe's seen: not kept
        base([src, dst, scratch, par], items, launch_off, G)
        for j in range(g):
            grp[heads // L * g + j] = vals[j].astype(grp.dtype)

    return k


def ids_kernel(reps: List[np.ndarray], items: np.ndarray, launch_off: int, G: int, launch_n: int = 0,
               kind: str = "gpu") -> None:
    """``launch_n``: the work items of the launch.  cek_local_num_groups() is
    the launch's group count on a GPU (gridDim.x); the CPU device's runner
    sets gridDim.x to the call's G / L (jit.cpp, __cek_run_*)."""
    (out,) = reps
    local_groups = launch_n // L if kind == "gpu" else G // L
    i = items[(items >= 0) & (items < IDS_CAP)]
    rec = [i, (i - launch_off) % L, (i - launch_off) // L, np.full_like(i, L), np.full_like(i, G),
           np.full_like(i, G // L), np.full_like(i, launch_off), i // L, (i - launch_off) // L,
           np.full_like(i, local_groups)]
    for s, v in enumerate(rec):
        out[i * IDS_EPW + s] = v


# ------------------------------------------------------------------ kernels (device side)


def probe_source(ctype: str) -> str:
    """The probe kernels in the project's kernel dialect, for one element
    type.  Every index is inside its array whatever the launch offset and the
    ranges are: a work item outside [0, offset + G) returns, its own elements
    are below (offset + G)·E, the mirrored element is taken inside [0, G·E)
    with the launch's own G, and the ids record is capped by a constant."""
    out = [f"typedef {ctype} T;\ntypedef unsigned long long U;\n#define CEK_L {L}\n#define IDS_CAP {IDS_CAP}\n"]
    for E, F in itertools.product((1, 2, 3), (1, 2, 3)):
        out.append(f"""
__global__ void probe_{E}_{F}(const T* src, T* dst, T* seen, const long long* par) {{
  const long long E = {E}, F = {F}, c = par[0], lim = par[1];
  const long long i = get_global_id(0), G = get_global_size(0);
  if (i < 0 || i >= lim) return;
  const long long own = i * E + (i + c) % E;
  const long long mir = G * E - 1 - own % (G * E);
  U last = 0;
  for (long long e = 0; e < E; ++e) {{
    const long long k = i * E + e;
    const U old = (U)dst[k];
    dst[k] = (T)((U)src[k] + 3ull * old + 5ull * (U)i + 7ull * (U)c + (U)e);
    if (k == own) last = old;
  }}
  for (long long j = 0; j < F; ++j) {{
    const long long kind = (i + c + j) & 3;
    const U v = kind == 0 ? (U)src[own] : kind == 1 ? (U)src[mir] : kind == 2 ? (U)src[0] : last;
    seen[i * F + j] = (T)(v + (U)kind);
  }}
}}
""")
    for E, g in ((2, 2), (1, 3)):
        out.append(f"""
__global__ void probeg_{E}_{g}(const T* src, T* dst, T* grp, const long long* par) {{
  const long long E = {E}, g = {g}, c = par[0], lim = par[1];
  const long long i = get_global_id(0);
  if (i < 0 || i >= lim) return;
  const U head = (U)src[i * E];
  for (long long e = 0; e < E; ++e) {{
    const long long k = i * E + e;
    dst[k] = (T)((U)src[k] + 3ull * (U)dst[k] + 5ull * (U)i + 7ull * (U)c + (U)e);
  }}
  if (get_local_id(0) == 0)
    for (long long j = 0; j < g; ++j) grp[i / CEK_L * g + j] = (T)(head + 13ull * (U)j + (U)c + (U)(i / CEK_L));
}}
""")
    out.append(f"""
__global__ void ids(long long* out) {{
  const long long i = get_global_id(0);
  if (i < 0 || i >= IDS_CAP) return;
  long long* o = out + i * {IDS_EPW};
  o[0] = i; o[1] = get_local_id(0); o[2] = get_group_id(0); o[3] = get_local_size(0);
  o[4] = get_global_size(0); o[5] = get_num_groups(0); o[6] = get_global_offset(0); o[7] = cek_global_group_id();
  o[8] = cek_local_group_id(); o[9] = cek_local_num_groups();
}}
""")
    out.append(f"""
__global__ void idsr(long long* out) {{
  const long long l = get_local_id(0);
  if (l < 0 || l >= CEK_L) return;
  long long* o = out + (IDS_CAP - CEK_L + l) * {IDS_EPW};
  o[0] = get_global_id(0); o[1] = l; o[2] = get_group_id(0); o[3] = get_local_size(0);
  o[4] = get_global_size(0); o[5] = get_num_groups(0); o[6] = get_global_offset(0); o[7] = cek_global_group_id();
  o[8] = cek_local_group_id(); o[9] = cek_local_num_groups();
}}
""")
    return "".join(out)


# ------------------------------------------------------------------ the emulator


class Emulator:
    """One cruncher over ``kinds`` (a "gpu" or "cpu" per device)."""

    def __init__(self, kinds: Sequence[str], faults: Sequence[str] = (), lazy_blobs: bool = False):
        # lazy_blobs: in a pipelined call a blob's kernels see only their own
        # blob's slice of a partial_read array uploaded, not the device's
        # other blobs (see run_case)
        self.lazy_blobs = lazy_blobs
        unknown = set(faults) - set(FAULTS)
        if unknown:
            raise KeyError(f"unknown faults {sorted(unknown)}")
        self.kinds = list(kinds)
        self.D = len(kinds)
        self.faults = frozenset(faults)
        self.replicas: Dict[Tuple[int, int], np.ndarray] = {}
        self.prev: Optional[Tuple[List[int], List[int]]] = None

    # ---- storage
    def copied(self, a: Arr) -> bool:
        return not a.flags.zc or "zero_copy_copied" in self.faults

    def replica(self, d: int, i: int, a: Arr) -> np.ndarray:
        if not self.copied(a) or self.kinds[d] == "cpu":
            return a.host
        r = self.replicas.get((d, i))
        if r is None or len(r) != len(a.host) or r.dtype != a.host.dtype:
            # a device buffer starts undefined: the sequences prime it first
            r = self.replicas[(d, i)] = np.full_like(a.host, 0x5A)
        return r

    # ---- ArraySpec::slice, clamped to the array (Worker::h2d / d2h)
    def slice(self, a: Arr, ref: int, rng: int, offset: int, up: bool) -> Tuple[int, int]:
        f = self.faults
        if "offset_dropped_slices" in f:
            ref -= offset
        if up and "partial_shift_group" in f:
            ref += L
        if a.epg > 0 and "epg_as_epw" not in f:
            b = ref * a.epg if "epg_from_ref" in f else ref // L * a.epg
            n = rng // L * a.epg
        else:
            e = a.epg if a.epg > 0 else a.epw
            if (up and "partial_no_epw" in f) or (not up and "write_no_epw" in f):
                e = 1
            b, n = ref * e, rng * e
        b = max(0, min(b, len(a.host)))
        return b, max(0, min(n, len(a.host) - b))

    def _bytes(self, a: Arr, n: int) -> int:
        if "bytes_by_epw" in self.faults and a.epg == 0:
            n //= a.epw
        return n * a.host.itemsize

    # ---- one device's phases
    def _upload(self, d, arrs, before, ref, rng, offset) -> int:
        f = self.faults
        up = 0
        for i, a in enumerate(arrs):
            if not self.copied(a):
                continue
            src = a.host if "no_phase_separation" in f else before[i]
            rep = self.replica(d, i, a)
            partial, read = a.flags.partial, a.flags.read
            if "read_wins_over_partial" in f and read:
                partial = False
            if partial:
                if "partial_uploads_all" in f:
                    b, n = 0, len(a.host)
                elif "partial_prev_ranges" in f and self.prev is not None:
                    b, n = self.slice(a, self.prev[1][d], self.prev[0][d], offset, True)
                else:
                    b, n = self.slice(a, ref, rng, offset, True)
                if rep is not a.host:
                    rep[b:b + n] = src[b:b + n]
                up += self._bytes(a, n)
            elif (read and "read_skipped" not in f) or (not read and "read_when_off" in f):
                if rep is not a.host:
                    rep[:] = src
                up += a.host.nbytes
        return up

    def _download(self, d, arrs, ref, rng, offset) -> int:
        f = self.faults
        down = 0
        for i, a in enumerate(arrs):
            if not self.copied(a):
                continue
            rep = self.replica(d, i, a)
            fl = a.flags
            whole = None
            if fl.write_all and (fl.write or "write_all_without_write" in f):
                owner = 0 if "write_all_owner0" in f else i % self.D
                if "write_all_slices" in f:
                    whole = False
                elif owner == d:
                    whole = True
            elif fl.write or "download_without_write" in f:
                whole = "write_whole_replica" in f
            if whole is None:
                continue
            b, n = (0, len(a.host)) if whole else self.slice(a, ref, rng, offset, False)
            if rep is not a.host:
                a.host[b:b + n] = rep[b:b + n]
            down += a.host.nbytes if whole else self._bytes(a, n)
        return down

    def _kernels(self, d, arrs, kernel, launches, G, offset, repeats, before, ref, rng, old=None) -> int:
        up = 0
        reps = [self.replica(d, i, a) for i, a in enumerate(arrs)]
        for r in range(repeats):
            if r and "repeat_reuploads" in self.faults:
                up += self._upload(d, arrs, before, ref, rng, offset)
            for off, n in launches:
                items = np.arange(off, off + n, dtype=np.int64)
                seen_by_blob = list(reps)
                for i, was in (old or {}).items():  # only this blob's slice of a partial array is up
                    b, k = self.slice(arrs[i], off, n, offset, True)
                    seen_by_blob[i] = was.copy()
                    seen_by_blob[i][b:b + k] = before[i][b:b + k]
                if "offset_dropped_ids" in self.faults:
                    items, off = items - offset, off - offset
                kernel(seen_by_blob, items, off, G, n, self.kinds[d])
        return up

    # ---- one compute()
    def call(self, arrs: Sequence[Arr], kernel: Callable, G: int, offset: int, ranges: Sequence[int],
             references: Sequence[int], enabled: Optional[Sequence[bool]] = None, repeats: int = 1,
             path: str = "plain", pipelined: bool = False) -> Tuple[int, int]:
        """Applies the call to the host arrays and replicas; returns the
        (h2d_bytes, d2h_bytes) the runtime reports for it."""
        f = self.faults
        D = self.D
        enabled = [r > 0 for r in ranges] if enabled is None else list(enabled)
        before = [a.host.copy() for a in arrs]
        active = [d for d in range(D) if ranges[d] > 0 or "zero_range_transfers" in f]
        plans = {d: launch_plan(path, references[d], ranges[d], pipelined) for d in active}
        up = down = 0
        if "no_phase_separation" in f:
            for d in active:
                up += self._upload(d, arrs, before, references[d], ranges[d], offset)
                up += self._kernels(d, arrs, kernel, plans[d], G, offset, repeats, before, references[d], ranges[d])
                down += self._download(d, arrs, references[d], ranges[d], offset)
            self._gather(arrs, ranges, references, enabled, offset)
        else:
            old = {d: {} for d in active}
            if self.lazy_blobs and pipelined:
                for d in active:
                    for i, a in enumerate(arrs):
                        if a.flags.partial and self.copied(a) and self.kinds[d] == "gpu":
                            old[d][i] = self.replica(d, i, a).copy()
            for d in active:
                up += self._upload(d, arrs, before, references[d], ranges[d], offset)
            for d in active:
                up += self._kernels(d, arrs, kernel, plans[d], G, offset, repeats, before, references[d], ranges[d],
                                    old[d])
            # every device downloads inside its own part of the call
            # (run_3phase, phase 3), and compute_once issues the gather once
            # every device has returned: the gather follows the downloads
            if "gather_before_downloads" in f:
                self._gather(arrs, ranges, references, enabled, offset)
            for d in active:
                down += self._download(d, arrs, references[d], ranges[d], offset)
            if "gather_before_downloads" not in f:
                self._gather(arrs, ranges, references, enabled, offset)
        self.prev = (list(ranges), list(references))
        return up, down

    def _gather(self, arrs, ranges, references, enabled, offset) -> None:
        """PeerTraffic::issue_gather: with two or more enabled devices, every
        device's slice of a gather array goes into every other enabled
        device's replica (a CPU device's replica is the host array)."""
        f = self.faults
        on = [d for d in range(self.D) if enabled[d]]
        if len(on) < 2 or "gather_missing" in f:
            return
        for i, a in enumerate(arrs):
            if not a.flags.gather or not self.copied(a):
                continue
            for s in on:
                b, n = self.slice(a, references[s], ranges[s], offset, False)
                src = self.replica(s, i, a)
                for d in ([0] if "gather_dev0_only" in f else on):
                    dst = self.replica(d, i, a)
                    if d != s and dst is not src:
                        dst[b:b + n] = src[b:b + n]


# ------------------------------------------------------------------ cases


@dataclasses.dataclass(frozen=True)
class Case:
    """One sequence of calls on one compute id."""
    name: str
    src: str = "partial"
    dst: str = "write"
    E: int = 2
    F: int = 3
    offset: int = 0
    tail: int = 0
    path: str = "plain"
    epg: int = 0          # > 0: the third array is per-group with this many elements
    kernel: str = "probe"  # or "ids"
    late: Tuple[str, str] = ("", "")  # (src, dst) flag sets from the rejoining call on, if they change
    short: bool = False   # arrays sized for G work items although the offset is not 0: the slices are clipped

    def __str__(self) -> str:
        return self.name


def flag_cases() -> List[Case]:
    """Every src × dst flag set on the plain path; E, F, the offset and the
    tail rotate so that each value meets each flag set of the other array."""
    out = []
    for n, (s, d) in enumerate(itertools.product(SRC_FLAGS, DST_FLAGS)):
        si, di = SRC_FLAGS.index(s), DST_FLAGS.index(d)
        out.append(Case(f"flags-{s}-{d}", s, d, E=1 + (si + di) % 3, F=1 + (si + 2 * di) % 3,
                        offset=(2 * L if (si + di) % 2 else 0), tail=(TAIL if di % 2 else 0)))
    return out


def epw_cases() -> List[Case]:
    return [Case(f"epw-{E}-{F}", "partial", "write", E=E, F=F, offset=2 * L, tail=TAIL)
            for E, F in itertools.product((1, 2, 3), (1, 2, 3))]


def epg_cases() -> List[Case]:
    return [Case("epg-2x2", "partial", "write", E=2, epg=2, offset=0, tail=0),
            Case("epg-1x3-offset", "partial", "write_all", E=1, epg=3, offset=2 * L, tail=TAIL),
            Case("epg-2x2-offset", "read", "write", E=2, epg=2, offset=2 * L, tail=TAIL)]


PATH_FLAGS = (("partial", "write"), ("read", "write_all"), ("neither", "neither"), ("both", "inplace"),
              ("partial", "gather"), ("zero_copy", "zero_copy"))


def path_cases(paths: Sequence[str] = PATHS[1:]) -> List[Case]:
    out = []
    for p in paths:
        for n, (s, d) in enumerate(PATH_FLAGS):
            if p == "graph" and d == "gather":
                continue  # refused: keep-resident gather arrays cannot be captured
            out.append(Case(f"{p}-{s}-{d}", s, d, E=1 + n % 3, F=1 + (n + 1) % 3,
                            offset=(2 * L if n % 2 else 0), tail=(TAIL if n % 2 else 0), path=p))
    return out


def ids_cases(paths: Sequence[str] = PATHS) -> List[Case]:
    return [Case(f"ids-{p}-{o}", kernel="ids", path=p, offset=o) for p in paths for o in (0, 2 * L)]


def late_cases() -> List[Case]:
    """The flags change in mid-sequence, so that what a call left in a replica
    outside the device's slice is looked at by the next call: an in-place dst
    becomes write without read (phase separation: device 1 must have uploaded
    the host as it was before device 0 wrote its slice back), a read src
    becomes resident (a device that sat a call out kept its old replica)."""
    return [Case("late-read-inplace", "read", "inplace", E=2, F=3, offset=2 * L, tail=TAIL, late=("neither", "write")),
            Case("late-partial-gather", "partial", "gather", E=3, F=1, late=("neither", "neither"))]


def clip_cases() -> List[Case]:
    """Arrays as long as compute() asks for, G·epw elements, with a global
    offset: the last slices run past the arrays' ends and are clipped there,
    in what moves and in the byte counts (the work items past the end return)."""
    return [Case("clip-partial-write", "partial", "write", E=2, F=3, offset=2 * L, short=True),
            Case("clip-both-write_all", "both", "write_all", E=3, F=1, offset=2 * L, short=True)]


def global_range(D: int) -> int:
    """Two work-groups per blob per device: the smallest size at which a slice
    shifted by one group, a moved partition and a blob boundary all show."""
    return D * L * BLOBS * 2


# ------------------------------------------------------------------ one case's arrays


class Plan:
    """The arrays of one case for ``D`` devices and one element type, and the
    per-call flag sets.  ``alloc(n, dtype)`` makes a host array."""

    def __init__(self, case: Case, D: int, dtype, alloc: Callable = None):
        alloc = alloc or (lambda n, dt: np.zeros(n, dt))
        self.case, self.D, self.dtype = case, D, np.dtype(dtype)
        self.G = G = global_range(D)
        lim = G if case.short else case.offset + G
        if case.kernel == "ids":
            self.kernel_name = "ids"
            self.kernel = ids_kernel
            self.lengths = [IDS_CAP * IDS_EPW + TAIL]
            self.dtypes = [np.dtype(np.int64)]
            self.epw, self.epg = [IDS_EPW], [0]
            self.case_flags = [flags_of("dst", "observe")]
        else:
            E = case.E
            if case.epg:
                self.kernel_name = f"probeg_{E}_{case.epg}"
                self.kernel = group_kernel(E, case.epg)
                third, epw3, epg3 = lim // L * case.epg + case.tail, 1, case.epg
            else:
                self.kernel_name = f"probe_{E}_{case.F}"
                self.kernel = probe_kernel(E, case.F)
                third, epw3, epg3 = lim * case.F + case.tail, case.F, 0
            self.lengths = [lim * E + case.tail, lim * E + case.tail, third, 2]
            self.dtypes = [self.dtype, self.dtype, self.dtype, np.dtype(np.int64)]
            self.epw, self.epg = [E, E, epw3, 1], [0, 0, epg3, 0]
            self.case_flags = [flags_of("src", case.src), flags_of("dst", case.dst), flags_of("dst", "observe"),
                               flags_of("dst", "const")]
        self.lim = lim
        self.hosts = [alloc(n, dt) for n, dt in zip(self.lengths, self.dtypes)]

    def arrs(self, hosts: Sequence[np.ndarray], flags: Sequence[Flags]) -> List[Arr]:
        return [Arr(h, f, e, g) for h, f, e, g in zip(hosts, flags, self.epw, self.epg)]

    def rewrite(self, hosts: Sequence[np.ndarray], version: int, counter: int) -> None:
        """The host arrays at ``version``; the call counter goes into par."""
        for t, h in enumerate(hosts):
            if self.case.kernel != "ids" and t == 3:
                h[:] = (counter, self.lim)
            else:
                h[:] = stamp(h.dtype, len(h), version, t)


@dataclasses.dataclass
class Step:
    """One compute() of a sequence."""
    flags: str = "case"           # "prime", "case", "late" or "resident" (dst without any transfer)
    rewrite: bool = True          # host arrays go to a new version before the call
    partition: Optional[str] = None  # "prime", "primed", "drop", "rejoin", "skew": applied before the call
    mode: str = ""                # "enter": enqueue mode on before; "leave": off after; "capture"; "replay"
    check: bool = True            # compare the host arrays after this call


def steps_of(case: Case, D: int) -> List[Step]:
    """Call 0 primes every replica with a plain read (device buffers start
    undefined); the host arrays get a new version before every call; the
    partition changes by disable_device / enable_device / set_time_scale."""
    many = D > 1
    head = [Step("prime", partition="prime"), Step(partition="primed"), Step(partition="drop" if many else None)]
    if case.path == "enqueue":
        # the batch: k+1 consumes what k left in the replica (no host transfer
        # for dst), the host is only compared once the mode is left
        return head + [Step(partition="rejoin" if many else None),
                       Step("resident", mode="enter", check=False), Step("resident", rewrite=False, check=False),
                       Step(rewrite=False, mode="leave")]
    if case.path == "async":
        # async enqueue puts successive computes on different streams and does
        # not order them: a batch holds independent computes only, here one
        return head + [Step(partition="rejoin" if many else None), Step(mode="enter leave")]
    if case.path == "graph":
        return head + [Step(partition="rejoin" if many else None), Step(mode="capture", check=False),
                       Step(mode="replay")]
    tail = "late" if case.late[0] else "case"
    return head + [Step(tail, partition="rejoin" if many else None), Step(tail, partition="skew" if many else None)]


def synthetic_ranges(D: int, G: int, partition_state: str) -> List[int]:
    """The partition an emulated runtime reports (the real one asks its
    balancer): equal, without the last device, or skewed by one blob step."""
    if D == 1:
        return [G]
    if partition_state == "drop":
        r = [G // (D - 1)] * (D - 1) + [0]
        r[0] += G - sum(r)
        return r
    r = [G // D] * D
    if partition_state == "skew":
        r[0] -= BLOBS * L
        r[1] += BLOBS * L
    return r


# ------------------------------------------------------------------ backends


class EmulatorBackend:
    """A runtime that is an Emulator (honest, or with faults)."""

    def __init__(self, kinds: Sequence[str], faults: Sequence[str] = ()):
        self.emu = Emulator(kinds, faults)
        self.kinds = list(kinds)
        self.state = "equal"
        self.frozen = None
        self.captured = None

    def alloc(self, n, dt):
        return np.zeros(n, dt)

    def new_case(self) -> None:
        pass

    def begin(self, plan: Plan) -> None:
        self.plan = plan

    def effective(self, flags: Sequence[Flags]) -> List[Flags]:
        return list(flags)

    def partition(self, what: str) -> None:
        self.state = {"prime": "equal", "primed": "equal", "drop": "drop", "rejoin": "equal", "skew": "skew"}[what]

    def run(self, plan: Plan, flags, step: Step, path: str) -> Optional[dict]:
        D, G = plan.D, plan.G
        case = plan.case
        if step.mode == "replay":
            flags, ranges, refs, en, pipelined = self.captured
        else:
            ranges = self.frozen if self.frozen is not None else synthetic_ranges(D, G, self.state)
            refs = [case.offset + sum(ranges[:d]) for d in range(D)]
            en = [not (self.state == "drop" and d == D - 1 and D > 1) for d in range(D)]
            if "enter" in step.mode:
                self.frozen = ranges
        arrs = plan.arrs(plan.hosts, flags)
        if step.mode != "replay":
            pipelined = expect_pipelined(path, arrs, ranges, D)
        if step.mode == "capture":
            self.captured = (flags, ranges, refs, en, pipelined)
            return None
        up, down = self.emu.call(arrs, plan.kernel, G, case.offset, ranges, refs, en,
                                 REPEATS if path == "repeat" else 1, path, pipelined)
        if "leave" in step.mode:
            self.frozen = None
        return {"ranges": list(ranges), "references": refs, "h2d_bytes": up, "d2h_bytes": down,
                "pipelined": pipelined, "enabled": en}

    def end(self) -> None:
        pass


class CruncherBackend:
    """The real runtime: one ClNumberCruncher over ``devices`` built from
    probe_source(ctype); ``kinds`` names each device "gpu" or "cpu"."""

    _ids = itertools.count(1000)

    def __init__(self, cruncher, kinds: Sequence[str]):
        self.cr = cruncher
        self.kinds = list(kinds)
        self.D = len(kinds)
        self.graph = None

    def alloc(self, n, dt):
        import cekirdekler_amd as ck

        a = ck.ClArray(int(n), np.dtype(dt))
        self._arrays.append(a)
        return a.array

    def begin(self, plan: Plan) -> None:
        self.plan = plan
        self.cid = next(self._ids)
        self.enabled = [True] * self.D
        cr = self.cr
        cr.repeat_count = 1
        cr.enqueue_mode_async_enable = False
        for d in range(self.D):
            cr.enable_device(d)
            cr.set_time_scale(d, 1.0)
        for a, e, g in zip(self._arrays, plan.epw, plan.epg):
            a.elements_per_work_item = e
            a.elements_per_group = g

    def new_case(self) -> None:
        self._arrays = []

    def _apply(self, flags: Sequence[Flags]) -> None:
        """Through ClArray's own setters: the hints off first (they refuse
        the flags they exclude), then the flags, then the hints."""
        for a, f in zip(self._arrays, flags):
            a.read_only = a.write_only = False
            a.read, a.partial_read, a.write, a.write_all = f.read, f.partial, f.write, f.write_all
            if f.ro:
                a.read_only = True
            if f.wo:
                a.write_only = True
            a.zero_copy, a.gather_resident = f.zc, f.gather
            got = (a.read, a.partial_read, a.write, a.write_all, a.read_only, a.write_only)
            if got != (f.read, f.partial, f.write, f.write_all, f.ro, f.wo):
                raise Mismatch(f"ClArray's setters gave {got} for {f}")

    def effective(self, flags: Sequence[Flags]) -> List[Flags]:
        """Zero-copy as the native layer takes it (only mapped host memory)."""
        self._apply(flags)
        return [dataclasses.replace(f, zc=bool(a._spec().zc)) for a, f in zip(self._arrays, flags)]

    def partition(self, what: str) -> None:
        last = self.D - 1
        if what in ("prime", "primed"):
            # A CPU device has no replica: its kernel writes the host arrays
            # while a GPU of the same call uploads them whole, so what such an
            # upload leaves outside the GPU's own slice is not defined.  The
            # priming call must define every element of every replica: with
            # GPUs in the set it runs on them alone.
            if "gpu" in self.kinds:
                for d, kind in enumerate(self.kinds):
                    if kind == "cpu":
                        self.cr.set_time_scale(d, 1.0)
                        (self.cr.disable_device if what == "prime" else self.cr.enable_device)(d)
                        self.enabled[d] = what == "primed"
        elif what == "drop":
            self.cr.disable_device(last)
            self.enabled[last] = False
        elif what == "rejoin":
            # the rejoining call splits equally; its scaled time skews the next
            self.cr.enable_device(last)
            self.enabled[last] = True
            self.cr.set_time_scale(0, 64.0)

    def run(self, plan: Plan, flags, step: Step, path: str) -> Optional[dict]:
        import cekirdekler_amd as ck

        cr, case = self.cr, plan.case
        if step.mode == "replay":
            self.graph.replay(1)
            self.graph.destroy()
            self.graph = None
            return dict(self.captured)
        self._apply(flags)
        group = ck.ClParameterGroup(self._arrays)
        cr.repeat_count = REPEATS if path == "repeat" else 1
        if "enter" in step.mode:
            cr.enqueue_mode_async_enable = path == "async"
            cr.enqueue_mode = True
        kw = dict(global_offset=case.offset, pipeline=path in ("event", "driver"),
                  pipeline_type=ck.PIPELINE_EVENT if path != "driver" else ck.PIPELINE_DRIVER,
                  pipeline_blobs=BLOBS)
        if step.mode == "capture":
            with cr.capture() as g:
                cr.compute(group, self.cid, plan.kernel_name, plan.G, L, **kw)
            self.graph = g
        else:
            cr.compute(group, self.cid, plan.kernel_name, plan.G, L, **kw)
        rec = cr.last_record()
        rec["enabled"] = list(self.enabled)
        if "leave" in step.mode:
            cr.enqueue_mode = False
            cr.enqueue_mode_async_enable = False
        if step.mode == "capture":
            self.captured = rec
            return None
        return rec

    def end(self) -> None:
        cr = self.cr
        if self.graph is not None:
            self.graph.destroy()
            self.graph = None
        if cr.enqueue_mode:
            cr.enqueue_mode = False
        cr.enqueue_mode_async_enable = False
        cr.repeat_count = 1
        for d in range(self.D):
            cr.enable_device(d)
            cr.set_time_scale(d, 1.0)
        cr.sync()
        for a in self._arrays:
            a.dispose()
        self._arrays = []


# ------------------------------------------------------------------ the harness


class Mismatch(AssertionError):
    pass


def run_case(case: Case, backend, model_kinds: Sequence[str], dtype, require_partition_change: bool = True,
             check_bytes: bool = True) -> dict:
    """Runs the case's sequence on ``backend`` and, call by call, on an honest
    Emulator over ``model_kinds`` fed with the ranges the backend reported.
    After every checked call the host arrays (every element: src, dst, the
    observations, par), both byte counts and the path taken must agree.
    Raises Mismatch with the first difference.  Returns what it saw."""
    D = len(model_kinds)
    backend.new_case()
    plan = Plan(case, D, dtype, backend.alloc)
    # A pipelined call uploads a partial_read array blob by blob while earlier
    # blobs' kernels run: an element of it outside the blob's own slice, but
    # inside the device's, is fresh or stale by timing.  Two models bound it:
    # one uploads the device's whole slice before any kernel, the other only
    # the running blob's; every element must equal one of the two (they differ
    # only in observations of such elements, and those never reach a replica).
    model, lazy = Emulator(model_kinds), Emulator(model_kinds, lazy_blobs=True)
    mhosts = [np.zeros(n, dt) for n, dt in zip(plan.lengths, plan.dtypes)]
    lhosts = [np.zeros(n, dt) for n, dt in zip(plan.lengths, plan.dtypes)]
    backend.begin(plan)
    seen_ranges, records = [], []
    names = ["out"] if case.kernel == "ids" else ["src", "dst", "grp" if case.epg else "seen", "par"]
    captured = None
    try:
        for n, step in enumerate(steps_of(case, D)):
            if step.partition:
                backend.partition(step.partition)
            if step.rewrite:
                plan.rewrite(plan.hosts, n, n)
                plan.rewrite(mhosts, n, n)
                plan.rewrite(lhosts, n, n)
            flags = plan.case_flags
            if step.flags == "prime":
                flags = [f.primed() for f in flags]
            elif step.flags == "late":
                flags = [flags_of("src", case.late[0]), flags_of("dst", case.late[1]), flags[2], flags[3]]
            elif step.flags == "resident" and case.kernel != "ids":
                flags = [flags[0], flags[1].resident(), flags[2], flags[3]]
            flags = backend.effective(flags)
            path = case.path if step.flags != "prime" else "plain"
            rec = backend.run(plan, flags, step, path)
            if step.mode == "capture":
                captured = flags
                continue
            if step.mode == "replay":
                flags = captured
            arrs = plan.arrs(mhosts, flags)
            want_pipe = expect_pipelined(path, arrs, rec["ranges"], D)
            where = f"{case.name} call {n} ranges {rec['ranges']} refs {rec['references']}"
            if bool(rec["pipelined"]) != want_pipe:
                raise Mismatch(f"{where}: pipelined {rec['pipelined']}, the model expects {want_pipe}")
            up, down = model.call(arrs, plan.kernel, plan.G, case.offset, rec["ranges"], rec["references"],
                                  rec["enabled"], REPEATS if path == "repeat" else 1, path, want_pipe)
            lazy.call(plan.arrs(lhosts, flags), plan.kernel, plan.G, case.offset, rec["ranges"], rec["references"],
                      rec["enabled"], REPEATS if path == "repeat" else 1, path, want_pipe)
            if sum(rec["ranges"]) != plan.G or rec["references"][0] != case.offset:
                raise Mismatch(f"{where}: the ranges do not cover [offset, offset + G)")
            if check_bytes and (rec["h2d_bytes"], rec["d2h_bytes"]) != (up, down):
                raise Mismatch(f"{where}: h2d/d2h bytes {rec['h2d_bytes']}/{rec['d2h_bytes']}, "
                               f"the model expects {up}/{down}")
            if "p2p_bytes" in rec:
                # no read fan-out in these cases: device-to-device bytes are the
                # gather's alone (all of them between GPUs; with a CPU device
                # the gather also moves slices through host memory)
                g = rec["gather_bytes"]
                between_gpus = rec["p2p_bytes"] == g or ("cpu" in model_kinds and rec["p2p_bytes"] < g)
                if rec["staged_bytes"] != 0 or not between_gpus:
                    raise Mismatch(f"{where}: staged {rec['staged_bytes']}, device-to-device {rec['p2p_bytes']}, "
                                   f"gather {g} bytes")
            seen_ranges.append(tuple(rec["ranges"]))
            records.append(rec)
            if not step.check:
                continue
            for name, got, want, want2 in zip(names, plan.hosts, mhosts, lhosts):
                if not np.array_equal(got, want):
                    bad = np.flatnonzero((got != want) & (got != want2))
                    if not len(bad):
                        continue
                    raise Mismatch(f"{where}: {name} differs at {len(bad)} of {len(got)} elements, first at "
                                   f"{bad[0]}: got {got[bad[0]]}, the model expects {want[bad[0]]}")
        if require_partition_change and D > 1 and len(set(seen_ranges)) < 2:
            raise Mismatch(f"{case.name}: the partition never changed ({seen_ranges[0]}): no stale-slice "
                           f"check in this sequence means anything")
    finally:
        backend.end()
    return {"ranges": seen_ranges, "records": records, "hosts": mhosts, "plan": plan, "kinds": list(model_kinds)}


def check_ids(result: dict, case: Case, D: int) -> None:
    """The work-item functions under partitioning, from the ids record of the
    last call: see docs/API.md, "Work-item functions"."""
    plan = result["plan"]
    rec = result["records"][-1]
    G, off = plan.G, case.offset
    out = result["hosts"][0][:IDS_CAP * IDS_EPW].reshape(IDS_CAP, IDS_EPW)
    rows = out[off:off + G]
    gid, lid, grp, lsz, gsz, ngr, goff, ggrp, lgrp, lngr = rows.T
    assert np.array_equal(gid, np.arange(off, off + G)), "every work item of [offset, offset + G) exactly once"
    assert np.array_equal(grp * L + lid + goff, gid)
    assert np.all(lsz == L) and np.all(gsz == G) and np.all(ngr == G // L)
    assert np.array_equal(ggrp, gid // L)
    assert np.array_equal(lgrp, grp)
    counts = set()
    for d, kind in enumerate(result["kinds"]):
        plan_d = launch_plan(case.path, rec["references"][d], rec["ranges"][d], bool(rec["pipelined"]))
        counts |= {n // L if kind == "gpu" else G // L for _, n in plan_d}
    assert set(lngr.tolist()) == counts, (sorted(set(lngr.tolist())), sorted(counts))
    want = set()
    for d in range(D):
        want |= {o for o, _ in launch_plan(case.path, rec["references"][d], rec["ranges"][d], bool(rec["pipelined"]))}
    assert set(goff.tolist()) == want, (sorted(set(goff.tolist())), sorted(want))


def check_repeat_kernel_shape(cruncher) -> None:
    """The repeat kernel (repeat_kernel_name) runs after each repetition as one
    work-group: offset 0, global size L, whatever the call's range and offset
    (Cores::launch_kernels_body).  ``idsr`` records it in the last L rows of
    the ids array, which no work item of the call owns; device 0 brings the
    whole array back (write + write_all, array index 0)."""
    import cekirdekler_amd as ck

    G, offset = global_range(1), 2 * L
    out = ck.ClArray(IDS_CAP * IDS_EPW, np.int64)
    out.array[:] = -1
    out.elements_per_work_item = IDS_EPW
    out.write_all = True
    cruncher.repeat_count, cruncher.repeat_kernel_name = 2, "idsr"
    try:
        cruncher.compute([out], next(CruncherBackend._ids), "ids", G, L, global_offset=offset)
        own = cruncher.last_record()["ranges"][0]  # device 0's replica holds device 0's work items
    finally:
        cruncher.repeat_count, cruncher.repeat_kernel_name = 1, ""
    rows = out.array.reshape(IDS_CAP, IDS_EPW)
    want = np.zeros((L, IDS_EPW), np.int64)
    want[:, 0] = want[:, 1] = np.arange(L)   # global id == local id: offset 0
    want[:, 3] = want[:, 4] = L              # local size, global size
    want[:, 5] = want[:, 9] = 1              # one group, globally and in the launch
    assert np.array_equal(rows[IDS_CAP - L:], want), rows[IDS_CAP - L:][:2]
    assert own > 0 and np.array_equal(rows[offset:offset + own, 0], np.arange(offset, offset + own))
    assert np.all(rows[offset + G:IDS_CAP - L] == -1)
    out.dispose()
