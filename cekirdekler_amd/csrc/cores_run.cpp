// The three execution shapes of one device's part of a compute(): 3-phase,
// event pipeline and driver pipeline, what they share (Cores::Ordering, the
// full reads, the kernel launches) and run_device, which picks one.
#include <algorithm>
#include <thread>
#include <tuple>

#include "cores.h"
#include "trace.h"

namespace cek {

// time the calling worker spent in the phase barrier of the current compute
static thread_local double t_phase_wait = 0;
static thread_local bool t_phase_arrived = false;

void Cores::launch_kernels(Worker& wk, hipStream_t s, const ComputeCall& c, long long ref,
                           long long range) {
  if (!record_timeline || no_compute) {
    launch_kernels_body(wk, s, c, ref, range);
    return;
  }
  Spans::Pending sp = spans_.timeline_begin(wk, c.compute_id, s);
  launch_kernels_body(wk, s, c, ref, range);
  spans_.timeline_end(wk, s, std::move(sp));
}

void Cores::launch_kernels_body(Worker& wk, hipStream_t s, const ComputeCall& c, long long ref,
                                long long range) {
  if (no_compute) return;
  const int reps = std::max(1, c.repeats);
  auto body = [&](hipStream_t st) {
    for (int r = 0; r < reps; ++r) {
      for (auto& k : c.kernels)
        wk.launch(st, k, c.arrays, ref, range, static_cast<int>(c.local_range), c.global_range);
      if (!c.repeat_kernel.empty())
        wk.launch(st, c.repeat_kernel, c.arrays, 0, c.local_range, static_cast<int>(c.local_range),
                  c.local_range);
    }
  };
  const int launches = reps * (static_cast<int>(c.kernels.size()) + (c.repeat_kernel.empty() ? 0 : 1));
  if (!wk.gpu() || graph_min_launches <= 0 || launches < graph_min_launches || range <= 0) {
    body(s);
    return;
  }
  // A launch-bound repeat loop is captured once into a hipGraph and replayed;
  // the key holds everything the captured launches bake in (kernels, ranges,
  // device buffer addresses).
  std::string key = std::to_string(reps) + "|" + c.repeat_kernel + "|" + std::to_string(ref) + "|" +
                    std::to_string(range) + "|" + std::to_string(c.local_range) + "|" +
                    std::to_string(c.global_range);
  for (auto& k : c.kernels) key += "|" + k;
  for (auto& a : c.arrays) key += "|" + std::to_string(reinterpret_cast<uintptr_t>(wk.buffer(a)));
  wk.launch_graph(s, key, body);
}

void Cores::full_reads(Worker& wk, hipStream_t s, const ComputeCall& c, uint64_t* h2d) {
  const bool dist = comm_ && dist_broadcast_reads;
  const int w = wk.index();
  const bool staged = peer_.staged(w);
  if (staged && s != wk.main_stream()) CEK_HIP(hipStreamWaitEvent(s, peer_.ready(w), 0));  // staged on the main stream
  for (size_t i = 0; i < c.arrays.size(); ++i) {
    const auto& a = c.arrays[i];
    if (a.zc || a.partial || !a.read) continue;
    if (staged && peer_.staged_array(i)) continue;  // already staged by the xGMI fan-out
    if (comm_ && dist_split_reads) {
      // Split upload + all-gather (every rank's host copy holds the same
      // data): rank g copies chunk g of the array over its own PCIe link,
      // then one RCCL ring all-gather over xGMI completes every replica.
      // Each link carries 1/N of the array instead of all of it.
      const int W = global_devices_;
      std::vector<uint64_t> offs(W), sizes(W);
      for (int g = 0; g < W; ++g) std::tie(offs[g], sizes[g]) = byte_chunk(a.bytes, W, a.elem_size, g);
      wk.h2d(s, a, offs[global_base_] / a.elem_size, sizes[global_base_] / a.elem_size);
      *h2d += sizes[global_base_];
      comm_->allgatherv(wk.buffer(a), offs, sizes, s);
    } else if (dist) {
      if (global_base_ == 0) {
        wk.h2d(s, a, 0, a.bytes / a.elem_size);
        *h2d += a.bytes;
      }
      comm_->broadcast(wk.buffer(a), a.bytes, 0, s);
    } else {
      wk.h2d(s, a, 0, a.bytes / a.elem_size);
      *h2d += a.bytes;
    }
  }
}

// The call issues RCCL collectives (broadcast / split-read all-gather /
// written-slice all-gather) that every rank must join, whatever its range.
bool Cores::collective(const ComputeCall& c) const {
  if (!comm_) return false;
  if (dist_gather_writes || dist_broadcast_reads || dist_split_reads) return true;
  return std::any_of(c.arrays.begin(), c.arrays.end(), [](const ArraySpec& a) { return a.gather && !a.zc; });
}

// Kernels that may store into zero-copy (host) memory: close the device's
// work with a system-scope release (the span events carry none).
static bool writes_host_memory(const ComputeCall& c) {
  return std::any_of(c.arrays.begin(), c.arrays.end(), [](const ArraySpec& a) { return a.zc && !a.ro; });
}

// A marker after this compute must release host-memory writes (system
// scope): kernels stored into zero-copy memory, or results were downloaded
// (a blit-kernel D2H into hipHostMalloc pages is a kernel store to host
// memory).  Device-resident computes get a fence-less marker.
static bool marker_needs_release(const ComputeCall& c) {
  return std::any_of(c.arrays.begin(), c.arrays.end(),
                     [](const ArraySpec& a) { return (a.zc && !a.ro) || (!a.zc && (a.write || a.write_all)); });
}

// The scheduler's side of the deferred downloads (downloads.h): whether this
// device's computes defer theirs now.
bool Cores::defer_downloads(const Worker& wk) const {
  // not with markers (a task's marker must follow its own download, and a
  // deferred one would wait for the next task), collectives, phase barriers
  // or a graph capture
  return deferred_downloads && wk.gpu() && enqueue_mode_ && async_enqueue && !fine_grained && !capturing_ &&
         !phase_ && !comm_;
}

void Cores::flush_downloads(Worker& wk, hipStream_t next, const ComputeCall* c) {
  const int w = wk.index();
  if (!downloads_.pending(w) && !spans_.ends_deferred(w)) return;
  wk.set_device();
  downloads_.flush(wk, next, c);
  spans_.record_deferred_ends(w);
}

// One device's part of one compute(): the transfers, kernel batches and event
// edges of the run_* functions below go through this object, which makes the
// HIP call (on a GPU) and writes the schedule-log line from the same
// arguments, so the log the schedule checker reads cannot drift from what was
// issued.  Event slots are taken in call order.  The pipelines log; the
// 3-phase path never did and stays unlogged.  A stack value per call: no
// allocation, the slice rules are inlined lambdas
//   rule(array, begin, count) -> false: this array does not move here
// Bytes of elements [begin, begin + count) that lie inside the array: what
// Worker::h2d / d2h copy of a slice that runs past its end (a global offset
// with an array sized for the global range alone)
static uint64_t bytes_inside(const ArraySpec& a, uint64_t begin, uint64_t count) {
  const uint64_t off = begin * a.elem_size;
  if (off >= a.bytes) return 0;
  return std::min<uint64_t>(count * a.elem_size, a.bytes - off);
}

struct Cores::Ordering {
  Cores& cs;
  Worker& wk;
  const int gidx;
  const ComputeCall& c;
  uint64_t& up;    // bytes host → device
  uint64_t& down;  // bytes device → host
  const bool logged;
  int slot = 0;

  void log(const char* op, Lane l, long long off, long long len, int event = -1) {
    if (logged) cs.sched_.add(gidx, op, l.id, off, len, event);
  }
  // an event on `from`, for work items [off, off + len): returns its slot
  int mark(Lane from, long long off, long long len, bool issue = true) {
    const int e = slot++;
    if (issue && wk.gpu()) CEK_HIP(hipEventRecord(wk.event(e), from.s));
    log("rec", from, off, len, e);
    return e;
  }
  void wait(Lane to, int e, long long off, long long len, bool issue = true) {
    if (issue && wk.gpu()) CEK_HIP(hipStreamWaitEvent(to.s, wk.event(e), 0));
    log("wait", to, off, len, e);
  }
  // `to` goes on after what `from` holds so far.  One in-order stream under
  // both names needs no event: the edge is logged and its slot consumed only.
  void link(Lane from, Lane to, long long off, long long len) {
    const bool issue = from.s != to.s;
    wait(to, mark(from, off, len, issue), off, len, issue);
  }
  void full_reads(Lane l) {
    cs.full_reads(wk, l.s, c, &up);
    log("h2d", l, -1, -1);
  }
  template <class Rule>
  void h2d(Lane l, long long off, long long len, Rule rule) {
    for (auto& a : c.arrays) {
      uint64_t b, n;
      if (a.zc || !a.partial || !rule(a, b, n)) continue;
      wk.h2d(l.s, a, b, n);
      up += bytes_inside(a, b, n);
    }
    log("h2d", l, off, len);
  }
  void kernels(Lane l, long long off, long long len) {
    cs.launch_kernels(wk, l.s, c, off, len);
    log("kernel", l, off, len);
  }
  template <class Rule>
  void d2h(Lane l, long long off, long long len, Rule rule) {
    for (auto& a : c.arrays) {
      uint64_t b, n;
      if (a.zc || !a.write || a.write_all || !rule(a, b, n)) continue;
      wk.d2h(l.s, a, b, n);
      down += bytes_inside(a, b, n);
    }
    log("d2h", l, off, len);
  }
  // array i's owner (device i mod D) downloads the whole array
  bool owns(size_t i) const { return static_cast<int>(i % cs.global_devices_) == gidx; }
  void write_all_downloads(Lane l) {
    for (size_t i = 0; i < c.arrays.size(); ++i) {
      const auto& a = c.arrays[i];
      if (a.zc || !a.write || !a.write_all || !owns(i)) continue;
      wk.d2h(l.s, a, 0, a.bytes / a.elem_size);
      down += a.bytes;
    }
  }
  void close(Lane l, bool wait_for_it) {
    if (cs.zc_release && !cs.enqueue_mode_ && writes_host_memory(c)) wk.system_release(l.s);
    if (cs.fine_grained) {
      if (cs.defer_marker)
        wk.defer_marker(l.s, marker_needs_release(c));
      else
        wk.add_marker(l.s, marker_needs_release(c));
    }
    if (wait_for_it && wk.gpu()) wk.wait_stream(l.s, cs.sleep_waits || cs.sleep_this_call_);
  }
};

void Cores::run_3phase(Worker& wk, int gidx, const ComputeCall& c, long long ref, long long range,
                       uint64_t* h2d, uint64_t* d2h) {
  Ordering o{*this, wk, gidx, c, *h2d, *d2h, /*logged=*/false};
  Lane l = wk.main_lane();
  if (wk.gpu() && enqueue_mode_ && async_enqueue) l = wk.compute_lane(wk.next_compute_queue());
  hipStream_t s = l.s;
  const bool defer = defer_downloads(wk);
  if (!defer || downloads_.must_flush_before(wk, s, c))
    flush_downloads(wk, s, &c);  // this compute runs after every earlier download
  if (wk.gpu() && s != wk.main_stream()) peer_.wait_gather(wk, s);
  const SpanModes sm = span_modes();
  spans_.begin(wk, s, sm);
  // across ranks: written slices all-gathered by RCCL (every written array
  // with dist_gather_writes, else the arrays flagged gather)
  const bool gather = comm_ && (dist_gather_writes || std::any_of(c.arrays.begin(), c.arrays.end(),
                                                                  [](const ArraySpec& a) { return a.gather; }));
  auto gathered = [&](const ArraySpec& a) {
    return comm_ && !a.zc && !a.write_all && (a.gather || (dist_gather_writes && (a.write || a.wo)));
  };
  // phase 1: host → device (partial slice wins over full read; an array
  // with explicit blob slices, run without its pipeline, goes up whole)
  o.h2d(l, ref, range, [&](const ArraySpec& a, uint64_t& b, uint64_t& n) {
    if (!a.blob_begin.empty()) {
      b = 0;
      n = a.bytes / a.elem_size;
    } else {
      a.slice(ref, range, c.local_range, b, n);
    }
    return true;
  });
  o.full_reads(l);
  // the earlier computes' downloads go into the copy queues after this
  // compute's uploads
  if (defer) flush_downloads(wk);
  // phase 2: kernels
  o.kernels(l, ref, range);
  // in-process gather: this device's kernels are enqueued
  peer_.kernels_done(wk, s);
  // optional device-side all-gather of written slices (distributed keep-resident)
  if (gather) {
    auto& st = state_[c.compute_id];
    for (auto& a : c.arrays) {
      if (!gathered(a)) continue;
      std::vector<uint64_t> offs(global_devices_), sizes(global_devices_);
      for (int g = 0; g < global_devices_; ++g) {
        uint64_t b, n;
        a.slice(st.references[g], st.ranges[g], c.local_range, b, n);
        offs[g] = b * a.elem_size;
        sizes[g] = n * a.elem_size;
        if (offs[g] + sizes[g] > a.bytes) sizes[g] = offs[g] < a.bytes ? a.bytes - offs[g] : 0;
      }
      comm_->allgatherv(wk.buffer(a), offs, sizes, s);
    }
  }
  // Phase separation when an array is both read whole and written back:
  // no device may write its slice into host memory another device is still
  // reading (reference: all reads and computes finish before any write).
  if (phase_) {
    spans_.gap_begin(wk, s);
    if (wk.gpu()) wk.wait_stream(s, sleep_waits || sleep_this_call_);
    t_phase_arrived = true;
    const double w0 = now_ms();
    phase_->arrive_and_wait();
    t_phase_wait = now_ms() - w0;  // not this device's work: kept out of its time
    spans_.gap_end(wk, s);
  }
  // phase 3: device → host, in the arrays' order (deferred in async enqueue
  // mode, downloads.h)
  bool deferred_any = false;
  for (size_t i = 0; i < c.arrays.size(); ++i) {
    const auto& a = c.arrays[i];
    if (a.zc || !a.write) continue;
    deferred_any = defer;
    if (a.write_all && !o.owns(i)) continue;
    uint64_t b = 0, n = a.bytes / a.elem_size;  // an owner's whole array; a replica holding every rank's slice
    if (!a.write_all && !gathered(a)) a.slice(ref, range, c.local_range, b, n);
    if (defer)
      downloads_.defer(wk, s, a, b, n);
    else
      wk.d2h(s, a, b, n);
    *d2h += bytes_inside(a, b, n);
  }
  if (deferred_any && wk.gpu() && spans_.on(sm))
    spans_.defer_end(wk, s);  // the span closes after the deferred download too
  else
    spans_.end(wk, s, sm);
  o.close(l, !enqueue_mode_);
}

void Cores::run_event_pipeline(Worker& wk, int gidx, const ComputeCall& c, long long ref,
                               long long range, uint64_t* h2d, uint64_t* d2h) {
  Ordering o{*this, wk, gidx, c, *h2d, *d2h, /*logged=*/true};
  const long long B = std::max(1, c.blobs);
  const long long chunk = range / B;
  const int halves = (B % 2 == 0) ? 2 : 1;
  const long long per_half = B / halves;
  const Lane m = wk.main_lane();
  spans_.begin(wk, m.s, span_modes());
  o.full_reads(m);
  const int full = o.mark(m, 0, 0);
  for (int h = 0; h < halves; ++h) o.wait(wk.pipe_lane(h, 1), full, 0, 0);
  // Interleave the two half-pipelines' chunks so both read streams start
  // early; explicit blobs (c.blob_bounds) alternate between the halves.
  const bool explicit_blobs = !c.blob_bounds.empty();
  const long long nblob = explicit_blobs ? static_cast<long long>(c.blob_bounds.size()) - 1 : per_half * halves;
  const int used_halves = explicit_blobs ? (nblob >= 2 ? 2 : 1) : halves;
  // Optional (pipeline_reads_two_streams, off): the partial arrays of an
  // explicit blob alternate between the main stream and a second upload
  // stream, and each blob's kernels wait for both.  Alone, one stream of
  // 8 MiB copies pays ~11 µs per copy that two streams hide (5.04 vs
  // 4.72 ms for 256 MiB); inside the shell pipeline the extra stream shares
  // a hardware queue with kernel and download streams and the call slows
  // from 7.1 to 12.7 ms (profiles/round4_session4.md), so it stays off.
  const int nread = (explicit_blobs && pipeline_reads_on_main_stream && pipeline_reads_two_streams) ? 2 : 1;
  const Lane rs2 = nread == 2 ? wk.pipe_lane(0, 0) : Lane{};
  if (nread == 2) o.wait(rs2, full, 0, 0);
  for (long long q = 0; q < nblob; ++q) {
    const long long k = explicit_blobs ? q : q / halves;
    const int h = explicit_blobs ? static_cast<int>(q % 2) : static_cast<int>(q % halves);
    // reads_on_main_stream: every blob's upload follows the full reads on
    // the main stream (one in-order chain of copies).  Explicit blobs always
    // upload there: blob q's kernels may read panels uploaded by earlier
    // blobs of the OTHER half (shell s reads panels 0..s), which only one
    // in-order upload chain orders before them
    const bool reads_main = pipeline_reads_on_main_stream || explicit_blobs;
    const Lane rs = reads_main ? m : wk.pipe_lane(h, 0), ks = wk.pipe_lane(h, 1);
    // writes_on_compute_stream: a blob's D2H follows its kernel on the same
    // stream (in-stream order) instead of a write stream gated by an event
    const Lane ws = pipeline_writes_on_compute_stream ? ks : wk.pipe_lane(pipeline_writes_one_stream ? 0 : h, 2);
    const long long off = explicit_blobs ? ref + c.blob_bounds[q] : ref + h * (range / halves) + k * chunk;
    const long long len = explicit_blobs ? c.blob_bounds[q + 1] - c.blob_bounds[q] : chunk;
    auto blob_slice = [&](const ArraySpec& a, uint64_t& b, uint64_t& n) {
      if (explicit_blobs && a.blob_begin.size() == c.blob_bounds.size() - 1) {
        b = a.blob_begin[q];
        n = a.blob_count[q];
      } else {
        a.slice(off, len, c.local_range, b, n);
      }
      return true;
    };
    // with two upload streams the partial arrays alternate between them, and
    // every blob's kernels wait for both, also a blob that uploads nothing
    // on the second (its kernels may need an earlier blob's panel, and
    // consecutive blobs' kernels run on different streams)
    for (int j = 0; j < nread; ++j) {
      const Lane r = j ? rs2 : rs;
      int pi = 0;
      o.h2d(r, off, len, [&](const ArraySpec& a, uint64_t& b, uint64_t& n) {
        return pi++ % nread == j && blob_slice(a, b, n);
      });
      o.link(r, ks, off, len);
    }
    o.kernels(ks, off, len);
    o.link(ks, ws, off, len);
    o.d2h(ws, off, len, blob_slice);
  }
  // write-all owners download after every chunk's kernels
  for (int h = 0; h < used_halves; ++h) {
    o.link(wk.pipe_lane(h, 1), m, 0, 0);
    o.link(wk.pipe_lane(h, 2), m, 0, 0);
  }
  o.write_all_downloads(m);
  spans_.end(wk, m.s, span_modes());
  o.close(m, true);
}

void Cores::run_driver_pipeline(Worker& wk, int gidx, const ComputeCall& c, long long ref,
                                long long range, uint64_t* h2d, uint64_t* d2h) {
  Ordering o{*this, wk, gidx, c, *h2d, *d2h, /*logged=*/true};
  const long long B = std::max(1, c.blobs);
  const long long chunk = range / B;
  const Lane m = wk.main_lane();
  spans_.begin(wk, m.s, span_modes());
  o.full_reads(m);
  const int full = o.mark(m, 0, 0);  // each queue waits for it at its first blob
  const int nq = wk.queue_concurrency();
  bool used[16] = {};
  auto is_read = [](const ArraySpec& a) { return !a.zc && a.partial; };
  auto is_written = [](const ArraySpec& a) { return !a.zc && a.write && !a.write_all; };
  // reads_main: a blob's upload goes into the main stream's one in-order
  // chain of copies and its queue waits for it, so no upload waits behind
  // an earlier blob's kernel in a compute queue
  const bool reads_main = driver_reads_on_main_stream && wk.gpu();
  const bool link_reads = reads_main && std::any_of(c.arrays.begin(), c.arrays.end(), is_read);
  // the blobs' downloads go to one download stream (the event pipeline's
  // first write stream)
  const bool own_dl = driver_downloads_own_stream && wk.gpu() &&
                      std::any_of(c.arrays.begin(), c.arrays.end(), is_written);
  const Lane dl = driver_downloads_own_stream && wk.gpu() ? wk.pipe_lane(0, 2) : Lane{};
  for (long long k = 0; k < B; ++k) {
    const int qi = static_cast<int>(k % nq);
    const Lane q = wk.compute_lane(qi);
    if (!used[qi]) o.wait(q, full, 0, 0);
    used[qi] = true;
    const long long off = ref + k * chunk;
    auto items = [&](const ArraySpec& a, uint64_t& b, uint64_t& n) {
      a.slice(off, chunk, c.local_range, b, n);
      return true;
    };
    o.h2d(reads_main ? m : q, off, chunk, items);
    if (link_reads) o.link(m, q, off, chunk);
    o.kernels(q, off, chunk);
    if (own_dl) o.link(q, dl, off, chunk);
    o.d2h(own_dl ? dl : q, off, chunk, items);
  }
  if (own_dl) o.link(dl, m, 0, 0);  // the call ends after the last download
  for (int q = 0; q < 16; ++q)
    if (used[q]) o.link(wk.compute_lane(q), m, 0, 0);
  o.write_all_downloads(m);
  spans_.end(wk, m.s, span_modes());
  o.close(m, true);
}

void Cores::run_device(int w, const ComputeCall& c, long long ref, long long range, bool pipelined,
                       double* out_ms, uint64_t* h2d, uint64_t* d2h) {
  t_phase_arrived = false;
  try {
    run_device_body(w, c, ref, range, pipelined, out_ms, h2d, d2h);
  } catch (...) {
    // a failing device must not leave the others waiting in the phase barrier
    if (phase_ && !t_phase_arrived && range > 0) phase_->arrive_and_drop();
    throw;
  }
}

void Cores::run_device_body(int w, const ComputeCall& c, long long ref, long long range, bool pipelined,
                       double* out_ms, uint64_t* h2d, uint64_t* d2h) {
  Worker& wk = *workers_[w];
  const int gidx = global_base_ + w;
  TraceRange tr(trace_enabled() ? "cek.device" + std::to_string(gidx) + ".id" + std::to_string(c.compute_id)
                                : std::string());
  t_phase_wait = 0;
  if (range > 0 && inject_[w] > 0) {
    --inject_[w];
    throw Error("injected failure on device " + std::to_string(w));
  }
  double t0 = now_ms();
  if (!wk.gpu()) peer_.wait_gather(wk, nullptr);  // host memory: the copies into it are done
  const double offset = range > 0 ? time_offset_[w] : 0.0;
  if (offset > 0) {  // injected fixed cost per compute (tests): real host time
    const double until = now_ms() + offset;
    while (now_ms() < until) std::this_thread::yield();
  }
  if (range > 0) {
    wk.set_device();
    if (pipelined) flush_downloads(wk);  // the pipelines' copies follow every earlier download
    if (!pipelined)
      run_3phase(wk, gidx, c, ref, range, h2d, d2h);
    else if (c.pipeline_event)
      run_event_pipeline(wk, gidx, c, ref, range, h2d, d2h);
    else
      run_driver_pipeline(wk, gidx, c, ref, range, h2d, d2h);
  } else if (collective(c)) {
    // still take part in the collectives (a rank the split rounded down to
    // an empty range must join every RCCL call the others make).  On the
    // inline path the calling thread's device is the caller's, not this
    // worker's: its streams, events and communicator need the worker's
    wk.set_device();
    run_3phase(wk, gidx, c, ref, 0, h2d, d2h);
  }
  double el = now_ms() - t0 - t_phase_wait;
  // Device-time spans only when every local device is a GPU: a CPU device
  // has only the host clock, and a GPU's span leaves out its launch, sync
  // and staging overhead, so the two would not be comparable (the reference
  // times every device with one host stopwatch, Worker.cs:779-807).
  if (range > 0 && wk.gpu() && !enqueue_mode_ && all_gpu_) {
    const double dev = spans_.ms(w, span_modes());  // the stream was drained: device time of this compute
    if (dev > 0) el = dev + offset;
  }
  *out_ms = el * time_scale_[w];
}

}  // namespace cek
