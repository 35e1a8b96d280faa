// Device-time spans: what the devices' own clocks say about a compute.
//
// For the balancer: each GPU device's work in a compute
// is bracketed by a pair of timing hipEvents on the stream it starts and ends
// on; the balancer gets the device time between them (hipEventElapsedTime)
// instead of host wall clock.  Sync mode reuses pair 0; enqueue mode takes a
// fresh pair per compute and, when the mode is left, credits each device with
// the union of its spans (so devices of one process re-balance by their own
// device time, not the shared wall clock).
//
// For the timeline: with Cores::record_timeline on, the kernels
// of every compute are bracketed by timing events of their own (host clock on
// the CPU device) until timeline() collects them.
//
// Spans owns every event of both and frees them; the scheduler tells it the
// modes it needs with each call (SpanModes).
#pragma once
#include <mutex>

#include "events.h"
#include "worker.h"

namespace cek {

// The scheduler's modes that decide whether and how spans are taken.
struct SpanModes {
  bool device_spans, single_device_spans;
  bool all_gpu;  // every local device is a GPU
  int global_devices;
  bool enqueue_mode, async_enqueue;
};

struct TimelineSpan {
  int device, compute_id;
  double begin_ms, end_ms;
  double abs_begin_ms, abs_end_ms;  // host clock (event_host_ms): comparable across devices
};

class Spans {
 public:
  explicit Spans(const Workers& workers) : workers_(workers) {}
  void bind() {  // once the workers exist: one slot per local device
    dev_.resize(workers_.size());
    pending_end_.resize(workers_.size());
  }

  bool on(const SpanModes& m) const;
  bool one_per_batch(const SpanModes& m) const;
  void begin(Worker& wk, hipStream_t s, const SpanModes& m);
  void end(Worker& wk, hipStream_t s, const SpanModes& m);
  // the idle gap of a phase barrier inside the span: taken out of ms()
  void gap_begin(Worker& wk, hipStream_t s);
  void gap_end(Worker& wk, hipStream_t s);
  double ms(int w, const SpanModes& m);  // sync mode: the last span (stream drained)
  double enqueue_ms(int w);              // enqueue mode: union of the spans so far
  void close_batch();
  void forget() {  // a graph capture ended: its computes took no spans
    for (auto& d : dev_) d.used = 0;
  }
  // A span whose end follows a deferred download: recorded on `s` by
  // record_deferred_ends(), when the downloads are issued.
  void defer_end(Worker& wk, hipStream_t s) { pending_end_[wk.index()].push_back({s, dev_[wk.index()].used - 1}); }
  bool ends_deferred(int w) const { return !pending_end_[w].empty(); }
  void record_deferred_ends(int w);

  // ---- timeline ----
  struct Pending {
    int device, compute_id;
    Event begin, end;                     // GPU: timing events (device epoch: first span's begin)
    double host_begin = 0, host_end = 0;  // CPU device: host clock
  };
  Pending timeline_begin(Worker& wk, int compute_id, hipStream_t s);
  void timeline_end(Worker& wk, hipStream_t s, Pending&& sp);
  // waits for the recorded work and returns the spans, relative to the first
  // span of their device, then clears the list
  std::vector<TimelineSpan> timeline();

 private:
  struct Dev {
    std::vector<std::pair<Event, Event>> pool;
    int used = 0;
    Event gap_a, gap_b;  // phase-barrier idle gap
    bool gap = false;
    hipStream_t batch = nullptr;  // enqueue mode: stream of the open batch span
  };
  struct PendingEnd {
    hipStream_t s;
    int index;
  };
  const Workers& workers_;
  std::vector<Dev> dev_;
  std::vector<std::vector<PendingEnd>> pending_end_;  // per local device
  std::mutex tl_mu_;
  std::vector<Pending> pending_;
};

}  // namespace cek
