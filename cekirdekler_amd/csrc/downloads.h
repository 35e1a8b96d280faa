// Deferred downloads of async enqueue mode: a compute's downloads are issued
// after the NEXT compute's uploads (or when the batch ends).  A stream's
// copies go to an SDMA queue that other streams share and that runs in
// submission order: a download, which waits for its kernel, would hold back
// every later compute's upload behind it, and the computes would run one
// after the other instead of side by side (rocprofv3 trace,
// profiles/r5/README.md).
//
// The scheduler decides when a compute defers (Cores::defer_downloads) and
// when the queue is flushed; this part keeps the queue and the events that
// order a flushed download against the next compute.
#pragma once
#include "events.h"
#include "worker.h"

namespace cek {

struct ComputeCall;

class DeferredDownloads {
 public:
  explicit DeferredDownloads(const Workers& workers) : workers_(workers) {}
  void bind() {  // once the workers exist: one queue per local device
    pending_.resize(workers_.size());
    order_events_.resize(workers_.size());
  }

  void defer(const Worker& wk, hipStream_t s, const ArraySpec& a, uint64_t begin, uint64_t count) {
    pending_[wk.index()].push_back({s, a, begin, count});
  }
  bool pending(int w) const { return !pending_[w].empty(); }
  // A deferred download may not be overtaken by the next compute's uploads
  // when they share an in-order stream (the download would follow the upload)
  // or touch the same array (a stale host copy going up over the result, or
  // the next upload reading host memory the download has not filled yet).
  bool must_flush_before(const Worker& wk, hipStream_t s, const ComputeCall& c) const;
  // Issue wk's pending downloads (its device is current).  With `next` (the
  // stream the next compute runs on) and that compute `c`, `next` also waits
  // for every pending download on another stream whose array the compute
  // touches.
  void flush(Worker& wk, hipStream_t next, const ComputeCall* c);
  // the streams holding a pending download of array `uid` on device w
  std::vector<hipStream_t> streams_holding(int w, uint64_t uid) const;

 private:
  struct PendingD2H {
    hipStream_t s;
    ArraySpec a;
    uint64_t begin, count;
  };
  const Workers& workers_;
  std::vector<std::vector<PendingD2H>> pending_;    // per local device
  std::vector<std::vector<Event>> order_events_;    // per local device (flush ordering)
};

}  // namespace cek
