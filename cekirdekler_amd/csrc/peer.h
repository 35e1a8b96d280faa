// Device→device traffic of one process: the peer topology, the per-call
// copy accounting, the xGMI fan-out of full `read` arrays and the
// keep-resident gather.  PeerTraffic owns their state and events; the
// scheduler passes the decisions that are its own (PeerView).
#pragma once
#include "balancer.h"
#include "events.h"
#include "worker.h"
#include "sched_log.h"

namespace cek {

struct ComputeCall;

// What the copies need to know of the scheduler for one call.
struct PeerView {
  const std::vector<bool>& enabled;  // local devices taking part in splits
  int global_base;                   // global index of local device 0
  bool enqueue_mode;                 // no host sync after the copies
};

// per-call device→device accounting
struct D2DCount {
  uint64_t bytes = 0, xgmi = 0, local = 0, staged = 0;
  bool pcie_fallback = false;
  const char* path() const {
    return pcie_fallback ? "pcie" : staged ? "staged" : xgmi ? "xgmi" : local ? "local" : "none";
  }
};

class PeerTraffic {
 public:
  PeerTraffic(const Workers& workers, SchedLog& log) : workers_(workers), log_(log) {}
  // Once the workers exist.  Distinct GPUs of this device set: enable peer
  // access among them (xGMI) so the read fan-out, the keep-resident gather
  // and copy_between move bytes GPU↔GPU directly.  A pair that cannot peer is
  // recorded: the read fan-out then falls back to one PCIe upload per device,
  // and gather copies between that pair are counted as staged.
  void bind();

  // ---- topology ----
  const std::vector<int>& ordinals() const { return peer_ordinals_; }
  const std::vector<std::vector<int>>& matrix() const { return peer_matrix_; }
  const std::string& path() const { return p2p_path_; }
  bool can_peer(int w1, int w2) const;  // local workers: same GPU, or peer access on

  // ---- accounting ----
  D2DCount d2d;  // of the running call; the scheduler resets it (d2d = {})

  // ---- xGMI fan-out of full `read` arrays ----
  // Stages the call's eligible arrays (at least min_bytes, never written) when
  // `allowed` and two or more local GPUs compute; adds the uploaded bytes to
  // h2d per worker and returns the peer-copied bytes.
  uint64_t stage_reads(const ComputeCall& c, const std::vector<long long>& ranges, std::vector<uint64_t>& h2d,
                       const PeerView& v, bool allowed, uint64_t min_bytes);
  bool staged(int w) const { return w < static_cast<int>(staged_dev_.size()) && staged_dev_[w]; }
  bool staged_array(size_t i) const { return i < staged_arr_.size() && staged_arr_[i]; }
  // recorded once every participant pulled: kernels may modify the staged arrays
  hipEvent_t ready(int w) const { return peer_ready_[w].peek(); }

  // ---- keep-resident gather (ArraySpec::gather) ----
  // kernels-done event per worker, copies-done event per GPU worker; later
  // work waits on every copies-done event while gather_pending
  bool gather_pending = false;
  bool call_gathers = false;  // the running call gathers in-process
  // wk's kernels of a gathering call are enqueued on s
  void kernels_done(Worker& wk, hipStream_t s) {
    if (call_gathers && wk.gpu()) CEK_HIP(hipEventRecord(kdone_[wk.index()].get(wk.dev()), s));
  }
  // Work about to run on stream s of wk must see the last gather's copies,
  // and must not overwrite a slice the copies are still reading.
  void wait_gather(Worker& wk, hipStream_t s);
  uint64_t issue_gather(const ComputeCall& c, const BalancerState& st, const std::vector<int>& arrays,
                        const PeerView& v,
                        const std::vector<std::vector<std::pair<long long, long long>>>* owned = nullptr);
  void share_slices(const BalancerState& st, const ArraySpec& a, long long local_range, const PeerView& v);
  // device→device (peer/xGMI) copy, or between a GPU and the CPU device's host memory
  void copy_between(int src_dev, const ArraySpec& src, int dst_dev, const ArraySpec& dst, uint64_t bytes,
                    bool enqueue_mode);

 private:
  void count_d2d(int ws, int wd, uint64_t bytes);
  uint64_t d2d_copy(int ws, int wd, char* dst, const char* src, uint64_t bytes, hipStream_t s, int stream_worker);

  const Workers& workers_;
  SchedLog& log_;
  std::vector<int> peer_ordinals_;
  std::vector<std::vector<int>> peer_matrix_;
  std::string p2p_path_ = "none";
  std::vector<int> ord_index_;  // local worker -> index into peer_ordinals_ (-1: CPU device)
  // read fan-out: per local worker, the events its peers' streams wait on
  struct PeerEvents {
    Event up;      // this GPU's chunk uploaded
    Event pulled;  // every other chunk pulled into this GPU
  };
  std::vector<PeerEvents> peer_ev_;
  std::vector<Event> peer_ready_;
  std::vector<char> staged_arr_;  // by array index, for the current call
  std::vector<char> staged_dev_;  // by local worker, for the current call
  // one slot per worker from bind() on: the devices of a gathering call take
  // their kernels-done events from their own threads at the same time
  std::vector<Event> kdone_, pushed_;
};

}  // namespace cek
