// Compute graphs: hipGraph capture of a sequence of computes and its replay.
//
// begin() puts every GPU's main stream into (relaxed) stream capture; the
// computes that follow are recorded, not run: enqueue-mode semantics (split
// frozen, no host syncs), main stream only, no markers, device spans,
// peer-read staging or nested repeat graphs.  end() instantiates one graph per
// GPU and returns its id; launch(id, n) replays it n times back to back on
// each GPU's main stream — one hipGraphLaunch per GPU per replay instead of
// one host call per kernel and copy.  Host transfers inside the graph read /
// write the host arrays at replay time (pinned or registered memory only).
// Buffers must exist before capture: run the computes once first.
//
// ComputeGraphs owns the graphs and the buffer logs that tell whether one is
// still valid; the modes the scheduler overrides for a capture are kept here.
#pragma once
#include <map>

#include "events.h"
#include "worker.h"

namespace cek {

// the scheduler's modes that a capture overrides
struct CaptureSaved {
  bool device_spans, peer_reads, async_enqueue, fine_grained, enqueue_mode, record_timeline;
  int graph_min_launches;
  bool kernel_times;
};

class ComputeGraphs {
 public:
  explicit ComputeGraphs(const Workers& workers) : workers_(workers) {}
  ~ComputeGraphs();  // destroys every graph exec with its device current

  // Starts the capture on every worker; on failure the captures already
  // begun are ended and discarded, and the error is thrown.
  void begin(const CaptureSaved& saved);
  const CaptureSaved& saved() const { return saved_; }
  // Ends the capture and instantiates the graphs: their id, or 0 with `err`
  // set (nothing is kept then).
  int end(std::string& err);
  // Ends the capture on the first n workers and throws the graphs away.
  void discard_capture(size_t n);
  void launch(int id, int times, bool sync);
  void destroy(int id);

 private:
  using BufLog = std::vector<std::pair<uint64_t, void*>>;
  void destroy_execs(std::vector<hipGraphExec_t>& execs);

  const Workers& workers_;
  CaptureSaved saved_{};
  std::map<int, std::vector<hipGraphExec_t>> graphs_;  // id -> one exec per local worker (null: CPU)
  // buffers each worker handed out while capturing: (uid, pointer) — a graph
  // replays those pointers, so launch() refuses to run once any of them was
  // released or reallocated
  std::vector<BufLog> cap_logs_;
  std::map<int, std::vector<BufLog>> graph_bufs_;
  int next_id_ = 1;
};

}  // namespace cek
