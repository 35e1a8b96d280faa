// Schedule recording (pipeline dependency checks): every
// transfer / kernel / event edge the pipelines issue, and every peer copy, is
// appended as (device, op, logical stream, first work item, work items,
// event) by the call that issues it.  The logical stream is the id of the
// Lane it ran on (lanes.h: main_lane_id, compute_lane_id, pipe_lane_id).
#pragma once
#include <mutex>
#include <string>
#include <vector>

namespace cek {

struct SchedOp {
  int device;
  std::string op;  // h2d | kernel | d2h | rec | wait | p2p | gather
  int stream;
  long long begin, count;
  int event;
};

class SchedLog {
 public:
  explicit SchedLog(const bool& on) : on_(on) {}  // the scheduler's record_schedule switch
  void add(int gidx, const char* op, int stream, long long begin, long long count, int event = -1) {
    if (!on_) return;
    std::lock_guard<std::mutex> g(mu_);
    ops_.push_back({gidx, op, stream, begin, count, event});
  }
  std::vector<SchedOp> ops() {
    std::lock_guard<std::mutex> g(mu_);
    return ops_;
  }
  void clear() {
    std::lock_guard<std::mutex> g(mu_);
    ops_.clear();
  }

 private:
  const bool& on_;
  std::mutex mu_;
  std::vector<SchedOp> ops_;
};

}  // namespace cek
