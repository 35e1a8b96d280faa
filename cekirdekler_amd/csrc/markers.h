// Markers for fine-grained queue control (ClCommandQueue.cs:103-112): a
// compute's completion is a (lane slot, value) pair that the host polls.
#pragma once
#include <deque>

#include "lanes.h"

namespace cek {

class Markers {
 public:
  // `lanes` outlives the markers (the worker declares it first).
  Markers(const DeviceInfo& dev, const LaneTable& lanes);
  ~Markers();
  Markers(const Markers&) = delete;
  Markers& operator=(const Markers&) = delete;

  // release: the marker also makes earlier writes to HOST memory visible
  // (a system-scope release; set when the compute downloaded results)
  void add(hipStream_t s, bool release);
  // A compute that takes its completion from the NEXT marker of its stream:
  // last() becomes (slot, the value that marker will carry) and no HIP call
  // is made; flush() records that marker on every stream with such computes
  void defer(hipStream_t s, bool release);
  void flush();
  bool has_deferred() const { return deferred_slots_ != 0; }
  long long reached();
  // (slot, value) of the newest marker; a marker is reached once
  // word(slot) >= value.  CPU device: slot -1 (always reached).
  std::pair<int, uint64_t> last() const { return {last_slot_, last_value_}; }
  uint64_t word(int slot);
  long long issued() const { return issued_; }

 private:
  static constexpr int kSlots = 32;  // the lanes, and kNoLane for any other stream
  // Event markers (the default): per stream slot, the recorded events not
  // yet seen complete (in issue order: a stream completes them in order),
  // spare events, and how many have completed.  A marker is a barrier packet
  // with a completion signal; hipStreamWriteValue64 runs as a blit kernel
  // (__amd_rocclr_streamOpsWrite) — a kernel dispatch per marker, ~10× the
  // host cost under 8 submitting threads (profiles/r5/README.md).
  struct Ring {
    std::deque<std::pair<Event, bool>> pending;  // (event, system-scope release)
    std::deque<Event> spare, spare_fenced;
    uint64_t done = 0;
  };

  const DeviceInfo& dev_;
  const LaneTable& lanes_;
  bool write_value_ = false;  // CEK_MARKERS=writevalue: the old path
  // one 64-bit word per stream slot in pinned host memory
  uint64_t* words_ = nullptr;
  uint64_t* words_dev_ = nullptr;  // device address of words_ (looked up once)
  uint64_t issued_per_slot_[kSlots] = {};
  std::mutex mu_;  // guards rings_
  Ring rings_[kSlots];
  uint32_t deferred_slots_ = 0;    // bit per stream slot with deferred markers
  uint32_t deferred_release_ = 0;  // ... whose marker must also release host writes
  long long issued_ = 0;
  int last_slot_ = -1;
  uint64_t last_value_ = 0;
};

}  // namespace cek
