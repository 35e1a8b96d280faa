// Device replicas of host arrays: one full-length device buffer per host
// array and device (Worker.cs:576-720), or for a zero-copy array the device
// view of its host memory; optional guard tails for the debug checks.
#pragma once
#include <unordered_map>

#include "device.h"

namespace cek {

// One kernel-parameter array of a compute() call (ClArray flags,
// ClArray.cs:1742-1888; token semantics Worker.cs:827-834, :1349-1356).
struct ArraySpec {
  uint64_t uid = 0;       // identity of the host array (buffer-cache key)
  void* host = nullptr;   // host pointer
  uint64_t bytes = 0;     // total bytes of the host array
  int elem_size = 4;
  bool read = true;       // H2D the whole array to every device
  bool partial = false;   // H2D only this device's slice (wins over read)
  bool write = true;      // D2H this device's slice
  bool write_all = false; // device (index mod D) D2H the whole array
  bool ro = false, wo = false;  // access hints
  bool zc = false;        // zero-copy: kernel reads/writes host memory
  // keep-resident gather: after the kernels, every device's written slice
  // is copied into every other device's replica (event-ordered device→device
  // copies over xGMI in one process, an RCCL all-gather across ranks), so an
  // iterative kernel reads everybody's results without a host round trip
  bool gather = false;
  int epw = 1;            // elements per work item
  int epg = 0;            // >0: elements per work-GROUP instead (per-group outputs)
  // explicit blob slices (event pipeline with ComputeCall::blob_bounds):
  // blob k moves elements [blob_begin[k], blob_begin[k] + blob_count[k])
  // instead of the slice proportional to its work items — e.g. blob k of a
  // square-shell GEMM needs row panel k of A and of B
  std::vector<uint64_t> blob_begin, blob_count;
  // Element slice [begin, begin+count) owned by work items [ref, ref+range).
  void slice(long long ref, long long range, long long local, uint64_t& begin, uint64_t& count) const {
    if (epg > 0) {
      begin = static_cast<uint64_t>(ref / local) * epg;
      count = static_cast<uint64_t>(range / local) * epg;
    } else {
      begin = static_cast<uint64_t>(ref) * epw;
      count = static_cast<uint64_t>(range) * epw;
    }
  }
};

class Replicas {
 public:
  // Debug checks: buffers allocated while on get a guard tail
  // of kGuardBytes filled with kGuardByte; every launch is then synchronised
  // (a fault names its kernel) and the guards of its arrays are verified, so
  // a kernel writing past the end of an array is reported by name.
  static constexpr size_t kGuardBytes = 4096;
  static constexpr unsigned char kGuardByte = 0xCE;

  explicit Replicas(const DeviceInfo& dev) : dev_(dev) {}
  ~Replicas() { release_all(); }
  Replicas(const Replicas&) = delete;
  Replicas& operator=(const Replicas&) = delete;

  // Device-visible pointer for a (CPU device: the host pointer); `checks`:
  // the replica carries a guard right past a.bytes.  Appended to the capture
  // log while one is set.
  void* buffer(const ArraySpec& a, bool checks);
  // graph capture: while a log is set, every (uid, pointer) handed out is
  // appended to it; buffer_is() tells whether uid still has that pointer
  void set_capture_log(std::vector<std::pair<uint64_t, void*>>* log);
  bool buffer_is(uint64_t uid, const void* ptr);
  void check_capturable(const ArraySpec& a);  // throws for pageable memory while capturing
  // After `kernel` on s: synchronises s and verifies the guards of arrs.
  void check_guards(hipStream_t s, const std::string& kernel, const std::vector<ArraySpec>& arrs);
  void release(uint64_t uid);
  void release_all();
  uint64_t bytes_allocated() const { return bytes_allocated_; }

 private:
  struct Replica {
    void* ptr = nullptr;    // hipMalloc'ed replica, if any
    uint64_t bytes = 0;     // its usable bytes (a guard, if any, lies past them)
    bool guarded = false;
    uint64_t guard_at = 0;  // guard offset (bytes) while guarded
    void* zc = nullptr;     // zero-copy: device view of the array's host memory
  };
  void* find_or_allocate(const ArraySpec& a, bool checks);

  const DeviceInfo& dev_;
  std::mutex mu_;  // guards everything below
  std::unordered_map<uint64_t, Replica> map_;
  std::vector<std::pair<uint64_t, void*>>* cap_log_ = nullptr;
  uint64_t bytes_allocated_ = 0;
};

}  // namespace cek
