// Kernel profiling timestamps (the counterpart of OpenCL's
// CL_PROFILING_COMMAND_START / END): a start and a stop event per launch that
// the runtime stamps from the dispatch itself.
#pragma once
#include <deque>

#include "device.h"

namespace cek {

class KernelStamps {
 public:
  explicit KernelStamps(const DeviceInfo& dev) : dev_(dev) {}
  ~KernelStamps();
  KernelStamps(const KernelStamps&) = delete;
  KernelStamps& operator=(const KernelStamps&) = delete;

  // A timing event for a launch: a spare one, else a new one.  The ring holds
  // up to 2 x kMax events, so it owns them raw and frees them with the device
  // set once; this is the part's one create / destroy pair.
  hipEvent_t event();
  // `kernel` was launched between start and stop.
  void push(const std::string& kernel, hipEvent_t start, hipEvent_t stop);
  // Waits for the recorded launches and drains them: (kernel, ms) in launch order.
  std::vector<std::pair<std::string, double>> drain();

 private:
  struct Stamp {
    std::string kernel;
    hipEvent_t start, stop;
  };
  static constexpr size_t kMax = 1 << 16;
  const DeviceInfo& dev_;
  std::mutex mu_;  // guards both containers
  std::deque<Stamp> stamps_;  // ring: the oldest are dropped past kMax
  std::vector<hipEvent_t> spare_;
};

}  // namespace cek
