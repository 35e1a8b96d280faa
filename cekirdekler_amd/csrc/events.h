// An owning HIP event, created on first use: the worker's and the scheduler's
// parts need most of their events only on some paths, a CPU-only cruncher must
// not touch HIP for them, and a stream capture must see no creation it did not
// see before.
#pragma once
#include "device.h"

namespace cek {

class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : e_(o.e_), ordinal_(o.ordinal_) { o.e_ = nullptr; }
  Event& operator=(Event&& o) noexcept {
    std::swap(e_, o.e_);
    std::swap(ordinal_, o.ordinal_);
    return *this;
  }
  ~Event() {
    // destroyed with its device current; the calling thread's device is put
    // back (timeline() frees events on the caller's thread)
    if (!e_) return;
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != ordinal_) (void)hipSetDevice(ordinal_);
    (void)hipEventDestroy(e_);
    if (prev >= 0 && prev != ordinal_) (void)hipSetDevice(prev);
  }

  // The event; the first call creates it with `flags` on GPU `dev`.
  hipEvent_t get(const DeviceInfo& dev, unsigned flags = hipEventDisableTiming) {
    if (!e_) {
      CEK_HIP(hipSetDevice(dev.ordinal));
      CEK_HIP(hipEventCreateWithFlags(&e_, flags));
      ordinal_ = dev.ordinal;
    }
    return e_;
  }
  // The event if get() created it, else null (nothing was recorded on it yet).
  hipEvent_t peek() const { return e_; }
  explicit operator bool() const { return e_ != nullptr; }

 private:
  hipEvent_t e_ = nullptr;
  int ordinal_ = -1;
};

}  // namespace cek
