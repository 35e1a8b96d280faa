#include "markers.h"

#include "memory.h"

namespace cek {

Markers::Markers(const DeviceInfo& dev, const LaneTable& lanes) : dev_(dev), lanes_(lanes) {
  if (const char* e = std::getenv("CEK_MARKERS")) write_value_ = std::string(e) == "writevalue";
  if (dev_.type != kGPU) return;
  bool pinned = false;
  words_ = static_cast<uint64_t*>(host_alloc(kSlots * sizeof(uint64_t), 4096, &pinned));
  std::memset(words_, 0, kSlots * sizeof(uint64_t));
  // one lookup here instead of a runtime call (under HIP's lock) per marker
  words_dev_ = static_cast<uint64_t*>(host_device_ptr(words_));
}

Markers::~Markers() {
  if (dev_.type != kGPU) return;
  (void)hipSetDevice(dev_.ordinal);  // once, for the rings' events
  host_free(words_);
}

void Markers::defer(hipStream_t s, bool release) {
  if (dev_.type != kGPU) {  // a CPU device's compute is done when it returns
    add(s, release);
    return;
  }
  const int slot = lanes_.id_of(s);
  if (slot >= kNoLane || !lanes_.stream(slot)) {  // not a slot flush() can find again
    add(s, release);
    return;
  }
  last_slot_ = slot;  // issued_ counts the marker when it is recorded
  last_value_ = issued_per_slot_[slot] + 1;
  deferred_slots_ |= 1u << slot;
  if (release) deferred_release_ |= 1u << slot;
}

void Markers::flush() {
  for (int slot = 0; deferred_slots_ != 0 && slot < kNoLane; ++slot)
    if (deferred_slots_ & (1u << slot)) add(lanes_.stream(slot), false);
}

void Markers::add(hipStream_t s, bool release) {
  ++issued_;
  if (dev_.type != kGPU) {
    last_slot_ = -1;
    last_value_ = static_cast<uint64_t>(issued_);
    return;
  }
  int slot = lanes_.id_of(s);
  if (slot < kNoLane && (deferred_slots_ & (1u << slot))) {
    // this marker also completes the computes deferred on the same stream
    release = release || (deferred_release_ & (1u << slot));
    deferred_slots_ &= ~(1u << slot);
    deferred_release_ &= ~(1u << slot);
  }
  uint64_t v = ++issued_per_slot_[slot];
  last_slot_ = slot;
  last_value_ = v;
  if (write_value_) {
    CEK_HIP(hipStreamWriteValue64(s, words_dev_ + slot, v, 0));
    return;
  }
  std::lock_guard<std::mutex> g(mu_);
  Ring& r = rings_[slot];
  auto& spare = release ? r.spare_fenced : r.spare;
  Event e;
  if (!spare.empty()) {
    e = std::move(spare.front());
    spare.pop_front();
  }
  // no timing; no system-scope release unless host memory was written: a
  // completion signal only
  CEK_HIP(hipEventRecord(e.get(dev_, release ? hipEventDisableTiming
                                             : (hipEventDisableTiming | hipEventDisableSystemFence)),
                         s));
  r.pending.emplace_back(std::move(e), release);
}

uint64_t Markers::word(int slot) {
  if (dev_.type != kGPU || slot < 0) return static_cast<uint64_t>(issued_);
  if (write_value_) return __atomic_load_n(&words_[slot], __ATOMIC_ACQUIRE);
  std::lock_guard<std::mutex> g(mu_);
  Ring& r = rings_[slot];
  while (!r.pending.empty()) {
    auto& front = r.pending.front();
    const hipError_t q = hipEventQuery(front.first.peek());
    if (q == hipErrorNotReady) break;
    if (q != hipSuccess) {
      (void)hipGetLastError();
      throw Error("marker event query failed on " + dev_.name);
    }
    (front.second ? r.spare_fenced : r.spare).push_back(std::move(front.first));
    r.pending.pop_front();
    ++r.done;
  }
  return r.done;
}

long long Markers::reached() {
  if (dev_.type != kGPU) return issued_;
  long long r = 0;
  for (int i = 0; i < kSlots; ++i) r += static_cast<long long>(word(i));
  return r;
}

}  // namespace cek
