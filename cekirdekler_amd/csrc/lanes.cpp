#include "lanes.h"

#include "jit.h"

namespace cek {

hipStream_t LaneTable::new_stream(bool copy_cus) {
  CEK_HIP(hipSetDevice(dev_.ordinal));
  hipStream_t s = nullptr;
  const int ncu = std::max(1, dev_.compute_units);
  std::vector<uint32_t> mask((ncu + 31) / 32, 0);
  if (dev_.cu_parts > 1) {
    // a CU-partitioned logical device: every stream (copy-kernel ones too)
    // sees its partition's CUs only
    for (int cu : partition_cus(ncu, dev_.cu_parts, dev_.cu_part)) mask[cu / 32] |= 1u << (cu % 32);
  } else if (cu_reserve_ <= 0) {
    CEK_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    return s;
  } else {
    const int every = std::max(1, ncu / cu_reserve_);
    for (int cu = 0; cu < ncu; ++cu) {
      const bool reserved = (cu % every) == every - 1 && cu / every < cu_reserve_;
      if (reserved == copy_cus) mask[cu / 32] |= 1u << (cu % 32);
    }
  }
  CEK_HIP(hipExtStreamCreateWithCUMask(&s, static_cast<uint32_t>(mask.size()), mask.data()));
  return s;
}

hipStream_t LaneTable::open(int id) {
  if (dev_.type != kGPU) return nullptr;
  const bool compute = id >= compute_lane_id(0) && id < pipe_lane_id(0, 0);
  if (compute && qconc_ == 1) id = main_lane_id();
  hipStream_t& s = s_[id];
  // the pipeline's write lanes run their copy kernels on the reserved CUs
  if (!s) s = new_stream(id >= pipe_lane_id(0, 0) && (id - pipe_lane_id(0, 0)) % 3 == 2);
  return s;
}

int LaneTable::id_of(hipStream_t s) const {
  for (int id = 0; id < pipe_lane_id(2, 0); ++id)
    if (s_[id] == s) return id;
  return kNoLane;
}

void LaneTable::sync_all() const {
  if (dev_.type != kGPU) return;
  CEK_HIP(hipSetDevice(dev_.ordinal));
  for_each_created([](hipStream_t s, int) { CEK_HIP(hipStreamSynchronize(s)); });
}

void LaneTable::join(hipStream_t target) {
  if (dev_.type != kGPU) return;
  CEK_HIP(hipSetDevice(dev_.ordinal));
  for_each_created([&](hipStream_t s, int id) {
    if (s == target) return;
    const hipEvent_t e = join_ev_[id].get(dev_);
    CEK_HIP(hipEventRecord(e, s));
    CEK_HIP(hipStreamWaitEvent(target, e, 0));
  });
}

void LaneTable::destroy() {
  if (dev_.type != kGPU) return;
  (void)hipSetDevice(dev_.ordinal);
  for (auto& dq : dyn_queues_) (void)hipFree(dq.second);
  dyn_queues_.clear();
  for (auto& s : s_) {
    if (s) (void)hipStreamDestroy(s);
    s = nullptr;
  }
}

void LaneTable::set_cu_reserve(int n) {
  if (dev_.type != kGPU) return;
  n = std::max(0, std::min(n, std::max(0, dev_.compute_units / 2)));
  if (n == cu_reserve_) return;
  sync_all();
  destroy();
  cu_reserve_ = n;
}

void* LaneTable::enqueue_queue(hipStream_t s) {
  void*& q = dyn_queues_[s];
  if (!q) {
    CEK_HIP(hipSetDevice(dev_.ordinal));
    CEK_HIP(hipMalloc(&q, kDynQueueBytes));
    // on the queue's own stream: a memset on the null stream is not ordered
    // with these (non-blocking) streams and could clear the level counts after
    // the first parent had enqueued
    CEK_HIP(hipMemsetAsync(q, 0, kDynHeaderBytes, s));
  }
  return q;
}

}  // namespace cek
