#include "downloads.h"

#include <algorithm>

#include "cores.h"  // ComputeCall

namespace cek {

bool DeferredDownloads::must_flush_before(const Worker& wk, hipStream_t s, const ComputeCall& c) const {
  for (const auto& p : pending_[wk.index()]) {
    if (p.s == s) return true;
    for (const auto& a : c.arrays)
      if (!a.zc && a.uid == p.a.uid) return true;
  }
  return false;
}

void DeferredDownloads::flush(Worker& wk, hipStream_t next, const ComputeCall* c) {
  const int w = wk.index();
  auto& pd = pending_[w];
  std::vector<hipStream_t> order;  // streams `next` must wait for
  for (const auto& p : pd) {
    wk.d2h(p.s, p.a, p.begin, p.count);
    if (c && p.s != next && std::find(order.begin(), order.end(), p.s) == order.end())
      for (const auto& a : c->arrays)
        if (!a.zc && a.uid == p.a.uid) {
          order.push_back(p.s);
          break;
        }
  }
  if (!order.empty() && wk.gpu()) {
    auto& ev = order_events_[w];
    while (ev.size() < order.size()) {
      ev.emplace_back();
      ev.back().get(wk.dev());
    }
    for (size_t i = 0; i < order.size(); ++i) {
      CEK_HIP(hipEventRecord(ev[i].peek(), order[i]));
      CEK_HIP(hipStreamWaitEvent(next, ev[i].peek(), 0));
    }
  }
  pd.clear();
}

std::vector<hipStream_t> DeferredDownloads::streams_holding(int w, uint64_t uid) const {
  std::vector<hipStream_t> streams;
  for (const auto& p : pending_[w])
    if (p.a.uid == uid && std::find(streams.begin(), streams.end(), p.s) == streams.end()) streams.push_back(p.s);
  return streams;
}

}  // namespace cek
