#include "spans.h"

#include <algorithm>
#include <map>

namespace cek {

// Device-time span events only where they are read: every local device a
// GPU (with a CPU device in the set all devices share the host clock, see
// Cores::run_device_body) and more than one device in the whole job.  With
// one device there is no split to balance, so its compute time is the host's
// stopwatch (the reference's clock, Worker.cs:779-807) and no span events go
// into its streams (two event records and an elapsed-time query per
// synchronous compute).  CEK_SINGLE_DEVICE_SPANS=1 keeps them there.
bool Spans::on(const SpanModes& m) const {
  return m.device_spans && m.all_gpu && (m.global_devices > 1 || m.single_device_spans);
}

// An enqueued batch gets one span per device (opened by its first compute,
// closed when the mode is left) when no two local devices share a GPU: one
// local device (a rank of a distributed job) or distinct GPUs in one
// process.  Logical devices of one GPU keep a span per compute — their
// batches overlap on shared hardware, and only per-compute spans separate
// their busy time.
bool Spans::one_per_batch(const SpanModes& m) const {
  if (!m.enqueue_mode || m.async_enqueue) return false;
  std::vector<int> ords;
  for (const auto& w : workers_) {
    if (!w->gpu()) continue;
    const int o = w->dev().ordinal;
    if (std::find(ords.begin(), ords.end(), o) != ords.end()) return false;
    ords.push_back(o);
  }
  return true;
}

// pairs [0, n) of d's pool exist, both events of each created
static void grow(std::vector<std::pair<Event, Event>>& pool, size_t n, const Worker& wk) {
  while (pool.size() < n) {
    pool.emplace_back();
    pool.back().first.get(wk.dev(), kTimingEventFlags);
    pool.back().second.get(wk.dev(), kTimingEventFlags);
  }
}

void Spans::begin(Worker& wk, hipStream_t s, const SpanModes& m) {
  if (!wk.gpu() || !on(m)) return;
  Dev& d = dev_[wk.index()];
  if (one_per_batch(m)) {
    // no event marker sits between two back-to-back computes of the batch
    if (d.used > 0) return;
    grow(d.pool, 1, wk);
    d.used = 1;
    d.batch = s;
    d.gap = false;
    CEK_HIP(hipEventRecord(d.pool[0].first.peek(), s));
    return;
  }
  // enqueue mode keeps up to kMaxSpans pairs; past that the last pair's end
  // is re-recorded, so its span stretches over the remaining computes
  constexpr int kMaxSpans = 1024;
  if (m.enqueue_mode && d.used >= kMaxSpans) return;
  const int i = m.enqueue_mode ? d.used++ : 0;
  grow(d.pool, i + 1, wk);
  d.gap = false;
  CEK_HIP(hipEventRecord(d.pool[i].first.peek(), s));
}

void Spans::end(Worker& wk, hipStream_t s, const SpanModes& m) {
  if (!wk.gpu() || !on(m)) return;
  Dev& d = dev_[wk.index()];
  if (one_per_batch(m)) return;  // closed at the mode's end
  const int i = m.enqueue_mode ? d.used - 1 : 0;
  if (i < 0) return;
  CEK_HIP(hipEventRecord(d.pool[i].second.peek(), s));
}

void Spans::gap_begin(Worker& wk, hipStream_t s) {
  if (!wk.gpu()) return;
  Dev& d = dev_[wk.index()];
  const hipEvent_t a = d.gap_a.get(wk.dev(), kTimingEventFlags);
  d.gap_b.get(wk.dev(), kTimingEventFlags);
  CEK_HIP(hipEventRecord(a, s));
}

void Spans::gap_end(Worker& wk, hipStream_t s) {
  if (!wk.gpu()) return;
  Dev& d = dev_[wk.index()];
  CEK_HIP(hipEventRecord(d.gap_b.peek(), s));
  d.gap = true;
}

double Spans::ms(int w, const SpanModes& m) {
  Dev& d = dev_[w];
  if (!on(m) || d.pool.empty()) return -1.0;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, d.pool[0].first.peek(), d.pool[0].second.peek()) != hipSuccess) {
    (void)hipGetLastError();
    return -1.0;
  }
  double out = ms;
  if (d.gap) {
    float g = 0.f;
    if (hipEventElapsedTime(&g, d.gap_a.peek(), d.gap_b.peek()) == hipSuccess)
      out -= g;
    else
      (void)hipGetLastError();
  }
  return out;
}

void Spans::close_batch() {
  for (size_t w = 0; w < dev_.size(); ++w) {
    Dev& d = dev_[w];
    if (!d.batch || d.used <= 0) continue;
    workers_[w]->set_device();
    CEK_HIP(hipEventRecord(d.pool[0].second.peek(), d.batch));
    d.batch = nullptr;
  }
}

double Spans::enqueue_ms(int w) {
  Dev& d = dev_[w];
  const int n = d.used;
  d.used = 0;
  if (n <= 0) return -1.0;
  workers_[w]->set_device();
  std::vector<std::pair<double, double>> iv;
  for (int i = 0; i < n; ++i) {
    float b = 0.f, e = 0.f;
    if (hipEventElapsedTime(&b, d.pool[0].first.peek(), d.pool[i].first.peek()) != hipSuccess ||
        hipEventElapsedTime(&e, d.pool[0].first.peek(), d.pool[i].second.peek()) != hipSuccess) {
      (void)hipGetLastError();
      return -1.0;
    }
    iv.emplace_back(b, e);
  }
  std::sort(iv.begin(), iv.end());
  double total = 0, cb = iv[0].first, ce = iv[0].second;
  for (size_t i = 1; i < iv.size(); ++i) {
    if (iv[i].first > ce) {
      total += ce - cb;
      cb = iv[i].first;
      ce = iv[i].second;
    } else {
      ce = std::max(ce, iv[i].second);
    }
  }
  return total + (ce - cb);
}

void Spans::record_deferred_ends(int w) {
  Dev& d = dev_[w];
  for (const auto& p : pending_end_[w])
    if (p.index >= 0 && p.index < static_cast<int>(d.pool.size()))
      CEK_HIP(hipEventRecord(d.pool[p.index].second.peek(), p.s));
  pending_end_[w].clear();
}

Spans::Pending Spans::timeline_begin(Worker& wk, int compute_id, hipStream_t s) {
  Pending sp{wk.index(), compute_id, {}, {}};
  if (wk.gpu()) {
    sp.begin.get(wk.dev(), kTimingEventFlags);
    sp.end.get(wk.dev(), kTimingEventFlags);
    CEK_HIP(hipEventRecord(sp.begin.peek(), s));
  } else {
    sp.host_begin = now_ms();
  }
  return sp;
}

void Spans::timeline_end(Worker& wk, hipStream_t s, Pending&& sp) {
  if (wk.gpu())
    CEK_HIP(hipEventRecord(sp.end.peek(), s));
  else
    sp.host_end = now_ms();
  std::lock_guard<std::mutex> g(tl_mu_);
  pending_.push_back(std::move(sp));
}

std::vector<TimelineSpan> Spans::timeline() {
  std::vector<Pending> spans;  // their events are freed when this returns
  {
    std::lock_guard<std::mutex> g(tl_mu_);
    spans.swap(pending_);
  }
  std::vector<TimelineSpan> out;
  std::map<int, const Pending*> epoch;  // first span per device
  for (auto& sp : spans) epoch.emplace(sp.device, &sp);
  for (auto& sp : spans) {
    const Pending& e0 = *epoch.at(sp.device);
    TimelineSpan t{sp.device, sp.compute_id, 0, 0, 0, 0};
    if (sp.begin) {
      CEK_HIP(hipEventSynchronize(sp.end.peek()));
      float b = 0, e = 0;
      CEK_HIP(hipEventElapsedTime(&b, e0.begin.peek(), sp.begin.peek()));
      CEK_HIP(hipEventElapsedTime(&e, e0.begin.peek(), sp.end.peek()));
      t.begin_ms = b;
      t.end_ms = e;
      const int ord = workers_[sp.device]->dev().ordinal;
      t.abs_begin_ms = event_host_ms(ord, sp.begin.peek());
      t.abs_end_ms = event_host_ms(ord, sp.end.peek());
    } else {
      t.begin_ms = sp.host_begin - e0.host_begin;
      t.end_ms = sp.host_end - e0.host_begin;
      t.abs_begin_ms = sp.host_begin;
      t.abs_end_ms = sp.host_end;
    }
    out.push_back(t);
  }
  return out;
}

}  // namespace cek
