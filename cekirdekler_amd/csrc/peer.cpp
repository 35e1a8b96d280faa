#include "peer.h"

#include <algorithm>
#include <tuple>

#include "cores.h"  // ComputeCall
#include "xgmi.h"

namespace cek {

void PeerTraffic::bind() {
  const size_t n = workers_.size();
  peer_ev_.resize(n);
  peer_ready_.resize(n);
  kdone_.resize(n);
  pushed_.resize(n);
  ord_index_.assign(n, -1);
  peer_ordinals_.clear();
  for (size_t w = 0; w < n; ++w) {
    if (!workers_[w]->gpu()) continue;
    const int o = workers_[w]->dev().ordinal;
    auto it = std::find(peer_ordinals_.begin(), peer_ordinals_.end(), o);
    ord_index_[w] = static_cast<int>(it - peer_ordinals_.begin());
    if (it == peer_ordinals_.end()) peer_ordinals_.push_back(o);
  }
  if (peer_ordinals_.size() >= 2) {
    peer_matrix_ = enable_peer_access_among(peer_ordinals_);
  } else {
    peer_matrix_.assign(peer_ordinals_.size(), std::vector<int>(peer_ordinals_.size(), 1));
  }
  p2p_path_ = peer_path(peer_matrix_);
}

bool PeerTraffic::can_peer(int w1, int w2) const {
  const int a = ord_index_.at(w1), b = ord_index_.at(w2);
  if (a < 0 || b < 0) return false;
  return a == b || (peer_matrix_[a][b] && peer_matrix_[b][a]);
}

void PeerTraffic::count_d2d(int ws, int wd, uint64_t bytes) {
  d2d.bytes += bytes;
  if (ord_index_[ws] == ord_index_[wd])
    d2d.local += bytes;
  else if (can_peer(ws, wd))
    d2d.xgmi += bytes;
  else
    d2d.staged += bytes;
}

// One device→device copy on stream s of local worker sw (either end): a D2D
// copy inside one GPU, a peer copy between GPUs (over xGMI when peer access
// is on; the runtime stages it through host memory otherwise), by SDMA or a
// copy kernel on sw's GPU, whichever the calibrated engine table says is
// faster for this pair and size (xgmi.h; SDMA for an uncalibrated pair).
uint64_t PeerTraffic::d2d_copy(int ws, int wd, char* dst, const char* src, uint64_t bytes, hipStream_t s, int sw) {
  if (!bytes || dst == src) return 0;
  const int os = workers_[ws]->dev().ordinal, od = workers_[wd]->dev().ordinal;
  const bool peer_ok = os == od || can_peer(ws, wd);
  if (peer_ok)
    peer_copy(dst, od, src, os, bytes, s, workers_[sw]->dev().ordinal);
  else
    CEK_HIP(hipMemcpyPeerAsync(dst, od, src, os, bytes, s));  // staged by the runtime
  count_d2d(ws, wd, bytes);
  return bytes;
}

void PeerTraffic::wait_gather(Worker& wk, hipStream_t s) {
  if (!gather_pending) return;
  for (const Event& p : pushed_) {
    if (!p) continue;
    if (wk.gpu())
      CEK_HIP(hipStreamWaitEvent(s, p.peek(), 0));
    else
      CEK_HIP(hipEventSynchronize(p.peek()));
  }
}

// Keep-resident gather of the call's `arrays` (indices into c.arrays): each
// device's slice (by this call's split) lands in every other device's replica.
// Issued from the calling thread once every device has enqueued its kernels:
// GPU g's main stream waits for the kernels of every GPU (no replica is
// overwritten while a kernel of this call still reads it), pulls the CPU
// device's slices from host memory, pushes its own slice to every other
// replica (peer copies over xGMI), and records pushed_[g].  No host sync in
// enqueue mode; otherwise the copies are complete when compute() returns.
uint64_t PeerTraffic::issue_gather(const ComputeCall& c, const BalancerState& st, const std::vector<int>& arrays,
                                   const PeerView& v,
                                   const std::vector<std::vector<std::pair<long long, long long>>>* owned) {
  const int n = static_cast<int>(workers_.size());
  std::vector<int> on;  // enabled local devices: they hold replicas
  for (int w = 0; w < n; ++w)
    if (v.enabled[w]) on.push_back(w);
  if (on.size() < 2 || arrays.empty()) return 0;
  // the work-item ranges each device holds fresh results for: its own slice
  // of this call's split, or (after a failover) its slice plus the slices it
  // recomputed for failed devices
  std::vector<std::vector<std::pair<long long, long long>>> own(n);
  for (int w : on) {
    if (owned)
      own[w] = (*owned)[w];
    else
      own[w].push_back({st.references[v.global_base + w], st.ranges[v.global_base + w]});
  }
  uint64_t moved = 0;
  struct Piece {
    std::vector<char*> ptr;
    std::vector<std::vector<std::pair<uint64_t, uint64_t>>> seg;  // per worker: (byte offset, bytes)
  };
  std::vector<Piece> pcs(arrays.size());
  for (size_t i = 0; i < arrays.size(); ++i) {
    const ArraySpec& a = c.arrays[arrays[i]];
    Piece& p = pcs[i];
    p.ptr.assign(n, nullptr);
    p.seg.assign(n, {});
    for (int w : on) {
      for (auto& r : own[w]) {
        uint64_t b, k;
        a.slice(r.first, r.second, c.local_range, b, k);
        const uint64_t off = std::min<uint64_t>(b * a.elem_size, a.bytes);
        const uint64_t len = std::min<uint64_t>(k * a.elem_size, a.bytes - off);
        if (len) p.seg[w].push_back({off, len});
      }
      workers_[w]->set_device();
      p.ptr[w] = static_cast<char*>(workers_[w]->buffer(a));
    }
  }
  std::vector<int> gpus;
  for (int w : on)
    if (workers_[w]->gpu()) gpus.push_back(w);
  for (int g : gpus) {
    Worker& wg = *workers_[g];
    wg.set_device();
    hipStream_t m = wg.main_stream();
    for (int d : gpus)
      if (kdone_[d]) CEK_HIP(hipStreamWaitEvent(m, kdone_[d].peek(), 0));
    for (size_t i = 0; i < arrays.size(); ++i) {
      const ArraySpec& a = c.arrays[arrays[i]];
      Piece& p = pcs[i];
      for (int s : on) {  // the CPU device's slices: host → this replica
        if (workers_[s]->gpu()) continue;
        for (auto& sg : p.seg[s]) {
          CEK_HIP(hipMemcpyAsync(p.ptr[g] + sg.first, static_cast<const char*>(a.host) + sg.first, sg.second,
                                 hipMemcpyHostToDevice, m));
          moved += sg.second;
        }
      }
      for (auto& sg : p.seg[g]) {
        for (int d : on) {  // this GPU's slices → every other replica
          if (d == g || p.ptr[d] == p.ptr[g]) continue;
          if (workers_[d]->gpu()) {
            moved += d2d_copy(g, d, p.ptr[d] + sg.first, p.ptr[g] + sg.first, sg.second, m, g);
            log_.add(v.global_base + d, "gather", 0, static_cast<long long>(sg.first),
                     static_cast<long long>(sg.second), v.global_base + g);
          } else {
            CEK_HIP(hipMemcpyAsync(p.ptr[d] + sg.first, p.ptr[g] + sg.first, sg.second, hipMemcpyDeviceToHost, m));
            moved += sg.second;
          }
        }
      }
    }
    CEK_HIP(hipEventRecord(pushed_[g].get(wg.dev()), m));
  }
  gather_pending = true;
  if (!v.enqueue_mode) {
    for (int g : gpus) {
      workers_[g]->set_device();
      CEK_HIP(hipStreamSynchronize(workers_[g]->main_stream()));
    }
    gather_pending = false;
  }
  return moved;
}

void PeerTraffic::copy_between(int src_dev, const ArraySpec& src, int dst_dev, const ArraySpec& dst, uint64_t bytes,
                               bool enqueue_mode) {
  Worker& ws = *workers_.at(src_dev);
  Worker& wd = *workers_.at(dst_dev);
  if (ws.gpu() && wd.gpu()) {
    // On the source's main stream, after everything queued on either
    // device (every stream: with async enqueue a compute may sit on a
    // compute queue, still writing the source or reading the destination).
    // Later work on ANY stream of either device waits for the copy through
    // the gather-pending events (no host sync in enqueue mode).
    ws.set_device();
    void* sp = ws.buffer(src);
    wd.set_device();
    void* dp = wd.buffer(dst);
    wd.join_streams(wd.main_stream());
    hipEvent_t before = kdone_[dst_dev].get(wd.dev());
    CEK_HIP(hipEventRecord(before, wd.main_stream()));
    ws.set_device();
    hipStream_t s = ws.main_stream();
    wait_gather(ws, s);
    ws.join_streams(s);
    CEK_HIP(hipStreamWaitEvent(s, before, 0));
    d2d = D2DCount();
    d2d_copy(src_dev, dst_dev, static_cast<char*>(dp), static_cast<const char*>(sp), bytes, s, src_dev);
    hipEvent_t after = pushed_[src_dev].get(ws.dev());
    CEK_HIP(hipEventRecord(after, s));
    wd.set_device();
    CEK_HIP(hipStreamWaitEvent(wd.main_stream(), after, 0));
    gather_pending = true;  // compute streams of both devices wait on `after` too
    if (!enqueue_mode) {
      ws.set_device();
      CEK_HIP(hipStreamSynchronize(s));
      gather_pending = false;
    }
    return;
  }
  if (ws.gpu()) {  // GPU → CPU device (host memory)
    ws.set_device();
    hipStream_t s = ws.main_stream();
    CEK_HIP(hipMemcpyAsync(dst.host, ws.buffer(src), bytes, hipMemcpyDeviceToHost, s));
    CEK_HIP(hipStreamSynchronize(s));
  } else {  // CPU → GPU
    wd.set_device();
    hipStream_t s = wd.main_stream();
    CEK_HIP(hipMemcpyAsync(wd.buffer(dst), src.host, bytes, hipMemcpyHostToDevice, s));
    CEK_HIP(hipStreamSynchronize(s));
  }
}

void PeerTraffic::share_slices(const BalancerState& st, const ArraySpec& a, long long local_range,
                               const PeerView& v) {
  // the copies follow whatever is queued on every GPU's main stream
  for (size_t w = 0; w < workers_.size(); ++w) {
    Worker& wk = *workers_[w];
    if (!wk.gpu() || !v.enabled[w]) continue;
    wk.set_device();
    wait_gather(wk, wk.main_stream());
    CEK_HIP(hipEventRecord(kdone_[w].get(wk.dev()), wk.main_stream()));
  }
  ComputeCall c;
  c.arrays = {a};
  c.local_range = local_range;
  d2d = D2DCount();
  issue_gather(c, st, {0}, v);
}

uint64_t PeerTraffic::stage_reads(const ComputeCall& c, const std::vector<long long>& ranges,
                                  std::vector<uint64_t>& h2d, const PeerView& v, bool allowed, uint64_t min_bytes) {
  const int nloc = static_cast<int>(workers_.size());
  staged_arr_.assign(c.arrays.size(), 0);
  staged_dev_.assign(nloc, 0);
  if (!allowed) return 0;
  std::vector<int> part;  // local GPUs computing in this call
  for (int w = 0; w < nloc; ++w)
    if (workers_[w]->gpu() && v.enabled[w] && ranges[v.global_base + w] > 0) part.push_back(w);
  const int P = static_cast<int>(part.size());
  if (P < 2) return 0;
  // every pair of distinct GPUs must peer; otherwise each device uploads the
  // whole array over its own PCIe link (reference behaviour), explicitly
  for (int x = 0; x < P; ++x)
    for (int y = 0; y < P; ++y)
      if (!can_peer(part[x], part[y])) {
        d2d.pcie_fallback = true;
        return 0;
      }
  bool any = false;
  for (size_t i = 0; i < c.arrays.size(); ++i) {
    const auto& a = c.arrays[i];
    if (!a.zc && a.read && !a.partial && !a.write && !a.wo && !a.write_all && a.bytes >= min_bytes) {
      staged_arr_[i] = 1;
      any = true;
    }
  }
  if (!any) return 0;
  for (int w : part) {
    const Worker& wk = *workers_[w];
    wk.set_device();
    peer_ev_[w].up.get(wk.dev());
    peer_ev_[w].pulled.get(wk.dev());
    staged_dev_[w] = 1;
  }
  auto up = [&](int k) { return peer_ev_[part[k]].up.peek(); };
  auto pulled = [&](int k) { return peer_ev_[part[k]].pulled.peek(); };
  uint64_t p2p = 0;
  for (size_t i = 0; i < c.arrays.size(); ++i) {
    if (!staged_arr_[i]) continue;
    const auto& a = c.arrays[i];
    // chunk k of P: 4 KiB-aligned byte ranges (multiples of every element size)
    std::vector<uint64_t> off(P), len(P);
    std::vector<char*> ptr(P);
    for (int k = 0; k < P; ++k) {
      std::tie(off[k], len[k]) = byte_chunk(a.bytes, P, 4096, k);
      workers_[part[k]]->set_device();
      ptr[k] = static_cast<char*>(workers_[part[k]]->buffer(a));
    }
    // 1) every GPU uploads its chunk over its own PCIe link, after the peers
    //    finished pulling from its replica in the previous call (enqueue mode
    //    runs ahead without host syncs)
    for (int k = 0; k < P; ++k) {
      Worker& wk = *workers_[part[k]];
      wk.set_device();
      hipStream_t m = wk.main_stream();
      for (int j = 0; j < P; ++j)
        if (j != k) CEK_HIP(hipStreamWaitEvent(m, pulled(j), 0));
      if (len[k]) {
        CEK_HIP(hipMemcpyAsync(ptr[k] + off[k], static_cast<const char*>(a.host) + off[k], len[k],
                               hipMemcpyHostToDevice, m));
        h2d[part[k]] += len[k];
      }
      CEK_HIP(hipEventRecord(up(k), m));
    }
    // 2) every GPU pulls the other chunks from their owners over xGMI
    for (int k = 0; k < P; ++k) {
      Worker& wd = *workers_[part[k]];
      wd.set_device();
      hipStream_t m = wd.main_stream();
      for (int j = 0; j < P; ++j) {
        if (j == k || !len[j]) continue;
        CEK_HIP(hipStreamWaitEvent(m, up(j), 0));
        p2p += d2d_copy(part[j], part[k], ptr[k] + off[j], ptr[j] + off[j], len[j], m, part[k]);
        log_.add(v.global_base + part[k], "p2p", 0, static_cast<long long>(off[j]), static_cast<long long>(len[j]),
                 v.global_base + part[j]);
      }
      CEK_HIP(hipEventRecord(pulled(k), m));
    }
  }
  // 3) a GPU's kernels may modify a staged array in place (read without
  //    write-back does not mean const): they start only once every peer has
  //    pulled this GPU's chunk out of its replica
  for (int k = 0; k < P; ++k) {
    Worker& wk = *workers_[part[k]];
    wk.set_device();
    hipStream_t m = wk.main_stream();
    for (int j = 0; j < P; ++j)
      if (j != k) CEK_HIP(hipStreamWaitEvent(m, pulled(j), 0));
    CEK_HIP(hipEventRecord(peer_ready_[part[k]].get(wk.dev()), m));
  }
  return p2p;
}

}  // namespace cek
