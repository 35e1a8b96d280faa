#include "graphs.h"

namespace cek {

// Ends w's capture: the captured graph, or null with *e set (the sticky
// error cleared).
static hipGraph_t end_capture(Worker& w, hipError_t* e) {
  w.set_device();
  hipGraph_t g = nullptr;
  *e = hipStreamEndCapture(w.main_stream(), &g);
  if (*e != hipSuccess) (void)hipGetLastError();
  w.set_capture_log(nullptr);
  return *e == hipSuccess ? g : nullptr;
}

void ComputeGraphs::destroy_execs(std::vector<hipGraphExec_t>& execs) {
  for (size_t i = 0; i < execs.size() && i < workers_.size(); ++i)
    if (execs[i]) {
      workers_[i]->set_device();
      (void)hipGraphExecDestroy(execs[i]);
      execs[i] = nullptr;
    }
}

ComputeGraphs::~ComputeGraphs() {
  for (auto& kv : graphs_) destroy_execs(kv.second);
}

void ComputeGraphs::discard_capture(size_t n) {
  for (size_t i = 0; i < n && i < workers_.size(); ++i) {
    hipError_t e;
    if (hipGraph_t g = end_capture(*workers_[i], &e)) (void)hipGraphDestroy(g);
  }
}

void ComputeGraphs::begin(const CaptureSaved& saved) {
  saved_ = saved;
  cap_logs_.assign(workers_.size(), {});
  for (size_t i = 0; i < workers_.size(); ++i) {
    Worker& w = *workers_[i];
    w.set_device();
    hipError_t e = hipStreamBeginCapture(w.main_stream(), hipStreamCaptureModeRelaxed);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      discard_capture(i);
      throw Error(std::string("hipStreamBeginCapture failed on ") + w.dev().name + ": " + hipGetErrorString(e));
    }
    w.set_capture_log(&cap_logs_[i]);
  }
}

int ComputeGraphs::end(std::string& err) {
  for (auto& w : workers_) {
    w->wait();
    w->set_capture_log(nullptr);
  }
  std::vector<hipGraphExec_t> execs(workers_.size(), nullptr);
  for (size_t i = 0; i < workers_.size(); ++i) {
    Worker& w = *workers_[i];
    hipError_t e;
    hipGraph_t g = end_capture(w, &e);
    if (!g) {
      err = std::string("stream capture failed on ") + w.dev().name + ": " + hipGetErrorString(e);
      continue;
    }
    e = hipGraphInstantiate(&execs[i], g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      err = std::string("graph instantiation failed on ") + w.dev().name + ": " + hipGetErrorString(e);
    }
  }
  if (!err.empty()) {
    destroy_execs(execs);
    return 0;
  }
  const int id = next_id_++;
  graphs_[id] = std::move(execs);
  graph_bufs_[id] = std::move(cap_logs_);
  cap_logs_.clear();
  return id;
}

void ComputeGraphs::launch(int id, int times, bool sync) {
  auto it = graphs_.find(id);
  if (it == graphs_.end()) throw Error("graph_launch: unknown graph id");
  const auto& bufs = graph_bufs_[id];
  for (size_t i = 0; i < bufs.size() && i < workers_.size(); ++i)
    for (const auto& ub : bufs[i])
      if (!workers_[i]->buffer_is(ub.first, ub.second))
        throw Error("graph " + std::to_string(id) + " is stale: array " + std::to_string(ub.first) +
                    " was released or reallocated on " + workers_[i]->dev().name +
                    " since the capture (capture it again)");
  for (size_t i = 0; i < workers_.size(); ++i) {
    if (!it->second[i]) continue;
    Worker& w = *workers_[i];
    w.set_device();
    for (int r = 0; r < times; ++r) CEK_HIP(hipGraphLaunch(it->second[i], w.main_stream()));
  }
  if (sync)
    for (auto& w : workers_) {
      w->set_device();
      CEK_HIP(hipStreamSynchronize(w->main_stream()));
    }
}

void ComputeGraphs::destroy(int id) {
  auto it = graphs_.find(id);
  if (it == graphs_.end()) return;
  destroy_execs(it->second);
  graphs_.erase(it);
  graph_bufs_.erase(id);
}

}  // namespace cek
