// State the square-shell GEMM streamer (shell_gemm.cpp) keeps per device
// between calls: the per-kernel dims block in device memory, what it holds,
// and the pinned staging buffer it is uploaded from.
#pragma once
#include "worker.h"

namespace cek {

struct ShellDims {
  ShellDims() = default;
  ShellDims(const ShellDims&) = delete;
  ~ShellDims();  // frees both buffers, the device one with its device current

  // At least `bytes` of device and staging memory on wk's device (current);
  // drains `up` before a smaller block is replaced.
  void reserve(const Worker& wk, size_t bytes, hipStream_t up);

  void* dev = nullptr;
  size_t cap = 0;
  std::vector<int> host;  // what dev holds (re-uploaded only on change)
  void* pin = nullptr;    // pinned staging for that upload
  int ordinal = -1;
};

}  // namespace cek
