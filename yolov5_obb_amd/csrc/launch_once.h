// Host-side launch helpers: what the library remembers per device.  Included by the headers whose host code launches kernels
// (HIP translation units only: the device headers that tests/native/*.cpp compiles for the host, without a HIP runtime, stay clear
// of it).
#pragma once
#include <atomic>
#include <stddef.h>
#include <hip/hip_runtime.h>

namespace obb {

// hipFuncSetAttribute applies to the function ON THE CURRENT DEVICE: a process that drives several GPUs has to raise a kernel's
// dynamic-LDS limit on each of them.  One of these per kernel (a function-local static).  need() returns the index of the current
// device when the attribute still has to be set there (or kAlways when the device cannot be told: set it every time), kDone when
// it was; the caller hands that index back to mark() AFTER the attribute call succeeded.  The index lives in the caller's frame,
// not in this shared object: two host threads on different GPUs cannot mark each other's device, and two threads on
// the same GPU at worst both set the attribute, which is harmless.
// the index of the current device, or -1 when it cannot be told
inline int current_device() {
  int dev = -1;
  return (hipGetDevice(&dev) == hipSuccess && dev >= 0) ? dev : -1;
}

struct OncePerDevice {
  static constexpr int kDone = -1, kAlways = -2;
  std::atomic<bool> seen[64] = {};
  __attribute__((noinline)) int need() const { return need(current_device()); }   // (one out-of-line copy, whoever asks)
  // dev: current_device() as the caller has read it already (a call of the drivers asks once: nms_driver.h, DeviceCus)
  int need(int dev) const {
    if (dev < 0 || dev >= 64) return kAlways;
    return seen[dev].load(std::memory_order_acquire) ? kDone : dev;
  }
  void mark(int dev) { if (dev >= 0 && dev < 64) seen[dev].store(true, std::memory_order_release); }
};

// The need / set / mark sequence, written once: raises the dynamic-LDS limit of every listed kernel to `bytes` on the current
// device unless `once` says it was done there.  The device is marked only after EVERY set succeeded; false: a set failed (the
// caller returns OBB_ERR_LAUNCH, and the next call tries again).  raise_lds_once_on: for a caller that knows current_device().
template <class... Kernel>
inline bool raise_lds_needed(int need, OncePerDevice& once, size_t bytes, Kernel... kernel) {   // need: what once.need said
  if (need == OncePerDevice::kDone) return true;
  if (!((hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess) && ...)) return false;
  once.mark(need);
  return true;
}
template <class... Kernel>
inline bool raise_lds_once(OncePerDevice& once, size_t bytes, Kernel... kernel) {
  return raise_lds_needed(once.need(), once, bytes, kernel...);
}
template <class... Kernel>
inline bool raise_lds_once_on(int dev, OncePerDevice& once, size_t bytes, Kernel... kernel) {
  return raise_lds_needed(once.need(dev), once, bytes, kernel...);
}

// A positive int per device, asked once per device (0: not asked yet): the same 64-slot table.  A device outside the table, or
// one that cannot be told (dev < 0), has no slot: get() says 0 and the caller asks every time.
struct IntPerDevice {
  std::atomic<int> v[64] = {};
  int get(int dev) const { return (dev >= 0 && dev < 64) ? v[dev].load(std::memory_order_acquire) : 0; }
  void set(int dev, int x) { if (dev >= 0 && dev < 64) v[dev].store(x, std::memory_order_release); }
};

}  // namespace obb
