// The dynamic-LDS limit of the kernels that need more than the default 64 KiB (gfx950: 160 KiB per CU).
// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the (kernel, device) pair, so every launch site keeps one DeviceOnce per
// kernel instantiation and raises the limit at the kernel's first launch on each device: lazily, so that nothing happens at
// load time, and outside any stream capture (engine_dec.hip runs the first call of every captured signature eagerly).
#pragma once
#include <atomic>
#include <mutex>

namespace sampt {

// Runs a callable the first time a device ordinal is seen; needs no HIP header (tests/device_once_main.cpp builds it alone).
class DeviceOnce {
 public:
  static constexpr int MAX_DEVICES = 64;    // an ordinal outside the table runs the callable every time
  // f() returns 0 for success.  The result of f(), or 0 where f has already succeeded for this ordinal; a failure is not
  // remembered, so the next call tries again.  Safe from several host threads, on the same or on different ordinals.
  template <class F>
  int run(int device, F&& f) {
    if (device < 0 || device >= MAX_DEVICES) return f();
    if (done_[device].load(std::memory_order_acquire)) return 0;
    std::lock_guard<std::mutex> lock(mu_);
    if (done_[device].load(std::memory_order_relaxed)) return 0;
    const int rc = f();
    if (rc == 0) done_[device].store(true, std::memory_order_release);
    return rc;
  }

 private:
  std::mutex mu_;
  std::atomic<bool> done_[MAX_DEVICES] = {};
};

}  // namespace sampt

#ifdef __HIPCC__
#include <string>

#include "common.h"

namespace sampt {

// Lets `kernel` be launched with up to `bytes` of dynamic LDS on the current device; one hipGetDevice per call after the first.
inline int allow_dynamic_lds(DeviceOnce& once, const void* kernel, int bytes, const char* who) {
  int device = -1;
  const char* what = ": hipGetDevice";
  hipError_t e = hipGetDevice(&device);
  if (e == hipSuccess) {
    what = ": hipFuncSetAttribute";
    e = (hipError_t)once.run(device, [&] { return (int)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); });
  }
  if (e == hipSuccess) return SAMPT_OK;
  set_error((std::string(who) + what).c_str(), e);
  return SAMPT_ERR_HIP;
}

}  // namespace sampt
#endif
