// Host-side launch support shared by every launcher: the per-device dynamic-LDS opt-in, the device's CU count, schedule knobs as numbers and
// the budget of the bounded spins.
#pragma once
#include <atomic>
#include <hip/hip_runtime.h>
#include "common.hpp"

constexpr int MVAE_MAX_DEVICES = 64;

// Kernels that take more than the default 64 KB of dynamic LDS: raise the limit of each of KERNELS to `cap` bytes.  The attribute belongs
// to (kernel function, DEVICE), so it is set the first time this kernel set is reached on the current device -- once per device, not once
// per process; the state is one flag per device and per instantiation, i.e. per kernel set -- NOT per cap: a kernel set is always opted in
// with the same `cap` (each set has one call site today; a second site with a larger cap would find the flag set and change nothing).
// A device index outside [0, MVAE_MAX_DEVICES) is not remembered: the attribute is then set at every call.
template <auto... KERNELS> static inline hipError_t lds_opt_in(int cap) {
  static std::atomic<bool> done[MVAE_MAX_DEVICES];
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const bool known = dev >= 0 && dev < MVAE_MAX_DEVICES;
  if (known && done[dev].load(std::memory_order_acquire)) return hipSuccess;
  ((e = e != hipSuccess ? e : hipFuncSetAttribute(reinterpret_cast<const void*>(KERNELS), hipFuncAttributeMaxDynamicSharedMemorySize, cap)), ...);
  if (e == hipSuccess && known) done[dev].store(true, std::memory_order_release);
  return e;
}

// Compute units of the current device, asked once per device (same bounds rule as above; `inline`, not `static`: ONE cache for the library,
// which the knob helpers below cannot have -- they call the `static` mvae_knob); 0 when the runtime cannot say (no device): every schedule
// that needs all of its workgroups resident at once then answers "not served".
inline int device_cus() {
  static std::atomic<int> cached[MVAE_MAX_DEVICES];
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  const bool known = dev >= 0 && dev < MVAE_MAX_DEVICES;
  if (known && (cus = cached[dev].load(std::memory_order_relaxed)) > 0) return cus;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 0) return 0;
  if (known) cached[dev].store(cus, std::memory_order_relaxed);
  return cus;
}

// A schedule knob (mvae_knob: honoured under MVAE_TUNING=1 only) as a number / as a switch; `dflt` when it is not set.  Knobs are read per
// call, and every setting computes the same results: the GPU tests force each tile variant and schedule through them.
static inline int knob_int(const char* name, int dflt) {
  const char* v = mvae_knob(name);
  return v ? atoi(v) : dflt;
}
static inline bool knob_on(const char* name, bool dflt) { return knob_int(name, dflt ? 1 : 0) != 0; }

// Polling rounds a bounded spin may take before its launch gives up.  ~0.2 s (2^17 x ~1.6 us): far beyond any step or any wait for a compute
// unit, short enough that a launch that cannot make progress costs a fifth of a second, not two (a failure is survived, so the price of one
// is what matters).  `knob_name` (MVAE_PERSIST_SPIN / MVAE_ROWRES_SPIN; tests: 1 = give up at the first hand-off that is not there yet, which
// exercises the failure path) overrides it under MVAE_TUNING=1 only.
static inline uint32_t spin_limit(const char* knob_name) { return (uint32_t)knob_int(knob_name, 1u << 17); }
