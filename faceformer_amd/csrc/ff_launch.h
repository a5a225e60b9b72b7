// Host side of a kernel launch, shared by the GEMM and attention files: the per-device bound, the once-per-(kernel, device)
// dynamic-LDS attribute, the run-time value -> template argument dispatcher, settings written by setters while launches read
// them, and the per-(device, stream) workspace areas.  Host code only: nothing here is read by a kernel.
#pragma once
#include <atomic>
#include <mutex>
#include <type_traits>
#include <vector>

#include "ff_common.h"

// devices per process that get cached per-device state (attribute flags, ff_num_cus(), the engine's stream pools)
constexpr int FF_MAX_DEVICES = 16;

// hipFuncSetAttribute is per device: one flag per (kernel, device); the attribute is idempotent, host threads may race here.
// A device index outside the tracked range sets it on every launch.
struct FFLdsLimit { std::atomic<bool> done[FF_MAX_DEVICES]; };
template <typename K>
int ff_lds_limit_once(K kernel, int bytes, FFLdsLimit* fl) {
  int dev = 0;
  FF_CHECK_HIP(hipGetDevice(&dev));
  const bool track = dev >= 0 && dev < FF_MAX_DEVICES;
  if (!track || !fl->done[dev].load(std::memory_order_acquire)) {
    FF_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    if (track) fl->done[dev].store(true, std::memory_order_release);
  }
  return FF_OK;
}

// ff_dispatch<1, 2, 0>(mode, [&](auto m) { return launch<m>(...); }): calls f with std::integral_constant<int, V> of the
// listed V that equals v.  The call site lists the values it allows -- f is instantiated for exactly those -- and the LAST
// one also takes every other v (the final `return` of the if-ladders this replaces).
template <int V, int... Rest, typename F>
int ff_dispatch(int v, F&& f) {
  if constexpr (sizeof...(Rest) == 0) return f(std::integral_constant<int, V>{});
  else return v == V ? f(std::integral_constant<int, V>{}) : ff_dispatch<Rest...>(v, f);
}

// A selection launch's arguments (PointerArgs, ff_device.h) from its step descriptor (ff_step_io, ff_common.h), checked and filled
// for operator `op`: the logits, the common members (S, mask, kv_len, B, spg, ge_bound, the terminator range) and the feedback
// members -- the next decoder input rows gathered from `memory` with their LayerNorm statistics, and the stop counter with its
// hand-over to the host.  ld_rule: also ldnext >= E (ff_beam_select never had that rule: both wordings are kept).  The caller
// adds `extra` where it has one.  (ff_pointer.hip)
struct PointerArgs;
int ff_step_args(PointerArgs* a, const char* op, bool ld_rule, const ff_step_io& io);

// A launch setting written by a setter (ff_set_gemm_tuning, ...) while other host threads launch: relaxed, like the knob table.
struct FFSetting {
  std::atomic<int> v;
  int get() const { return v.load(std::memory_order_relaxed); }
  int set(int x) { return v.exchange(x, std::memory_order_relaxed); }   // returns the previous value
};

// Partial-tile workspace areas, one per (device, stream): launches on one stream are ordered, launches on different streams
// may overlap and must not share slots.  An area is `ws_bytes` of floats and `slots` zeroed flags, allocated on first use and
// kept for the life of the process.
struct FFStreamAreas {
  const size_t ws_bytes;
  const int slots;
  struct Area { int device; hipStream_t st; float* ws; unsigned int* flags; };
  std::mutex mu;
  std::vector<Area> areas;

  int acquire(hipStream_t st, float** ws, unsigned int** flags) {
    int dev = 0;
    FF_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    for (const Area& a : areas)
      if (a.device == dev && a.st == st) {
        *ws = a.ws; *flags = a.flags;
        return FF_OK;
      }
    Area a{dev, st, nullptr, nullptr};
    FF_CHECK_HIP(hipMalloc(&a.ws, ws_bytes));
    FF_CHECK_HIP(hipMalloc(&a.flags, slots * sizeof(unsigned int)));
    FF_CHECK_HIP(hipMemset(a.flags, 0, slots * sizeof(unsigned int)));
    FF_CHECK_HIP(hipDeviceSynchronize());
    areas.push_back(a);
    *ws = a.ws; *flags = a.flags;
    return FF_OK;
  }
};
