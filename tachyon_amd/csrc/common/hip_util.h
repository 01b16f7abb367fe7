// Small HIP runtime helpers shared by the drivers.
// (The reference's thin runtime layer is tachyon/device/gpu/: gpuStream /
// gpuMemPool aliases, GpuMemory RAII, GpuPointerGetAttributes.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "sections.h"

namespace tachyon_amd {

[[noreturn]] inline void hip_fail(hipError_t e, const char* what, const char* file, int line) {
  char buf[512];
  snprintf(buf, sizeof buf, "tachyon_mi355x: HIP error '%s' (%d) in %s at %s:%d", hipGetErrorString(e),
           (int)e, what, file, line);
  throw std::runtime_error(buf);
}

#define TA_HIP(expr)                                                \
  do {                                                              \
    hipError_t _e = (expr);                                         \
    if (_e != hipSuccess) ::tachyon_amd::hip_fail(_e, #expr, __FILE__, __LINE__); \
  } while (0)

// Device-resident scratch that only grows; reused across calls so the hot path
// never allocates (allocation is not capturable and costs ~100 us at GB sizes).
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  ~DeviceBuffer() { release(); }

  void* ensure(size_t bytes) {
    if (bytes > cap_) {
      release();
      size_t want = bytes < 256 ? 256 : bytes;
      TA_HIP(hipMalloc(&ptr_, want));
      cap_ = want;
    }
    return ptr_;
  }
  template <class T>
  T* as() const { return static_cast<T*>(ptr_); }
  size_t capacity() const { return cap_; }
  void release() {
    if (ptr_) (void)hipFree(ptr_);
    ptr_ = nullptr;
    cap_ = 0;
  }

 private:
  void* ptr_ = nullptr;
  size_t cap_ = 0;
};

// True if `p` is device (or managed) memory visible to the current device --
// the analogue of the reference's GpuPointerGetAttributes check
// (icicle_msm_bn254_g1.cc:37-45).
inline bool is_device_pointer(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t attr;
  hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return attr.type == hipMemoryTypeDevice || attr.isManaged;
}

// The device that owns `p` (device or managed memory), or -1 for host memory.
inline int pointer_device(const void* p) {
  if (!p) return -1;
  hipPointerAttribute_t attr;
  hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  return (attr.type == hipMemoryTypeDevice || attr.isManaged) ? attr.device : -1;
}

inline unsigned ceil_div(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }

inline void require_gpu() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0)
    throw std::runtime_error("tachyon_mi355x: no HIP device available (the MI355X backend has no CPU fallback)");
}

// True for a pointer the Fr kernels can use in place: device memory on a
// 16-byte boundary (anything else is staged)
inline bool usable_in_place(const void* p) { return is_device_pointer(p) && ((uintptr_t)p & 15) == 0; }

struct OwnedStream {
  hipStream_t s = nullptr;
  OwnedStream() { TA_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
  OwnedStream(const OwnedStream&) = delete;
  OwnedStream& operator=(const OwnedStream&) = delete;
  ~OwnedStream() { (void)hipStreamDestroy(s); }
};

// Runs f; if it throws, the stream is drained first, so that nothing of the
// caller's stays in flight
template <class Fn>
void drained_on_throw(hipStream_t stream, Fn&& f) {
  try {
    f();
  } catch (...) {
    (void)hipStreamSynchronize(stream);
    throw;
  }
}

// Device views of `count` columns of lens[i] elements each: the pointer itself
// where it is usable in place, else a copy in `buf`, enqueued on `stream` --
// each distinct column once, so equal columns have equal views.  An empty
// column's view is null.  The copies are valid until buf's next use.
template <class T>
std::vector<T*> stage_columns(T* const* ptrs, const size_t* lens, size_t count, DeviceBuffer& buf,
                              hipStream_t stream) {
  using Elem = std::remove_const_t<T>;
  std::map<std::pair<T*, size_t>, T*> view;  // null: to be copied
  size_t total = 0;
  for (size_t i = 0; i < count; ++i) {
    if (!lens[i]) continue;
    const auto [it, fresh] = view.emplace(std::make_pair(ptrs[i], lens[i]), nullptr);
    if (!fresh) continue;
    if (usable_in_place(ptrs[i])) it->second = ptrs[i];
    else total += lens[i];
  }
  Elem* d = total ? static_cast<Elem*>(buf.ensure(total * sizeof(Elem))) : nullptr;
  std::vector<T*> dev(count, nullptr);
  for (size_t i = 0; i < count; ++i) {
    if (!lens[i]) continue;
    T*& v = view[{ptrs[i], lens[i]}];
    if (!v) {
      TA_HIP(hipMemcpyAsync(d, ptrs[i], lens[i] * sizeof(Elem), hipMemcpyDefault, stream));
      v = d;
      d += lens[i];
    }
    dev[i] = v;
  }
  return dev;
}

// The packer's image into `buf`, enqueued on `stream` (the packer keeps the
// host side alive); returns the device address
inline unsigned char* upload_image(const SectionPacker& image, DeviceBuffer& buf, hipStream_t stream) {
  const size_t bytes = image.size() ? image.size() : 1;
  unsigned char* d = static_cast<unsigned char*>(buf.ensure(bytes));
  TA_HIP(hipMemcpyAsync(d, image.data(), bytes, hipMemcpyHostToDevice, stream));
  return d;
}

// Stream-event spans of one call, summed by phase
class PhaseClock {
 public:
  explicit PhaseClock(hipStream_t stream) : stream_(stream) {}
  PhaseClock(const PhaseClock&) = delete;
  PhaseClock& operator=(const PhaseClock&) = delete;
  ~PhaseClock() {
    for (Span& s : spans_) {
      if (s.a) (void)hipEventDestroy(s.a);
      if (s.b) (void)hipEventDestroy(s.b);
    }
  }
  void begin(int phase) {
    spans_.push_back({phase, nullptr, nullptr});
    TA_HIP(hipEventCreate(&spans_.back().a));
    TA_HIP(hipEventRecord(spans_.back().a, stream_));
  }
  void end() {
    TA_HIP(hipEventCreate(&spans_.back().b));
    TA_HIP(hipEventRecord(spans_.back().b, stream_));
  }
  // ms[phase] += the phase's spans, for the phases < count; after the stream
  // is synchronised
  void sum(float* ms, int count) const {
    for (const Span& s : spans_) {
      float t = 0.f;
      if (s.phase < count && s.a && s.b && hipEventElapsedTime(&t, s.a, s.b) == hipSuccess) ms[s.phase] += t;
    }
  }

 private:
  struct Span {
    int phase;
    hipEvent_t a, b;
  };
  hipStream_t stream_;
  std::vector<Span> spans_;
};

}  // namespace tachyon_amd
