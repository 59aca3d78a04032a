// Private to csrc: the owners of every allocation a handle or a stream holds — device memory (DeviceBuffer<T>) and
// page-locked host words (PinnedBuffer<T>).  No other code of the library calls hipMalloc / hipFree and their host forms
// (bp_host_alloc / bp_host_free, which hand page-locked memory to the caller, excepted).
//
// A buffer belongs to one device and must be freed with that device current: bp_destroy, bp_stream_close and every entry
// point that can grow or replace a buffer set the handle's device before they touch one.
//
// The calls return hipError_t (flac_device.hip has no handle in scope); BP_HIP at a call site turns that into the handle's
// error text and BP_ERR_OUT_OF_MEMORY / BP_ERR_HIP.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>

namespace bp {

// bytes of device memory the DeviceBuffers of this library hold (bp_api.hip defines it; the A/B library exports the count
// as bp_ab_live_device_bytes)
extern std::atomic<int64_t> g_live_device_bytes;

template <class T>
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
    if (this != &o) {
      (void)reset();
      p_ = o.p_, cap_ = o.cap_;
      o.p_ = nullptr, o.cap_ = 0;
    }
    return *this;
  }
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  ~DeviceBuffer() { (void)reset(); }

  operator T*() const { return p_; }
  size_t capacity() const { return cap_; }  // elements of T
  // a byte buffer's contents as the records they are
  template <class U>
  U* as() const {
    static_assert(sizeof(T) == 1, "typed views are for byte buffers");
    return reinterpret_cast<U*>(p_);
  }

  hipError_t reset() {
    if (!p_) return hipSuccess;
    g_live_device_bytes -= (int64_t)bytes();
    const hipError_t e = hipFree(p_);
    p_ = nullptr, cap_ = 0;
    return e;
  }

  // Room for n elements, exactly n when it allocates: grows only, the contents are not kept.  A zero-length request
  // allocates one element.
  hipError_t reserve(size_t n) {
    if (p_ && n <= cap_) return hipSuccess;
    // hipFree waits for the whole device, so work of an earlier call that still reads the old buffer has finished
    hipError_t e = reset();
    if (e != hipSuccess) return e;
    void* p = nullptr;
    if ((e = hipMalloc(&p, (n ? n : 1) * sizeof(T))) != hipSuccess) return e;
    p_ = static_cast<T*>(p), cap_ = n;
    g_live_device_bytes += (int64_t)bytes();
    return hipSuccess;
  }

  // reserve(n), then the n elements at `host` copied in (the host waits); a failed copy leaves the buffer empty
  hipError_t upload(const T* host, size_t n) {
    hipError_t e = reserve(n);
    if (e == hipSuccess && (e = hipMemcpy(p_, host, n * sizeof(T), hipMemcpyHostToDevice)) != hipSuccess) (void)reset();
    return e;
  }

 private:
  size_t bytes() const { return (cap_ ? cap_ : 1) * sizeof(T); }
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// n page-locked elements, allocated once or grown between calls (hipHostMallocPortable): the words a stream's copy or kernel leaves for the host
template <class T>
class PinnedBuffer {
 public:
  PinnedBuffer() = default;
  PinnedBuffer(const PinnedBuffer&) = delete;
  PinnedBuffer& operator=(const PinnedBuffer&) = delete;
  ~PinnedBuffer() {
    if (p_) (void)hipHostFree(p_);
  }
  operator T*() const { return p_; }
  hipError_t alloc(size_t n) {
    void* p = nullptr;
    const hipError_t e = p_ ? hipSuccess : hipHostMalloc(&p, n * sizeof(T), hipHostMallocPortable);
    if (p) p_ = static_cast<T*>(p), cap_ = n;
    return e;
  }
  // Room for n elements: grows only, the contents are not kept (the words of a call whose count the caller chooses).  The
  // stream that wrote the old block must have drained.
  hipError_t reserve(size_t n) {
    if (p_ && n <= cap_) return hipSuccess;
    if (p_) (void)hipHostFree(p_);
    p_ = nullptr, cap_ = 0;
    return alloc(n ? n : 1);
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

}  // namespace bp
