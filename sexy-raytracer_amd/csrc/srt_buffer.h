// srt_buffer.h -- device memory that frees itself: the context's cached work areas, the scene's arrays and the
// temporaries of the entry points (srt_api.cpp and the other host files).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

class DeviceBuffer {  // move-only
 public:
  DeviceBuffer() = default;
  DeviceBuffer(DeviceBuffer&& o) noexcept { swap(o); }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
    swap(o);
    return *this;
  }
  ~DeviceBuffer() {
    if (p_) (void)hipFree(p_);
  }

  // Grow-only: a buffer that holds `bytes` already is kept; otherwise it is freed and `bytes` are allocated.  After a
  // failure the buffer is empty.
  hipError_t reserve(size_t bytes) {
    if (bytes <= bytes_) return hipSuccess;
    *this = DeviceBuffer();
    const hipError_t e = hipMalloc(&p_, bytes);
    if (e == hipSuccess) bytes_ = bytes; else p_ = nullptr;
    return e;
  }

  template <typename T = void>
  T* get() const { return static_cast<T*>(p_); }
  size_t bytes() const { return bytes_; }

 private:
  void swap(DeviceBuffer& o) noexcept {
    std::swap(p_, o.p_);
    std::swap(bytes_, o.bytes_);
  }
  void* p_ = nullptr;
  size_t bytes_ = 0;
};
