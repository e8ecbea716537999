// The one owner of a device allocation: hipMalloc in alloc / upload, hipFree in release and the destructor.  Move-only (a copy would free twice).
// Host-only; the kernels' argument structs stay plain pointers, filled from `.ptr`.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <utility>

namespace pt {

template <typename T>
struct DevBuf
{
  T*     ptr   = nullptr;
  size_t count = 0;

  DevBuf() = default;
  DevBuf(const DevBuf&)            = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : ptr(std::exchange(o.ptr, nullptr)), count(std::exchange(o.count, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept
  {
    if(this != &o)
    {
      release();
      ptr   = std::exchange(o.ptr, nullptr);
      count = std::exchange(o.count, 0);
    }
    return *this;
  }
  ~DevBuf() { release(); }

  // n elements, uninitialised; what was held is released first.  n == 0 and a failed allocation both leave the buffer empty.
  hipError_t alloc(size_t n)
  {
    release();
    if(n == 0)
      return hipSuccess;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&ptr), n * sizeof(T));
    if(e == hipSuccess)
      count = n;
    else
      ptr = nullptr;
    return e;
  }
  hipError_t upload(const T* src, size_t n)
  {
    const hipError_t e = alloc(n);
    if(e != hipSuccess || n == 0)
      return e;
    return hipMemcpy(ptr, src, n * sizeof(T), hipMemcpyHostToDevice);
  }
  void release()
  {
    if(ptr)
      (void)hipFree(ptr);
    ptr   = nullptr;
    count = 0;
  }
  uint64_t bytes() const { return uint64_t(count) * sizeof(T); }
};

}  // namespace pt
