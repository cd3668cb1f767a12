// zb_hostbuf.hpp — the owning buffers of the host side (zb_engine.hip): DevBuf<T> is device memory, PinBuf<T> pinned
// host memory. A buffer knows its capacity and frees itself, so an engine member needs no entry in a free list and a
// failed growth leaves an empty buffer, never a capacity without memory behind it. Host only: kernels get the raw
// pointer (the implicit conversion).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <utility>

#include "zb_checked.hpp"

namespace zbg {

// what a growing buffer allocates for a request of n elements: max(n + n / div + add, floor) (div 0: no share of n)
struct Growth {
  size_t div = 0, add = 0, floor = 0;
  size_t of(size_t n) const { return std::max(n + (div ? n / div : 0) + add, floor); }
};

struct DevMem {  // (the guard-band build names the buffer and the caller's line, as its hipMalloc macro does)
  static hipError_t alloc(void** p, size_t bytes, const char* name, const char* file, int line) {
#ifdef ZB_CHECKED
    return checked_malloc(p, bytes, name, file, line);
#else
    return hipMalloc(p, bytes);
#endif
  }
  static void release(void* p) {
#ifdef ZB_CHECKED
    (void)checked_free(p);
#else
    (void)hipFree(p);
#endif
  }
};
struct PinMem {
  static hipError_t alloc(void** p, size_t bytes, const char*, const char*, int) { return hipHostMalloc(p, bytes); }
  static void release(void* p) { (void)hipHostFree(p); }
};

template <class T, class Mem>
class OwnedBuf {
 public:
  // pad: elements allocated past the capacity (the scan scratches keep 16 spare bytes)
  OwnedBuf(const char* name, size_t pad = 0) : name_(name), pad_(pad) {}
  OwnedBuf(const OwnedBuf&) = delete;
  OwnedBuf& operator=(const OwnedBuf&) = delete;
  ~OwnedBuf() { reset(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  T* operator->() const { return p_; }
  size_t cap() const { return cap_; }  // elements
  const char* name() const { return name_; }

  void reset() {
    if (p_) Mem::release(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  void swap(OwnedBuf& o) {
    std::swap(p_, o.p_);
    std::swap(cap_, o.cap_);
  }

  // A buffer of exactly n elements in place of the old one, whatever that held: the stream is synchronised first
  // (queued work may still use the old buffer), contents are not kept. For the members of a group that shares one
  // capacity test; everything else calls reserve.
  hipError_t renew(hipStream_t s, size_t n, const char* file = __builtin_FILE(), int line = __builtin_LINE()) {
    hipError_t r = hipStreamSynchronize(s);
    if (r != hipSuccess) return r;
    reset();
    void* q = nullptr;
    r = Mem::alloc(&q, (n + pad_) * sizeof(T), name_, file, line);
    if (r != hipSuccess) return r;
    p_ = (T*)q;
    cap_ = n;
    return hipSuccess;
  }
  // room for n elements: nothing when the buffer holds them, else a new buffer of g.of(n)
  hipError_t reserve(hipStream_t s, size_t n, Growth g = {}, const char* file = __builtin_FILE(),
                     int line = __builtin_LINE()) {
    if (n <= cap_ && p_) return hipSuccess;
    return renew(s, g.of(n), file, line);
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
  const char* name_;
  size_t pad_;
};

template <class T>
using DevBuf = OwnedBuf<T, DevMem>;
template <class T>
using PinBuf = OwnedBuf<T, PinMem>;

}  // namespace zbg
