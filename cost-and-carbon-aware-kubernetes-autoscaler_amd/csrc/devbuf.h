// devbuf.h — DevBuf<T>: the owner of one device allocation of libccka.so.
//
// Pointer and element count travel together and the destructor frees, so a
// context's buffers need no free list. Sizes are elements of T. A reallocation
// does not keep the contents. Move-only.
#pragma once
#include <cstddef>
#include <cstdint>

namespace ccka {

// The default allocator (hipMalloc / hipFree), defined at the end of this
// header unless CCKA_DEVBUF_NO_HIP is set (the CPU test's allocator instead).
struct HipAlloc;

template <class T, class Alloc = HipAlloc>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p_ = o.p_; n_ = o.n_;
      o.p_ = nullptr; o.n_ = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  int64_t count() const { return n_; }

  void release() {
    if (p_) Alloc::free(p_);
    p_ = nullptr;
    n_ = 0;
  }
  // grow-only: at least n elements (the allocation is kept when it holds them)
  bool reserve(int64_t n) { return (n >= 0 && n <= n_) || fresh(n); }
  // exact: n elements (the allocation is kept only when it has that size)
  bool resize(int64_t n) { return n == n_ || fresh(n); }

 private:
  // empty on n == 0 (success) and on every failure: a negative n, a byte count
  // beyond size_t (refused before the allocator sees it), no memory
  bool fresh(int64_t n) {
    release();
    if (n == 0) return true;
    if (n < 0 || (uint64_t)n > SIZE_MAX / sizeof(T)) return false;
    p_ = static_cast<T*>(Alloc::alloc((size_t)n * sizeof(T)));
    if (!p_) return false;
    n_ = n;
    return true;
  }
  T* p_ = nullptr;
  int64_t n_ = 0;
};

// Buffers that are sized together: `ok` is the && of their reserve / resize
// calls; a failure of one empties them all.
template <class... B>
bool all_or_none(bool ok, B&... bufs) {
  if (!ok) (bufs.release(), ...);
  return ok;
}

}  // namespace ccka

#ifndef CCKA_DEVBUF_NO_HIP
#include <hip/hip_runtime.h>
namespace ccka {
struct HipAlloc {
  static void* alloc(size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes) == hipSuccess) return p;
    (void)hipGetLastError();  // the failure is reported by the return value, not left sticky
    return nullptr;
  }
  static void free(void* p) { (void)hipFree(p); }
};
}  // namespace ccka
#endif
