// Host-only: the owner of one block of GPU or pinned memory (a context's
// buffers, api.hip; a call's scratch). A pointer and its capacity in elements,
// freed once by the destructor, never copied. It converts to T*, so kernel
// launches and copies read as they would with a raw pointer.
//
// The rule of grow(c, count): count <= capacity changes nothing. Otherwise the
// capacity drops to 0, the old block is freed and max(count, 1) elements are
// allocated; contents are not carried over. A failed allocation leaves the
// buffer empty with capacity 0, sets c->err to the policy's message and
// returns MANTIS_ERR_OOM. alloc(c, count) is the same without the first
// sentence (a buffer several others are sized with: their common quantity is
// the caller's condition).
//
// The allocate / free pair is the policy A: hipMalloc / hipFree and
// hipHostMalloc / hipHostFree in api.hip, counting malloc / free in
// tools/bufcheck_main.cpp.
#pragma once
#include <cstddef>

#include "../../include/mantis.h"

namespace mk {

template <class T, class A>
class Buf {
 public:
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { release(); }

  operator T*() const { return p_; }
  T* get() const { return p_; }
  size_t capacity() const { return cap_; }

  void release() {
    cap_ = 0;
    if (p_) A::free(p_);
    p_ = nullptr;
  }
  template <class C>
  mantis_status alloc(C* c, size_t count) {
    release();
    p_ = (T*)A::alloc(sizeof(T) * (count ? count : 1));
    if (!p_) {
      c->err = A::kFailed;
      return MANTIS_ERR_OOM;
    }
    cap_ = count;
    return MANTIS_OK;
  }
  template <class C>
  mantis_status grow(C* c, size_t count) {
    return count <= cap_ ? MANTIS_OK : alloc(c, count);
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

}  // namespace mk
