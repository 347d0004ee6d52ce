// cld_owned.h -- what a runtime context owns on a GPU, released by construction:
// growable device / pinned-host buffers, streams and events.  A context
// declares its streams and events before its buffers, so the buffers are freed
// first and the streams and events destroyed after them.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <algorithm>

#include "cld_mi355x.h"

namespace cld {

enum class Mem {
  Device,        // hipMalloc
  Pinned,        // hipHostMalloc, default flags
  PinnedMapped,  // hipHostMalloc, coherent and mapped: the GPU writes it while the host polls
};

// A buffer of T: the pointer, its capacity in elements, and the hipFree /
// hipHostFree at the end.  Reads as the pointer it holds.
template <class T, Mem M = Mem::Device>
class Buf {
 public:
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { release(); }

  // Room for n elements.  Enough already: nothing happens.  Otherwise the
  // old block is freed and max(n, 1.5 x capacity) elements are allocated: the
  // contents are NOT kept.  On failure the buffer is empty (null, capacity 0)
  // and CLD_ENOMEM comes back; a caller may retry with less.
  int reserve(size_t n) {
    if (cap_ >= n) return CLD_OK;
    const size_t want = std::max(n, cap_ * 3 / 2);
    release();
    constexpr unsigned kFlags = M == Mem::Pinned ? hipHostMallocDefault : hipHostMallocCoherent | hipHostMallocMapped;
    const hipError_t e = M == Mem::Device ? hipMalloc((void**)&p_, want * sizeof(T))
                                          : hipHostMalloc((void**)&p_, want * sizeof(T), kFlags);
    if (e != hipSuccess) {
      p_ = nullptr;
      return CLD_ENOMEM;
    }
    cap_ = want;
    return CLD_OK;
  }
  void release() {
    if (p_) (void)(M == Mem::Device ? hipFree(p_) : hipHostFree(p_));
    p_ = nullptr;
    cap_ = 0;
  }
  operator T*() const { return p_; }
  size_t capacity() const { return cap_; }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// A stream or an event, made by its owner (hipStreamCreate*(&s.h), hipEventCreate*(&e.h)) and destroyed with it.
template <class H, hipError_t (*Destroy)(H)>
struct Handle {
  H h = nullptr;
  Handle() = default;
  Handle(const Handle&) = delete;
  Handle& operator=(const Handle&) = delete;
  ~Handle() { if (h) (void)Destroy(h); }
  operator H() const { return h; }
};
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventDestroy>;

}  // namespace cld
