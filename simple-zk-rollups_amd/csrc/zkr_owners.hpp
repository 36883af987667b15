// zkr_owners.hpp -- the four owners of HIP resources: device memory (DevBuf, Dev<T>), pinned host memory (PinnedBuf, Pinned<T>),
// events (ScopedEvent) and streams (OwnStream).  Each frees what it holds when its scope or its struct ends, moves but does not
// copy, and converts to the raw handle, so a launch helper reads `srt.counts` or `sl.ev_w` as it would a plain pointer or event.
// Entry points return early on every failed HIP call; none of those paths may leave a resource behind.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "../../include/zkr.h"

namespace zkr {

void set_error(const char *fmt, ...);
#define ZKR_HIP_CHECK(expr)                                                                 \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess) {                                                                 \
      set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return ZKR_ERR_HIP;                                                                   \
    }                                                                                       \
  } while (0)

// the shape all four share: one raw handle, null when empty; FREE(handle) runs in reset()
template <class H, class Free>
struct Owner {
  H p = nullptr;
  Owner() = default;
  Owner(const Owner &) = delete;
  Owner &operator=(const Owner &) = delete;
  Owner(Owner &&o) noexcept : p(o.release()) {}
  Owner &operator=(Owner &&o) noexcept {
    if (this != &o) { reset(); p = o.release(); }
    return *this;
  }
  ~Owner() { reset(); }
  void reset() {
    if (p) Free()(p);
    p = nullptr;
  }
  H release() { H q = p; p = nullptr; return q; }
  operator H() const { return p; }
};
struct FreeDevice { void operator()(void *p) const { (void)hipFree(p); } };
struct FreePinned { void operator()(void *p) const { (void)hipHostFree(p); } };
struct FreeEvent { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
struct FreeStream { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };

// untyped memory (point tables, bucket sets: G1 or G2 by a run-time flag); `(T *)buf` and buf.as<T>() read it as T
template <class Free>
struct MemBuf : Owner<void *, Free> {
  template <class T> T *as() const { return static_cast<T *>(this->p); }
  template <class T> explicit operator T *() const { return static_cast<T *>(this->p); }
};
struct DevBuf : MemBuf<FreeDevice> {
  int alloc(size_t bytes) { reset(); ZKR_HIP_CHECK(hipMalloc(&p, bytes ? bytes : 1)); return 0; }
};
// a device buffer that held secrets: zeroed, and the zeroing waited for, before it is freed -- however the call is left
struct SecretBuf : DevBuf {  // whose own destructor frees, after this one has run
  size_t bytes = 0;
  hipStream_t s = nullptr;
  ~SecretBuf() {
    if (!p) return;
    (void)hipMemsetAsync(p, 0, bytes, s);
    (void)hipStreamSynchronize(s);
  }
  int alloc(size_t n) { bytes = n; return DevBuf::alloc(n); }
};
struct PinnedBuf : MemBuf<FreePinned> {
  int alloc(size_t bytes) { reset(); ZKR_HIP_CHECK(hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault)); return 0; }
};
// `count` elements of T over either of the two
template <class T, class Buf>
struct Typed {
  Buf buf;
  int alloc(size_t count) { return buf.alloc(count * sizeof(T)); }
  void reset() { buf.reset(); }
  T *release() { return static_cast<T *>(buf.release()); }
  operator T *() const { return static_cast<T *>(buf.p); }
  template <class U> explicit operator U *() const { return static_cast<U *>(buf.p); }  // `(uint8_t *)d_w + bytes`, as with the raw pointer
  T *operator->() const { return static_cast<T *>(buf.p); }
};
template <class T> using Dev = Typed<T, DevBuf>;
template <class T> using Pinned = Typed<T, PinnedBuf>;

struct ScopedEvent : Owner<hipEvent_t, FreeEvent> {
  int create(unsigned flags = hipEventDefault) { reset(); ZKR_HIP_CHECK(hipEventCreateWithFlags(&p, flags)); return 0; }  // every long-lived event here: hipEventDisableTiming
};
struct OwnStream : Owner<hipStream_t, FreeStream> {
  int create(unsigned flags = hipStreamNonBlocking) { reset(); ZKR_HIP_CHECK(hipStreamCreateWithFlags(&p, flags)); return 0; }
};

}  // namespace zkr
