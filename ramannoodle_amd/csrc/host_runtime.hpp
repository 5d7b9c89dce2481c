// What a translation unit that owns device handles needs on the host: the error types thrown below the C ABI, the owners
// of device memory, streams, events and page-locked memory, and the guard every entry runs in.  Host only.
//
// A handle type H gives set_error() and guarded(): `lock` (a std::recursive_mutex), `error` (a std::string),
// `int device_index() const` (the device the handle lives on) and `static std::string &create_error()` (the text kept for
// a null handle -- a failed create -- one string per handle type).  With a null handle name the type:
// set_error<rn_potgnn>(nullptr, ...).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <exception>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <utility>

#include "../../include/rn_potgnn.h"

namespace rn {

struct HipError {
  hipError_t code;
  const char *what;
};
struct RnInvalid {};  // an argument found invalid inside guarded() (the error text is already set)

#define HIP_TRY(expr)                                       \
  do {                                                      \
    hipError_t _e = (expr);                                 \
    if (_e != hipSuccess) throw ::rn::HipError{_e, #expr};  \
  } while (0)

struct DeviceBuf {
  void *p = nullptr;
  size_t bytes = 0;
  ~DeviceBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  void ensure(size_t n) {  // grow-only
    if (n <= bytes) return;
    release();
    HIP_TRY(hipMalloc(&p, n));
    bytes = n;
  }
  void upload(const void *src, size_t n) {
    ensure(n);
    HIP_TRY(hipMemcpy(p, src, n, hipMemcpyHostToDevice));
  }
  template <typename T>
  T *as() const { return reinterpret_cast<T *>(p); }
};

// Owners of a stream, an event (no timing) and a page-locked host buffer: created on first get() / ensure(), released by
// the destructor, move-only.  `s` / `e` / `p` read what there is without creating it (null before the first use).
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(Stream &&o) noexcept : s(o.s) { o.s = nullptr; }
  Stream &operator=(Stream &&o) noexcept { std::swap(s, o.s); return *this; }
  ~Stream() { if (s) (void)hipStreamDestroy(s); }
  hipStream_t get() {  // non-blocking with respect to the null stream
    if (!s) HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    return s;
  }
};
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
  Event &operator=(Event &&o) noexcept { std::swap(e, o.e); return *this; }
  ~Event() { if (e) (void)hipEventDestroy(e); }
  hipEvent_t get() {
    if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return e;
  }
};
struct PinnedBuf {
  void *p = nullptr;
  size_t bytes = 0;
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
  PinnedBuf &operator=(PinnedBuf &&o) noexcept { std::swap(p, o.p), std::swap(bytes, o.bytes); return *this; }
  ~PinnedBuf() { release(); }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
  }
  void ensure(size_t n) {  // grow-only; the contents do not survive growing
    if (n <= bytes) return;
    release();
    HIP_TRY(hipHostMalloc(&p, n, hipHostMallocDefault));
    bytes = n;
  }
  template <typename T>
  T *as() const { return reinterpret_cast<T *>(p); }
};

inline bool all_finite(const double *v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

template <class H>
void set_error(H *h, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (h) {  // (entry points report argument errors before they enter guarded(): the error text is handle state too)
    std::lock_guard<std::recursive_mutex> hold(h->lock);
    h->error = buf;
  } else {
    H::create_error() = buf;
  }
}

// Every entry point that touches a handle runs inside guarded(): calls on ONE handle are serialised by the handle's own
// lock (they share its workspaces, streams and tape), so a handle may be used from several threads; distinct handles are
// independent.  No exception leaves the C ABI.
template <class H>
int guarded(H *h, const std::function<void()> &fn) {
  std::unique_lock<std::recursive_mutex> lock;
  if (h) lock = std::unique_lock<std::recursive_mutex>(h->lock);
  try {
    if (h) HIP_TRY(hipSetDevice(h->device_index()));
    fn();
    return RN_OK;
  } catch (const RnInvalid &) {
    return RN_ERR_INVALID_ARGUMENT;
  } catch (const HipError &e) {
    set_error(h, "HIP error %d (%s) in %s", (int)e.code, hipGetErrorString(e.code), e.what);
    return e.code == hipErrorOutOfMemory ? RN_ERR_OUT_OF_MEMORY : RN_ERR_HIP;
  } catch (const std::bad_alloc &) {
    set_error(h, "host allocation failed");
    return RN_ERR_OUT_OF_MEMORY;
  } catch (const std::exception &e) {
    set_error(h, "internal error: %s", e.what());
    return RN_ERR_HIP;
  } catch (...) {
    set_error(h, "internal error: unknown exception");
    return RN_ERR_HIP;
  }
}

}  // namespace rn
