// The host runtime of the entries that keep their state per process, not per handle: the line-shape and multi-peak fits
// (lineshape.hip, peakfit.hip, through fit_entry.hpp), the covariance moments (spectrum_covariance.hip), the harmonic
// trajectories (spectrum_harmonic.hip) and the band moments (spectrum_band.hip); and the holders every spectrum reducer
// uses (DeviceBuffer, Fit, Source, PhaseTimer; spectrum_common.hpp and spectrum_segment_core.hpp include this file).
// Host code only: no kernels, no hipFFT.  host_runtime.hpp is the other host runtime, of the entries that take a
// handle (the evaluator and the interpolation model): exceptions, owned streams, the error text in the handle.
//
// The rules of an entry file built on this one:
//  * Status and text.  An entry returns an rn_potgnn.h status; a refusal or failure leaves its text in the file's own
//    `thread_local ErrorText`, which the module's rn_*_last_error returns: per module and per thread.
//  * Order.  The argument checks come first and touch no device; then select_device; then, for a device entry of the
//    MD reducers' kind, Source::wait on the producer's stream; then the lock.
//  * Workspace.  The device arrays of a module live in DeviceBuffers of the file, registered with one Workspace, whose
//    mutex is held from bind() to the return.  They belong to one device at a time: bind() releases them when the
//    device changes.  A buffer that a `workspace_limit` counts is sized with Fit::kExact, so that a later call never
//    holds more than its limit; every other buffer with Fit::kGrowOnly.
//  * HIP errors.  After the allocations every HIP call goes through one FirstError; the work that follows a failure is
//    skipped, the closing wait is not (the buffers may be in use), and the first error's string becomes the text.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rn_potgnn.h"

namespace rn_spectrum {

// the text of a thread's most recent refusal or failure in one module
struct ErrorText {
  std::string text;
  int fail(int rc, const char *format, ...) {
    char buffer[512];
    va_list args;
    va_start(args, format);
    vsnprintf(buffer, sizeof buffer, format, args);
    va_end(args);
    text = buffer;
    return rc;
  }
};

inline int select_device(int device, ErrorText &error) {
  int devices = 0;
  if (hipGetDeviceCount(&devices) != hipSuccess || device < 0 || device >= devices)
    return error.fail(RN_ERR_NO_DEVICE, "device %d is not one of the %d GPUs", device, devices);
  if (hipSetDevice(device) != hipSuccess) return error.fail(RN_ERR_HIP, "hipSetDevice(%d) failed", device);
  return RN_OK;
}

// the first HIP error of a call: ok(hipCall(...)) is false from the first failure on
struct FirstError {
  hipError_t first = hipSuccess;
  bool operator()(hipError_t status) {
    if (first == hipSuccess) first = status;
    return first == hipSuccess;
  }
};

inline int64_t first_non_finite(const double *values, int64_t count) {  // its index, or -1
  for (int64_t i = 0; i < count; ++i)
    if (!std::isfinite(values[i])) return i;
  return -1;
}

enum class Fit { kExact, kGrowOnly };  // which rule applies to which buffer: see the head of this file

// a device allocation, freed with its holder
struct DeviceBuffer {
  void *ptr = nullptr;
  size_t bytes = 0;
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer &) = delete;
  DeviceBuffer &operator=(const DeviceBuffer &) = delete;
  ~DeviceBuffer() { release(); }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    bytes = 0;
  }
  int ensure(size_t want, Fit fit = Fit::kExact) {
    if (ptr && (fit == Fit::kExact ? bytes == want : bytes >= want)) return RN_OK;
    release();
    if (hipMalloc(&ptr, want) != hipSuccess) {
      ptr = nullptr;
      return RN_ERR_OUT_OF_MEMORY;
    }
    bytes = want;
    return RN_OK;
  }
  template <class T>
  T *as() const {
    return static_cast<T *>(ptr);
  }
};

// The device arrays of one module: its mutex, the device they are on and the buffers themselves (declared before it in
// the file).  The caller selects the device, locks `mutex` for the rest of the call and binds.
struct Workspace {
  std::mutex mutex;
  int device = -1;
  std::vector<DeviceBuffer *> buffers;
  Workspace(std::initializer_list<DeviceBuffer *> list) : buffers(list) {}
  // Buffers belong to the device they were allocated on: on a change they are released there, with whatever else
  // `also_release` frees.  When switching back to the old device fails nothing is released.
  template <class AlsoRelease>
  void bind(int to, AlsoRelease also_release) {
    if (device == to) return;
    if (device >= 0 && hipSetDevice(device) == hipSuccess) {
      for (DeviceBuffer *buffer : buffers) buffer->release();
      also_release();
      (void)hipSetDevice(to);
    }
    device = to;
  }
  void bind(int to) {
    bind(to, [] {});
  }
};

// Where a call's time series is: a host array (staged into the entry's buffer, outside the workspace accounting), or
// HBM, written by work on `stream`.  All reduction work runs on the null stream, so the producer's stream is
// synchronised first.
struct Source {
  const double *data;
  bool on_host;
  void *stream;
  static Source host(const double *data) { return {data, true, nullptr}; }
  static Source device(const double *data, void *stream) { return {data, false, stream}; }
  int wait() const {
    return !on_host && stream && hipStreamSynchronize((hipStream_t)stream) != hipSuccess ? RN_ERR_HIP : RN_OK;
  }
  int on_device(DeviceBuffer &staging, size_t bytes, const double **d_data) const {
    *d_data = data;
    if (!on_host) return RN_OK;
    if (int rc = staging.ensure(bytes, Fit::kGrowOnly)) return rc;
    *d_data = staging.as<const double>();
    return hipMemcpy(staging.ptr, data, bytes, hipMemcpyHostToDevice) == hipSuccess ? RN_OK : RN_ERR_HIP;
  }
};

// HIP-event times of the phases of a module's most recent call (the segment reducers: builder, forward FFTs, power
// kernel, back half), kept only while profiling is on; one per module, under its mutex.  A phase lasts from its mark to
// the next mark or close, on the stream of its mark, because run_segments launches the transforms and the back half
// itself.  A reducer that launches everything itself (the VDOS) marks all the same: on one stream, with nothing between
// the end of a phase and the next mark, that is the span of a begin / end pair plus one event.
struct PhaseTimer {
  struct Span {
    int phase;
    hipStream_t stream;
    hipEvent_t a, b;
  };
  bool enabled = false;
  std::vector<double> millis;  // what phase_times writes: a module's *_phase_times array has as many doubles
  std::vector<Span> spans;
  bool open = false;
  explicit PhaseTimer(int phases = 4) : millis((size_t)phases, 0.0) {}
  void close() {
    if (enabled && open) (void)hipEventRecord(spans.back().b, spans.back().stream);
    open = false;
  }
  void mark(int phase, hipStream_t stream = nullptr) {
    if (!enabled) return;
    close();
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess) return;
    if (hipEventCreate(&b) != hipSuccess) {
      (void)hipEventDestroy(a);
      return;
    }
    (void)hipEventRecord(a, stream);
    spans.push_back({phase, stream, a, b});
    open = true;
  }
  void reset() {
    for (double &v : millis) v = 0.0;
  }
  void collect() {  // after the call's last copy to the host; while profiling is on it waits for the device
    if (!enabled) return;
    close();
    (void)hipDeviceSynchronize();
    for (Span &s : spans) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) millis[(size_t)s.phase] += ms;
      (void)hipEventDestroy(s.a);
      (void)hipEventDestroy(s.b);
    }
    spans.clear();
  }
  // the bodies of a module's two extern "C" profiling entries
  int set_profiling(std::mutex &mutex, int on) {
    std::lock_guard<std::mutex> lock(mutex);
    enabled = on != 0;
    reset();
    return RN_OK;
  }
  int phase_times(std::mutex &mutex, double *out) {
    if (!out) return RN_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(mutex);
    std::copy(millis.begin(), millis.end(), out);
    return RN_OK;
  }
};

}  // namespace rn_spectrum
