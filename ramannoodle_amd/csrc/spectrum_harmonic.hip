// Entries of the harmonic trajectories (include/rn_harmonic.h; kernel: kernels_harmonic.hip).
//
// The inputs (ref, omega_dt, amp, phase in one packed buffer, and D) are copied into a grow-only device workspace per
// process, under one lock, with blocking copies: they are staged when an entry returns.  The kernel runs on the caller's
// stream (the device entry) or on the null stream (the host entry, whose result lives in an allocation of the call and is
// copied to the host array before it returns).  An event recorded after each kernel is waited for before the next call
// writes the workspace: a kernel still in flight on another stream keeps its inputs.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rn_harmonic.h"
#include "kernels.hpp"
#include "spectrum_common.hpp"

namespace {

using rn_spectrum::DeviceBuffer;
using rn_spectrum::Fit;

thread_local std::string g_error;

int fail(int rc, const char *format, ...) {
  char text[512];
  va_list args;
  va_start(args, format);
  vsnprintf(text, sizeof text, format, args);
  va_end(args);
  g_error = text;
  return rc;
}

std::mutex g_mutex;
int g_device = -1;
DeviceBuffer g_small, g_modes;   // ref [K], omega_dt [M], amp [R][M], phase [R][M]; D [M][K]
hipEvent_t g_done = nullptr;     // after the most recent kernel; under g_mutex, as everything here
bool g_profiling = false;
double g_millis[3] = {0, 0, 0};  // copies to the device, the kernel, the copy to the host

// the HIP-event time of one phase on one stream, while profiling is on
struct Span {
  hipEvent_t a = nullptr, b = nullptr;
  hipStream_t stream = nullptr;
  void begin(hipStream_t st) {
    if (!g_profiling) return;
    stream = st;
    if (hipEventCreate(&a) != hipSuccess) a = nullptr;
    if (hipEventCreate(&b) != hipSuccess) b = nullptr;
    if (a) (void)hipEventRecord(a, stream);
  }
  void end() {
    if (b) (void)hipEventRecord(b, stream);
  }
  double collect() {  // waits for the phase
    float ms = 0.f;
    if (a && b && hipEventSynchronize(b) == hipSuccess) (void)hipEventElapsedTime(&ms, a, b);
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    a = b = nullptr;
    return ms;
  }
};

int64_t first_non_finite(const double *values, int64_t count) {
  for (int64_t i = 0; i < count; ++i)
    if (!std::isfinite(values[i])) return i;
  return -1;
}

int ht_synthesize(int device, const double *ref, const double *D, const double *omega_dt, const double *amp,
                  const double *phase, int32_t N, int32_t M, int32_t R, int64_t T, int64_t t0, double *out, bool to_host,
                  void *stream) {
  if (!ref || !D || !omega_dt || !amp || !phase || !out) return fail(RN_ERR_INVALID_ARGUMENT, "a null pointer");
  if (N < 1 || M < 1 || R < 1 || T < 1)
    return fail(RN_ERR_INVALID_ARGUMENT, "N = %d atoms, M = %d modes, R = %d runs or T = %lld frames is not positive",
                (int)N, (int)M, (int)R, (long long)T);
  const int64_t exact = (int64_t)1 << 53;
  if (t0 < 0 || t0 > exact || T > exact - t0)
    return fail(RN_ERR_INVALID_ARGUMENT, "t0 = %lld with T = %lld frames: the frame indices must lie in [0, 2^53]",
                (long long)t0, (long long)T);
  const int64_t K = (int64_t)3 * N;
  const int64_t workgroups = rn::harmonic_workgroups(K, R, T);
  if (workgroups < 0 || T > INT64_MAX / 8 / K / R)
    return fail(RN_ERR_INVALID_ARGUMENT, "R = %d runs of T = %lld frames of %d atoms exceed the grid (2^31 - 1 workgroups)",
                (int)R, (long long)T, (int)N);
  const struct {
    const char *name;
    const double *values;
    int64_t count;
  } arrays[] = {{"ref", ref, K}, {"D", D, (int64_t)M * K}, {"omega_dt", omega_dt, M}, {"amp", amp, (int64_t)R * M},
                {"phase", phase, (int64_t)R * M}};
  for (const auto &array : arrays) {
    const int64_t bad = first_non_finite(array.values, array.count);
    if (bad >= 0)
      return fail(RN_ERR_INVALID_ARGUMENT, "%s[%lld] = %g is not finite", array.name, (long long)bad, array.values[bad]);
  }

  int devices = 0;
  if (hipGetDeviceCount(&devices) != hipSuccess || device < 0 || device >= devices)
    return fail(RN_ERR_NO_DEVICE, "device %d is not one of the %d GPUs", device, devices);
  if (hipSetDevice(device) != hipSuccess) return fail(RN_ERR_HIP, "hipSetDevice(%d) failed", device);

  std::lock_guard<std::mutex> lock(g_mutex);
  if (g_done && hipEventSynchronize(g_done) != hipSuccess)  // (the last kernel reads the workspace)
    return fail(RN_ERR_HIP, "the previous synthesis failed: %s", hipGetErrorString(hipGetLastError()));
  if (g_device != device) {  // (buffers and the event belong to the device they were made on)
    if (g_device >= 0 && hipSetDevice(g_device) == hipSuccess) {
      g_small.release();
      g_modes.release();
      if (g_done) (void)hipEventDestroy(g_done);
      g_done = nullptr;
      (void)hipSetDevice(device);
    }
    g_device = device;
  }
  if (!g_done && hipEventCreateWithFlags(&g_done, hipEventDisableTiming) != hipSuccess) {
    g_done = nullptr;
    return fail(RN_ERR_HIP, "hipEventCreate failed");
  }

  // ref, omega_dt, amp, phase: one packed copy
  const int64_t rm = (int64_t)R * M;
  std::vector<double> small((size_t)(K + M + 2 * rm));
  std::copy_n(ref, K, small.begin());
  std::copy_n(omega_dt, M, small.begin() + K);
  std::copy_n(amp, rm, small.begin() + K + M);
  std::copy_n(phase, rm, small.begin() + K + M + rm);
  const size_t out_bytes = (size_t)R * (size_t)T * (size_t)K * sizeof(double);
  DeviceBuffer result;  // the host entry's out, freed with the call
  int rc = g_small.ensure(small.size() * sizeof(double), Fit::kGrowOnly);
  if (rc == RN_OK) rc = g_modes.ensure((size_t)M * K * sizeof(double), Fit::kGrowOnly);
  if (rc == RN_OK && to_host) rc = result.ensure(out_bytes);
  if (rc != RN_OK)
    return fail(rc, "no device memory for %d runs of %lld frames of %d atoms and %d modes", (int)R, (long long)T, (int)N,
                (int)M);
  hipError_t e = hipSuccess;
  auto ok = [&](hipError_t status_of_call) {
    if (e == hipSuccess) e = status_of_call;
    return e == hipSuccess;
  };
  const hipStream_t work = to_host ? nullptr : (hipStream_t)stream;
  double *const d_out = to_host ? result.as<double>() : out;
  Span copies, kernel, download;
  for (double &v : g_millis) v = 0.0;
  copies.begin(nullptr);
  ok(hipMemcpy(g_small.ptr, small.data(), small.size() * sizeof(double), hipMemcpyHostToDevice));
  ok(hipMemcpy(g_modes.ptr, D, (size_t)M * K * sizeof(double), hipMemcpyHostToDevice));
  ok(hipStreamSynchronize(nullptr));  // the inputs are in HBM before a kernel on any stream reads them
  copies.end();
  if (e == hipSuccess) {
    const double *d_small = g_small.as<const double>();
    kernel.begin(work);
    rn::launch_harmonic_synthesis(d_small, g_modes.as<const double>(), d_small + K, d_small + K + M, d_small + K + M + rm,
                                  K, M, R, T, t0, d_out, work);
    ok(hipGetLastError());
    kernel.end();
    ok(hipEventRecord(g_done, work));
  }
  if (to_host) {
    download.begin(nullptr);
    ok(hipMemcpy(out, result.ptr, out_bytes, hipMemcpyDeviceToHost));
    download.end();
    ok(hipStreamSynchronize(nullptr));  // (also after a failure: `result` is freed on return)
  }
  if (g_profiling) {
    g_millis[0] = copies.collect();
    g_millis[1] = kernel.collect();
    g_millis[2] = download.collect();
  }
  if (e != hipSuccess) return fail(RN_ERR_HIP, "%s", hipGetErrorString(e));
  return RN_OK;
}

}  // namespace

extern "C" int rn_ht_synthesize(int device, const double *ref, const double *D, const double *omega_dt, const double *amp,
                                const double *phase, int32_t N, int32_t M, int32_t R, int64_t T, int64_t t0, double *out) {
  return ht_synthesize(device, ref, D, omega_dt, amp, phase, N, M, R, T, t0, out, true, nullptr);
}

extern "C" int rn_ht_synthesize_device(int device, const double *ref, const double *D, const double *omega_dt,
                                       const double *amp, const double *phase, int32_t N, int32_t M, int32_t R, int64_t T,
                                       int64_t t0, double *d_out, void *stream) {
  return ht_synthesize(device, ref, D, omega_dt, amp, phase, N, M, R, T, t0, d_out, false, stream);
}

extern "C" int rn_ht_set_profiling(int enabled) {
  std::lock_guard<std::mutex> lock(g_mutex);
  g_profiling = enabled != 0;
  for (double &v : g_millis) v = 0.0;
  return RN_OK;
}

extern "C" int rn_ht_phase_times(double *millis) {
  if (!millis) return RN_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lock(g_mutex);
  std::copy_n(g_millis, 3, millis);
  return RN_OK;
}

extern "C" const char *rn_ht_last_error(void) { return g_error.c_str(); }
