// Entries of the harmonic trajectories (include/rn_harmonic.h; kernel: kernels_harmonic.hip).
//
// The workspace (entry_runtime.hpp) holds the inputs, grow-only: ref, omega_dt, amp and phase in one packed buffer, and
// D, copied with blocking copies, so they are staged when an entry returns.  The kernel runs on the caller's stream (the
// device entry, which does not wait for it unless profiling is on) or on the null stream (the host entry, whose result
// lives in an allocation of the call and is copied to the host array before it returns).  An event recorded after each
// kernel is waited for before the next call writes the workspace: a kernel still in flight on another stream keeps its
// inputs.
#include <cstdint>
#include <mutex>
#include <vector>

#include "../../include/rn_harmonic.h"
#include "entry_runtime.hpp"
#include "kernels.hpp"

namespace {

using rn_spectrum::DeviceBuffer;
using rn_spectrum::Fit;

thread_local rn_spectrum::ErrorText g_error;
DeviceBuffer g_small, g_modes;   // ref [K], omega_dt [M], amp [R][M], phase [R][M]; D [M][K]
rn_spectrum::Workspace g_workspace{&g_small, &g_modes};
hipEvent_t g_done = nullptr;     // after the most recent kernel; under the workspace's mutex, as everything here
rn_spectrum::PhaseTimer g_timer(3);  // copies to the device, the kernel, the copy to the host (millis[3] of rn_harmonic.h)

int ht_synthesize(int device, const double *ref, const double *D, const double *omega_dt, const double *amp,
                  const double *phase, int32_t N, int32_t M, int32_t R, int64_t T, int64_t t0, double *out, bool to_host,
                  void *stream) {
  if (!ref || !D || !omega_dt || !amp || !phase || !out) return g_error.fail(RN_ERR_INVALID_ARGUMENT, "a null pointer");
  if (N < 1 || M < 1 || R < 1 || T < 1)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT,
                        "N = %d atoms, M = %d modes, R = %d runs or T = %lld frames is not positive", (int)N, (int)M, (int)R,
                        (long long)T);
  const int64_t exact = (int64_t)1 << 53;
  if (t0 < 0 || t0 > exact || T > exact - t0)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT,
                        "t0 = %lld with T = %lld frames: the frame indices must lie in [0, 2^53]", (long long)t0, (long long)T);
  const int64_t K = (int64_t)3 * N;
  const int64_t workgroups = rn::harmonic_workgroups(K, R, T);
  if (workgroups < 0 || T > INT64_MAX / 8 / K / R)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT,
                        "R = %d runs of T = %lld frames of %d atoms exceed the grid (2^31 - 1 workgroups)", (int)R,
                        (long long)T, (int)N);
  const struct {
    const char *name;
    const double *values;
    int64_t count;
  } arrays[] = {{"ref", ref, K}, {"D", D, (int64_t)M * K}, {"omega_dt", omega_dt, M}, {"amp", amp, (int64_t)R * M},
                {"phase", phase, (int64_t)R * M}};
  for (const auto &array : arrays) {
    const int64_t bad = rn_spectrum::first_non_finite(array.values, array.count);
    if (bad >= 0)
      return g_error.fail(RN_ERR_INVALID_ARGUMENT, "%s[%lld] = %g is not finite", array.name, (long long)bad,
                          array.values[bad]);
  }

  if (int rc = rn_spectrum::select_device(device, g_error)) return rc;

  std::lock_guard<std::mutex> lock(g_workspace.mutex);
  if (g_done && hipEventSynchronize(g_done) != hipSuccess)  // (the last kernel reads the workspace)
    return g_error.fail(RN_ERR_HIP, "the previous synthesis failed: %s", hipGetErrorString(hipGetLastError()));
  g_workspace.bind(device, [] {  // (the event belongs to the device it was made on, as the buffers do)
    if (g_done) (void)hipEventDestroy(g_done);
    g_done = nullptr;
  });
  if (!g_done && hipEventCreateWithFlags(&g_done, hipEventDisableTiming) != hipSuccess) {
    g_done = nullptr;
    return g_error.fail(RN_ERR_HIP, "hipEventCreate failed");
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
    return g_error.fail(rc, "no device memory for %d runs of %lld frames of %d atoms and %d modes", (int)R, (long long)T,
                        (int)N, (int)M);
  rn_spectrum::FirstError ok;
  const hipStream_t work = to_host ? nullptr : (hipStream_t)stream;
  double *const d_out = to_host ? result.as<double>() : out;
  g_timer.reset();
  g_timer.mark(0);
  ok(hipMemcpy(g_small.ptr, small.data(), small.size() * sizeof(double), hipMemcpyHostToDevice));
  ok(hipMemcpy(g_modes.ptr, D, (size_t)M * K * sizeof(double), hipMemcpyHostToDevice));
  ok(hipStreamSynchronize(nullptr));  // the inputs are in HBM before a kernel on any stream reads them
  if (ok.first == hipSuccess) {
    const double *d_small = g_small.as<const double>();
    g_timer.mark(1, work);
    rn::launch_harmonic_synthesis(d_small, g_modes.as<const double>(), d_small + K, d_small + K + M, d_small + K + M + rm,
                                  K, M, R, T, t0, d_out, work);
    ok(hipGetLastError());
    g_timer.close();
    ok(hipEventRecord(g_done, work));
  }
  if (to_host) {
    g_timer.mark(2);
    ok(hipMemcpy(out, result.ptr, out_bytes, hipMemcpyDeviceToHost));
    g_timer.close();
    ok(hipStreamSynchronize(nullptr));  // (also after a failure: `result` is freed on return)
  }
  g_timer.collect();  // (while profiling is on, this waits for the kernel: the device entry too)
  if (ok.first != hipSuccess) return g_error.fail(RN_ERR_HIP, "%s", hipGetErrorString(ok.first));
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

extern "C" int rn_ht_set_profiling(int enabled) { return g_timer.set_profiling(g_workspace.mutex, enabled); }

extern "C" int rn_ht_phase_times(double *millis) { return g_timer.phase_times(g_workspace.mutex, millis); }

extern "C" const char *rn_ht_last_error(void) { return g_error.text.c_str(); }
