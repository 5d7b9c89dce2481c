// Entries of the nearest-reference distance and the farthest-point selection (include/rn_select.h; kernels:
// kernels_select.hip).
//
// X and R are staged on the device (host entries) or read where they are (device entries) through Source
// (entry_runtime.hpp): the producer's stream is synchronised before the lock is taken, all work runs on the null
// stream, and the entry waits for the device before it returns, when the results are in the host arrays.  center and
// scale always are host arrays; they go to the device as params [2][D] (zeros and ones where they are null, which
// leave every operand as it is, bit for bit).  The workspace holds the staged operands, params, the norms of R, the
// search partials, (dist2, index) or (mind, the two pick partial buffers, the column mean, the picks), all grow-only.
// The picks of a selection are `count` launches on the stream with nothing from the host in between.
#include <cstdint>
#include <limits>
#include <mutex>
#include <vector>

#include "../../include/rn_select.h"
#include "entry_runtime.hpp"
#include "kernels.hpp"

namespace {

using rn_spectrum::DeviceBuffer;
using rn_spectrum::Fit;
using rn_spectrum::PhaseTimer;
using rn_spectrum::Source;

thread_local rn_spectrum::ErrorText g_error;
DeviceBuffer g_x, g_r, g_params, g_norms, g_search, g_dist2, g_index, g_pick_partials, g_mean, g_picks, g_pick_dist2;
rn_spectrum::Workspace g_workspace{&g_x,     &g_r,          &g_params, &g_norms, &g_search,    &g_dist2,
                                   &g_index, &g_pick_partials, &g_mean,   &g_picks, &g_pick_dist2};
PhaseTimer g_timer;  // copies to the device, the nearest search, the picks, copies to the host; under its mutex

constexpr int64_t kMaxRows = INT32_MAX;  // the grids, and rows x splits of the search partials

// the checks both entries share; `params` becomes (center, scale) [2][D]
int check_operands(Source X, int64_t S, Source R, int64_t M, int64_t min_M, int64_t D, const double *center,
                   const double *scale, std::vector<double> &params) {
  if (D < 1) return g_error.fail(RN_ERR_INVALID_ARGUMENT, "D = %lld columns is not positive", (long long)D);
  if (S < 0 || M < min_M)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT, "S = %lld rows is negative or M = %lld reference rows is less than %lld",
                        (long long)S, (long long)M, (long long)min_M);
  if (S > kMaxRows || M > kMaxRows || D > kMaxRows)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT, "S = %lld, M = %lld or D = %lld exceeds 2^31 - 1", (long long)S,
                        (long long)M, (long long)D);
  if ((S > 0 && !X.data) || (M > 0 && !R.data)) return g_error.fail(RN_ERR_INVALID_ARGUMENT, "a null pointer");
  params.assign((size_t)(2 * D), 0.0);
  for (int64_t c = 0; c < D; ++c) {
    if (center) params[(size_t)c] = center[c];
    params[(size_t)(D + c)] = scale ? scale[c] : 1.0;
  }
  if (const int64_t at = rn_spectrum::first_non_finite(params.data(), 2 * D); at >= 0)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT, "%s[%lld] is not finite", at < D ? "center" : "scale",
                        (long long)(at < D ? at : at - D));
  if (X.on_host)
    if (const int64_t at = rn_spectrum::first_non_finite(X.data, S * D); at >= 0)
      return g_error.fail(RN_ERR_INVALID_ARGUMENT, "X[%lld][%lld] is not finite", (long long)(at / D), (long long)(at % D));
  if (R.on_host)
    if (const int64_t at = rn_spectrum::first_non_finite(R.data, M * D); at >= 0)
      return g_error.fail(RN_ERR_INVALID_ARGUMENT, "R[%lld][%lld] is not finite", (long long)(at / D), (long long)(at % D));
  return RN_OK;
}

// after the checks: device, producer's stream.  The caller then locks and binds.
int enter(int device, Source X, Source R) {
  if (int rc = rn_spectrum::select_device(device, g_error)) return rc;
  if (X.wait() != RN_OK || R.wait() != RN_OK)
    return g_error.fail(RN_ERR_HIP, "the producer's stream could not be synchronised");
  return RN_OK;
}

// the operands and params on the device (phase 0); d_R stays null when M = 0
int stage(Source X, int64_t S, Source R, int64_t M, int64_t D, const std::vector<double> &params, const double **d_X,
          const double **d_R) {
  int rc = X.on_device(g_x, (size_t)(S * D) * sizeof(double), d_X);
  *d_R = nullptr;
  if (rc == RN_OK && M > 0) rc = R.on_device(g_r, (size_t)(M * D) * sizeof(double), d_R);
  if (rc == RN_OK) rc = g_params.ensure(params.size() * sizeof(double), Fit::kGrowOnly);
  if (rc == RN_OK && hipMemcpy(g_params.ptr, params.data(), params.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
    rc = RN_ERR_HIP;
  return rc;
}

// the buffers of a search, then its three kernels: (dist2, index) of every row of X, on the device
int ensure_search(int64_t S, int64_t M) {
  int64_t splits, tiles_per_split;
  rn::select_splits(S, M, &splits, &tiles_per_split);
  int rc = g_norms.ensure((size_t)M * sizeof(double), Fit::kGrowOnly);
  if (rc == RN_OK) rc = g_search.ensure((size_t)(splits * S) * sizeof(rn::SelectBest), Fit::kGrowOnly);
  if (rc == RN_OK) rc = g_dist2.ensure((size_t)S * sizeof(double), Fit::kGrowOnly);
  if (rc == RN_OK) rc = g_index.ensure((size_t)S * sizeof(int64_t), Fit::kGrowOnly);
  return rc;
}

void search(const double *d_X, int64_t S, const double *d_R, int64_t M, int64_t D, int exclude_self) {
  const double *params = g_params.as<const double>();
  rn::launch_select_norms(d_R, M, D, params, g_norms.as<double>(), nullptr);
  rn::launch_select_search(d_X, S, d_R, M, D, params, g_norms.as<const double>(), exclude_self,
                           g_search.as<rn::SelectBest>(), nullptr);
  rn::launch_select_merge(d_X, S, d_R, M, D, params, g_search.as<const rn::SelectBest>(), g_dist2.as<double>(),
                          g_index.as<int64_t>(), nullptr);
}

int failed(int rc, int64_t S, int64_t M, int64_t D) {
  g_timer.collect();
  return g_error.fail(rc, "%s for S = %lld rows, M = %lld reference rows of D = %lld columns",
                      rc == RN_ERR_OUT_OF_MEMORY ? "no device memory" : "the copy of the operands failed", (long long)S,
                      (long long)M, (long long)D);
}

int finish(rn_spectrum::FirstError &ok) {
  g_timer.collect();
  ok(hipDeviceSynchronize());  // (also after a failure: the buffers may be in use)
  if (ok.first != hipSuccess) return g_error.fail(RN_ERR_HIP, "%s", hipGetErrorString(ok.first));
  return RN_OK;
}

int nearest(int device, Source X, int64_t S, Source R, int64_t M, int64_t D, const double *center, const double *scale,
            int exclude_self, double *dist2, int64_t *index) {
  std::vector<double> params;
  if (int rc = check_operands(X, S, R, M, 1, D, center, scale, params)) return rc;
  if (S > 0 && (!dist2 || !index)) return g_error.fail(RN_ERR_INVALID_ARGUMENT, "a null pointer");
  if (S == 0) return RN_OK;
  if (int rc = enter(device, X, R)) return rc;

  std::lock_guard<std::mutex> lock(g_workspace.mutex);
  g_workspace.bind(device);
  g_timer.reset();
  g_timer.mark(0);
  const double *d_X = nullptr, *d_R = nullptr;
  int rc = stage(X, S, R, M, D, params, &d_X, &d_R);
  if (rc == RN_OK) rc = ensure_search(S, M);
  if (rc != RN_OK) return failed(rc, S, M, D);
  rn_spectrum::FirstError ok;
  g_timer.mark(1);
  search(d_X, S, d_R, M, D, exclude_self != 0);
  ok(hipGetLastError());
  g_timer.mark(3);
  ok(hipMemcpy(dist2, g_dist2.ptr, (size_t)S * sizeof(double), hipMemcpyDeviceToHost));
  ok(hipMemcpy(index, g_index.ptr, (size_t)S * sizeof(int64_t), hipMemcpyDeviceToHost));
  return finish(ok);
}

int farthest(int device, Source X, int64_t S, int64_t D, Source R, int64_t M, const double *center, const double *scale,
             int64_t first, int64_t count, int64_t *picks, double *dist2) {
  std::vector<double> params;
  if (int rc = check_operands(X, S, R, M, 0, D, center, scale, params)) return rc;
  if (count < 0 || count > S)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT, "count = %lld picks of S = %lld rows", (long long)count, (long long)S);
  if (first >= S) return g_error.fail(RN_ERR_INVALID_ARGUMENT, "first = %lld is not a row of S = %lld", (long long)first, (long long)S);
  if (first >= 0 && M > 0)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT, "first = %lld with M = %lld reference rows: the reference decides the first pick",
                        (long long)first, (long long)M);
  if (count > 0 && (!picks || !dist2)) return g_error.fail(RN_ERR_INVALID_ARGUMENT, "a null pointer");
  if (count == 0) return RN_OK;
  if (int rc = enter(device, X, R)) return rc;

  std::lock_guard<std::mutex> lock(g_workspace.mutex);
  g_workspace.bind(device);
  g_timer.reset();
  g_timer.mark(0);
  const double *d_X = nullptr, *d_R = nullptr;
  const int64_t slices = rn::select_slices(S);
  int rc = stage(X, S, R, M, D, params, &d_X, &d_R);
  if (rc == RN_OK) rc = M > 0 ? ensure_search(S, M) : g_dist2.ensure((size_t)S * sizeof(double), Fit::kGrowOnly);
  if (rc == RN_OK) rc = g_pick_partials.ensure((size_t)(2 * slices) * sizeof(rn::SelectBest), Fit::kGrowOnly);
  if (rc == RN_OK) rc = g_mean.ensure((size_t)D * sizeof(double), Fit::kGrowOnly);
  if (rc == RN_OK) rc = g_picks.ensure((size_t)count * sizeof(int64_t), Fit::kGrowOnly);
  if (rc == RN_OK) rc = g_pick_dist2.ensure((size_t)count * sizeof(double), Fit::kGrowOnly);
  if (rc != RN_OK) return failed(rc, S, M, D);
  rn_spectrum::FirstError ok;
  const double *d_params = g_params.as<const double>();
  double *mind = g_dist2.as<double>();  // the search leaves the seed where the picks update it
  rn::SelectBest *partials[2] = {g_pick_partials.as<rn::SelectBest>(), g_pick_partials.as<rn::SelectBest>() + slices};
  const bool from_none = M == 0;
  g_timer.mark(1);
  if (!from_none) {
    search(d_X, S, d_R, M, D, 0);
  } else if (first < 0) {
    rn::launch_select_column_mean(d_X, S, D, g_mean.as<double>(), nullptr);
    rn::launch_select_distance_to(d_X, S, D, d_params, g_mean.as<const double>(), mind, nullptr);
  } else {
    rn::launch_select_fill(mind, S, std::numeric_limits<double>::infinity(), nullptr);
  }
  g_timer.mark(2);
  if (first < 0) rn::launch_select_argmax(mind, S, partials[0], nullptr);
  for (int64_t k = 0; k < count; ++k)
    rn::launch_select_pick(d_X, S, D, d_params, mind, partials[k & 1], partials[(k + 1) & 1], k == 0 ? first : -1,
                           from_none && k == 0, k + 1 == count, k, g_picks.as<int64_t>(), g_pick_dist2.as<double>(),
                           nullptr);
  ok(hipGetLastError());
  g_timer.mark(3);
  ok(hipMemcpy(picks, g_picks.ptr, (size_t)count * sizeof(int64_t), hipMemcpyDeviceToHost));
  ok(hipMemcpy(dist2, g_pick_dist2.ptr, (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
  return finish(ok);
}

}  // namespace

extern "C" int rn_select_nearest(int device, const double *X, int64_t S, const double *R, int64_t M, int64_t D,
                                 const double *center, const double *scale, int exclude_self, double *dist2,
                                 int64_t *index) {
  return nearest(device, Source::host(X), S, Source::host(R), M, D, center, scale, exclude_self, dist2, index);
}

extern "C" int rn_select_nearest_device(int device, const double *d_X, int64_t S, const double *d_R, int64_t M, int64_t D,
                                        const double *center, const double *scale, int exclude_self, double *dist2,
                                        int64_t *index, void *stream) {
  return nearest(device, Source::device(d_X, stream), S, Source::device(d_R, stream), M, D, center, scale, exclude_self,
                 dist2, index);
}

extern "C" int rn_select_farthest(int device, const double *X, int64_t S, int64_t D, const double *R, int64_t M,
                                  const double *center, const double *scale, int64_t first, int64_t count, int64_t *picks,
                                  double *dist2) {
  return farthest(device, Source::host(X), S, D, Source::host(R), M, center, scale, first, count, picks, dist2);
}

extern "C" int rn_select_farthest_device(int device, const double *d_X, int64_t S, int64_t D, const double *d_R, int64_t M,
                                         const double *center, const double *scale, int64_t first, int64_t count,
                                         int64_t *picks, double *dist2, void *stream) {
  return farthest(device, Source::device(d_X, stream), S, D, Source::device(d_R, stream), M, center, scale, first, count,
                  picks, dist2);
}

extern "C" int rn_select_tile_rows(void) { return rn::kSelectTile; }

extern "C" int64_t rn_select_reference_splits(int64_t S, int64_t M) {
  int64_t splits = 0, tiles_per_split = 0;
  rn::select_splits(S, M, &splits, &tiles_per_split);
  return splits;
}

extern "C" int rn_select_set_profiling(int enabled) { return g_timer.set_profiling(g_workspace.mutex, enabled); }

extern "C" int rn_select_phase_times(double *millis) { return g_timer.phase_times(g_workspace.mutex, millis); }

extern "C" const char *rn_select_last_error(void) { return g_error.text.c_str(); }
