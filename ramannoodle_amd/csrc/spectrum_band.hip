// Entries of the band moments of MD runs (include/rn_bandmodes.h; kernels: kernels_band.hip).
//
// The host finds the U bins with a nonzero weight in some row and lays out the rows of the transform, row 2 i + part of
// active bin i padded with -1 to Rp = a multiple of 64, and the weights of those rows, [B][Rp], divided by Q and zero
// in the padding.  Positions and alpha are staged on the device (host entry) or read where they are (device entry)
// through Source (entry_runtime.hpp): the producer's stream is synchronised before the lock is taken, all work runs on
// the null stream, and the entry waits for the device before it returns, when moments is in the host array.  The
// segments go through in equal blocks, the largest whose V and chunk partials fit workspace_limit beside the phase
// table, the weights and the result: per block one transform launch and one update, which adds to the result of the
// blocks before it.  hipFFT is not used (spectrum_segment_core.hpp is here for num_bins, check_table and balanced).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/rn_bandmodes.h"
#include "kernels.hpp"
#include "spectrum_segment_core.hpp"

namespace {

using rn_spectrum::DeviceBuffer;
using rn_spectrum::first_non_finite;
using rn_spectrum::Fit;
using rn_spectrum::PhaseTimer;
using rn_spectrum::Source;

thread_local rn_spectrum::ErrorText g_error;
DeviceBuffer g_pos, g_alpha, g_sqrt_mass, g_starts, g_taper, g_table, g_row_bins, g_weights, g_transforms, g_partials,
    g_moments;
rn_spectrum::Workspace g_workspace{&g_pos,      &g_alpha,   &g_sqrt_mass,  &g_starts,   &g_taper,  &g_table,
                                   &g_row_bins, &g_weights, &g_transforms, &g_partials, &g_moments};
// copies to the device and the phase table, transforms, rank updates, the copy to the host; under the workspace's mutex
PhaseTimer g_timer;

int bm_moments(int device, Source pos, const double *lattice, int64_t S, int32_t N, const double *masses, Source alpha,
               int64_t W, const int64_t *starts, int64_t Q, const double *taper, const double *bin_weights, int64_t B,
               int64_t bins, size_t workspace_limit, double *moments) {
  if (!pos.data || !lattice || !masses || !starts || !taper || !bin_weights || !moments)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT, "a null pointer");
  if (N < 1) return g_error.fail(RN_ERR_INVALID_ARGUMENT, "N = %d atoms is not positive", (int)N);
  if (B < 1 || B > 65535)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT, "B = %lld weight rows is not in [1, 65535]", (long long)B);
  if (W < 3) return g_error.fail(RN_ERR_INVALID_ARGUMENT, "W = %lld frames per segment is less than 3", (long long)W);
  if (W - 1 > (int64_t)1 << 28)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT, "W = %lld frames per segment is more than 2^28 + 1", (long long)W);
  if (bins != rn_spectrum::num_bins(W - 1))
    return g_error.fail(RN_ERR_INVALID_ARGUMENT, "bins = %lld is not (W - 1 + 1) / 2 - 1 = %lld", (long long)bins,
                        (long long)rn_spectrum::num_bins(W - 1));
  if (S < 1 || S > ((int64_t)1 << 40) || rn_spectrum::check_table(S, W, starts, Q, 1, bins) != RN_OK)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT,
                        "the start table is refused: Q = %lld segments of W = %lld frames, each start in [0, S - W], S = %lld",
                        (long long)Q, (long long)W, (long long)S);
  for (int32_t i = 0; i < N; ++i)
    if (!(std::isfinite(masses[i]) && masses[i] > 0.0))
      return g_error.fail(RN_ERR_INVALID_ARGUMENT, "masses[%d] = %g is not finite and positive", (int)i, masses[i]);
  if (const int64_t i = first_non_finite(lattice, 9); i >= 0)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT, "lattice[%d] is not finite", (int)i);
  if (const int64_t i = first_non_finite(bin_weights, B * bins); i >= 0)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT, "bin_weights[%lld][%lld] is not finite", (long long)(i / bins),
                        (long long)(i % bins));

  // the rows of the transform and their weights
  const int64_t n = W - 1, K = (int64_t)3 * N, Kc = K + (alpha.data ? 6 : 0);
  std::vector<int64_t> active;  // bins m = 1 .. bins with a nonzero weight in some row
  for (int64_t i = 0; i < bins; ++i)
    for (int64_t b = 0; b < B; ++b)
      if (bin_weights[b * bins + i] != 0.0) {
        active.push_back(i + 1);
        break;
      }
  const size_t result_bytes = (size_t)B * Kc * Kc * sizeof(double);
  if (active.empty()) {
    std::memset(moments, 0, result_bytes);
    return RN_OK;
  }
  const int64_t U = (int64_t)active.size(), Rp = rn::band_padded(2 * U), Kp = rn::band_padded(Kc);
  std::vector<int> row_bins(Rp, -1);
  std::vector<double> weights((size_t)B * Rp, 0.0), sqrt_mass(N);
  for (int64_t i = 0; i < U; ++i) {
    row_bins[2 * i] = row_bins[2 * i + 1] = (int)active[i];
    for (int64_t b = 0; b < B; ++b)
      weights[b * Rp + 2 * i] = weights[b * Rp + 2 * i + 1] = bin_weights[b * bins + active[i] - 1] / (double)Q;
  }
  for (int32_t i = 0; i < N; ++i) sqrt_mass[i] = std::sqrt(masses[i]);

  // segments per block: the largest equal blocks whose V and chunk partials fit beside what does not depend on them
  const size_t limit = workspace_limit ? workspace_limit : rn_spectrum::kDefaultWorkspace;
  const size_t fixed_bytes = (size_t)n * 2 * sizeof(double) + (size_t)Rp * sizeof(int) + weights.size() * sizeof(double) +
                             result_bytes;
  auto block_bytes = [&](int64_t count) {
    return (size_t)count * Rp * Kp * sizeof(double) + rn::band_partial_doubles(Kc, B, count * Rp) * sizeof(double);
  };
  int64_t per_block = Q;
  while (per_block > 1 && (fixed_bytes + block_bytes(per_block) > limit ||
                           rn::band_transform_workgroups(Kc, Rp, per_block) < 0 ||
                           rn::band_chunks(per_block * Rp) * rn::band_pairs(Kc) > INT32_MAX))
    per_block = (per_block + 1) / 2;
  per_block = rn_spectrum::balanced(Q, per_block);
  if (fixed_bytes + block_bytes(per_block) > limit)
    return g_error.fail(RN_ERR_OUT_OF_MEMORY,
                        "workspace_limit = %zu bytes: one segment of %lld rows x %lld columns needs %zu bytes beside the %zu of "
                        "the tables and the result", limit, (long long)Rp, (long long)Kp, block_bytes(1), fixed_bytes);
  if (rn::band_transform_workgroups(Kc, Rp, per_block) < 0 ||
      rn::band_chunks(per_block * Rp) * rn::band_pairs(Kc) > INT32_MAX)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT, "%lld rows x %lld columns exceed the grid (2^31 - 1 workgroups)",
                        (long long)Rp, (long long)Kp);

  if (int rc = rn_spectrum::select_device(device, g_error)) return rc;
  if (pos.wait() != RN_OK) return g_error.fail(RN_ERR_HIP, "the producer's stream could not be synchronised");

  std::lock_guard<std::mutex> lock(g_workspace.mutex);
  g_workspace.bind(device);
  const double *d_pos = nullptr, *d_alpha = nullptr;
  g_timer.reset();
  g_timer.mark(0);
  int rc = pos.on_device(g_pos, (size_t)S * K * sizeof(double), &d_pos);
  if (rc == RN_OK && alpha.data) rc = alpha.on_device(g_alpha, (size_t)S * 9 * sizeof(double), &d_alpha);
  if (rc == RN_OK) rc = g_sqrt_mass.ensure((size_t)N * sizeof(double), Fit::kGrowOnly);
  if (rc == RN_OK) rc = g_starts.ensure((size_t)Q * sizeof(int64_t), Fit::kGrowOnly);
  if (rc == RN_OK) rc = g_taper.ensure((size_t)n * sizeof(double), Fit::kGrowOnly);
  // (what workspace_limit counts is sized exactly: a later call with a smaller limit holds no more than its limit)
  if (rc == RN_OK) rc = g_table.ensure((size_t)n * 2 * sizeof(double));
  if (rc == RN_OK) rc = g_row_bins.ensure((size_t)Rp * sizeof(int));
  if (rc == RN_OK) rc = g_weights.ensure(weights.size() * sizeof(double));
  if (rc == RN_OK) rc = g_transforms.ensure((size_t)per_block * Rp * Kp * sizeof(double));
  if (rc == RN_OK) rc = g_partials.ensure(rn::band_partial_doubles(Kc, B, per_block * Rp) * sizeof(double));
  if (rc == RN_OK) rc = g_moments.ensure(result_bytes);
  if (rc != RN_OK) {
    g_timer.collect();
    return g_error.fail(rc, "%s for %lld frames of %d atoms, %lld segments (%lld per block) of %lld rows x %lld columns",
                        rc == RN_ERR_OUT_OF_MEMORY ? "no device memory" : "the copy of the positions or of alpha failed",
                        (long long)S, (int)N, (long long)Q, (long long)per_block, (long long)Rp, (long long)Kp);
  }
  rn_spectrum::FirstError ok;
  ok(hipMemcpy(g_sqrt_mass.ptr, sqrt_mass.data(), (size_t)N * sizeof(double), hipMemcpyHostToDevice));
  ok(hipMemcpy(g_starts.ptr, starts, (size_t)Q * sizeof(int64_t), hipMemcpyHostToDevice));
  ok(hipMemcpy(g_taper.ptr, taper, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  ok(hipMemcpy(g_row_bins.ptr, row_bins.data(), (size_t)Rp * sizeof(int), hipMemcpyHostToDevice));
  ok(hipMemcpy(g_weights.ptr, weights.data(), weights.size() * sizeof(double), hipMemcpyHostToDevice));
  if (ok.first == hipSuccess) {
    rn::launch_band_phases(n, g_table.as<double>(), nullptr);
    for (int64_t q0 = 0; q0 < Q; q0 += per_block) {
      const int64_t count = std::min(per_block, Q - q0);
      g_timer.mark(1);
      rn::launch_band_transform(d_pos, d_alpha, lattice, g_sqrt_mass.as<const double>(), K, Kc, n,
                                g_starts.as<const int64_t>(), q0, count, g_taper.as<const double>(),
                                g_table.as<const double>(), g_row_bins.as<const int>(), Rp, g_transforms.as<double>(),
                                nullptr);
      g_timer.mark(2);
      rn::launch_band_update(g_transforms.as<const double>(), count * Rp, Rp, Kc, g_weights.as<const double>(), B,
                             q0 > 0, g_partials.as<double>(), g_moments.as<double>(), nullptr);
    }
    ok(hipGetLastError());
  }
  g_timer.mark(3);
  ok(hipMemcpy(moments, g_moments.ptr, result_bytes, hipMemcpyDeviceToHost));
  g_timer.collect();
  const hipError_t waited = hipDeviceSynchronize();  // (also after a failure: the buffers may be in use)
  ok(waited);
  if (ok.first != hipSuccess) return g_error.fail(RN_ERR_HIP, "%s", hipGetErrorString(ok.first));
  return RN_OK;
}

}  // namespace

extern "C" int rn_bm_moments(int device, const double *pos, const double *lattice, int64_t S, int32_t N,
                             const double *masses, const double *alpha, int64_t W, const int64_t *starts, int64_t Q,
                             const double *taper, const double *bin_weights, int64_t B, int64_t bins,
                             size_t workspace_limit, double *moments) {
  return bm_moments(device, Source::host(pos), lattice, S, N, masses, Source::host(alpha), W, starts, Q, taper,
                    bin_weights, B, bins, workspace_limit, moments);
}

extern "C" int rn_bm_moments_device(int device, const double *d_pos, const double *lattice, int64_t S, int32_t N,
                                    const double *masses, const double *d_alpha, int64_t W, const int64_t *starts,
                                    int64_t Q, const double *taper, const double *bin_weights, int64_t B, int64_t bins,
                                    size_t workspace_limit, double *moments, void *stream) {
  return bm_moments(device, Source::device(d_pos, stream), lattice, S, N, masses, Source::device(d_alpha, stream), W,
                    starts, Q, taper, bin_weights, B, bins, workspace_limit, moments);
}

extern "C" int rn_bm_set_profiling(int enabled) { return g_timer.set_profiling(g_workspace.mutex, enabled); }

extern "C" int rn_bm_phase_times(double *millis) { return g_timer.phase_times(g_workspace.mutex, millis); }

extern "C" const char *rn_bm_last_error(void) { return g_error.text.c_str(); }
