// Entries of the covariance moments of quasi-harmonic mode analysis (include/rn_quasiharmonic.h; kernels:
// kernels_covariance.hip).
//
// The host cuts every block of frames into chunks of kCovarianceChunkFrames frames, ascending, the last one shorter:
// chunk = (first frame, frames, steps), where a chunk's steps are its frames but, in the last chunk of a block with
// joined = 0, the last one.  The table and the anchor go to the device; the positions are staged there (host entry)
// or read where they are (device entry) through Source (entry_runtime.hpp): the producer's stream is synchronised
// before the lock is taken, all work runs on the null stream, and the entry waits for the device before it returns,
// when first and second are in the host arrays.  The workspace holds the positions, the table, the anchor, the chunk
// partials, first and second, all grow-only.  counts is computed on the host.
#include <cstdint>
#include <mutex>
#include <vector>

#include "../../include/rn_quasiharmonic.h"
#include "entry_runtime.hpp"
#include "kernels.hpp"

namespace {

using rn_spectrum::DeviceBuffer;
using rn_spectrum::Fit;
using rn_spectrum::PhaseTimer;
using rn_spectrum::Source;

thread_local rn_spectrum::ErrorText g_error;
DeviceBuffer g_pos, g_tables, g_anchor, g_partials, g_first_partials, g_first, g_second;
rn_spectrum::Workspace g_workspace{&g_pos, &g_tables, &g_anchor, &g_partials, &g_first_partials, &g_first, &g_second};
PhaseTimer g_timer;  // copies to the device, rank updates, the sums over the chunks, copies to the host; under its mutex

int qh_moments(int device, Source pos, int64_t T, int32_t N, const double *anchor, const int64_t *bounds,
               const int32_t *joined, int64_t B, double *first, double *second, int64_t *counts) {
  if (!pos.data || !anchor || !bounds || !joined || !first || !second || !counts)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT, "a null pointer");
  if (N < 1 || T < 1)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT, "N = %d atoms or T = %lld frames is not positive", (int)N,
                        (long long)T);
  if (B < 1) return g_error.fail(RN_ERR_INVALID_ARGUMENT, "B = %lld blocks is not positive", (long long)B);
  if (B > T)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT, "B = %lld blocks of T = %lld frames: bounds cannot ascend strictly",
                        (long long)B, (long long)T);
  if (bounds[0] != 0 || bounds[B] != T)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT, "bounds run from %lld to %lld, not from 0 to T = %lld",
                        (long long)bounds[0], (long long)bounds[B], (long long)T);
  for (int64_t b = 0; b < B; ++b) {
    if (bounds[b + 1] <= bounds[b])
      return g_error.fail(RN_ERR_INVALID_ARGUMENT, "bounds[%lld] = %lld, bounds[%lld] = %lld: not strictly ascending",
                          (long long)b, (long long)bounds[b], (long long)(b + 1), (long long)bounds[b + 1]);
    if (joined[b] != 0 && joined[b] != 1)
      return g_error.fail(RN_ERR_INVALID_ARGUMENT, "joined[%lld] = %d is neither 0 nor 1", (long long)b,
                          (int)joined[b]);
  }
  if (joined[B - 1] != 0)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT, "joined[%lld] = 1: the last block has no step out of it",
                        (long long)(B - 1));

  // the chunk table
  const int64_t K = (int64_t)3 * N;
  const int64_t width = rn::kCovarianceChunkFrames;
  std::vector<int64_t> tables;  // [chunk][3], then block_chunks [B + 1]
  std::vector<int64_t> block_chunks(B + 1, 0);
  for (int64_t b = 0; b < B; ++b) {
    const int64_t frames = bounds[b + 1] - bounds[b], steps = frames - 1 + joined[b];
    counts[2 * b] = frames;
    counts[2 * b + 1] = steps;
    for (int64_t f = bounds[b]; f < bounds[b + 1]; f += width) {
      const int64_t nf = std::min(width, bounds[b + 1] - f);
      tables.insert(tables.end(), {f, nf, std::min(nf, bounds[b] + steps - f)});
    }
    block_chunks[b + 1] = (int64_t)(tables.size() / 3);
  }
  const int64_t num_chunks = block_chunks[B];
  const int64_t pairs = rn::covariance_pairs(K);
  if (B > 65535 || num_chunks * pairs > INT32_MAX)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT,
                        "B = %lld blocks or %lld chunks of %lld tile pairs exceed the grid (65535 blocks, 2^31 - 1 workgroups)",
                        (long long)B, (long long)num_chunks, (long long)pairs);
  tables.insert(tables.end(), block_chunks.begin(), block_chunks.end());

  if (int rc = rn_spectrum::select_device(device, g_error)) return rc;
  if (pos.wait() != RN_OK) return g_error.fail(RN_ERR_HIP, "the producer's stream could not be synchronised");

  std::lock_guard<std::mutex> lock(g_workspace.mutex);
  g_workspace.bind(device);
  const size_t first_bytes = (size_t)B * K * sizeof(double), second_bytes = 2 * first_bytes * K;
  const double *d_pos = nullptr;
  g_timer.reset();
  g_timer.mark(0);
  int rc = pos.on_device(g_pos, (size_t)T * K * sizeof(double), &d_pos);
  if (rc == RN_OK) rc = g_tables.ensure(tables.size() * sizeof(int64_t), Fit::kGrowOnly);
  if (rc == RN_OK) rc = g_anchor.ensure((size_t)K * sizeof(double), Fit::kGrowOnly);
  if (rc == RN_OK)
    rc = g_partials.ensure(rn::covariance_workspace_doubles(K, num_chunks) * sizeof(double), Fit::kGrowOnly);
  if (rc == RN_OK) rc = g_first_partials.ensure((size_t)num_chunks * K * sizeof(double), Fit::kGrowOnly);
  if (rc == RN_OK) rc = g_first.ensure(first_bytes, Fit::kGrowOnly);
  if (rc == RN_OK) rc = g_second.ensure(second_bytes, Fit::kGrowOnly);
  if (rc != RN_OK) {
    g_timer.collect();
    return g_error.fail(rc, "%s for %lld frames of %d atoms in %lld blocks (%lld chunks of %lld tile pairs)",
                        rc == RN_ERR_OUT_OF_MEMORY ? "no device memory" : "the copy of the positions failed", (long long)T,
                        (int)N, (long long)B, (long long)num_chunks, (long long)pairs);
  }
  rn_spectrum::FirstError ok;
  const int64_t *d_tables = g_tables.as<const int64_t>();
  ok(hipMemcpy(g_tables.ptr, tables.data(), tables.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  ok(hipMemcpy(g_anchor.ptr, anchor, (size_t)K * sizeof(double), hipMemcpyHostToDevice));
  if (ok.first == hipSuccess) {
    g_timer.mark(1);
    rn::launch_covariance_chunks(d_pos, K, g_anchor.as<const double>(), d_tables, num_chunks, g_partials.as<double>(),
                                 g_first_partials.as<double>(), nullptr);
    g_timer.mark(2);
    rn::launch_covariance_reduce(g_partials.as<const double>(), g_first_partials.as<const double>(), K,
                                 d_tables + 3 * num_chunks, B, g_first.as<double>(), g_second.as<double>(), nullptr);
    ok(hipGetLastError());
  }
  g_timer.mark(3);
  ok(hipMemcpy(first, g_first.ptr, first_bytes, hipMemcpyDeviceToHost));
  ok(hipMemcpy(second, g_second.ptr, second_bytes, hipMemcpyDeviceToHost));
  g_timer.collect();
  const hipError_t waited = hipDeviceSynchronize();  // (also after a failure: the buffers may be in use)
  ok(waited);
  if (ok.first != hipSuccess) return g_error.fail(RN_ERR_HIP, "%s", hipGetErrorString(ok.first));
  return RN_OK;
}

}  // namespace

extern "C" int rn_qh_moments(int device, const double *pos, int64_t T, int32_t N, const double *anchor,
                             const int64_t *bounds, const int32_t *joined, int64_t B, double *first, double *second,
                             int64_t *counts) {
  return qh_moments(device, Source::host(pos), T, N, anchor, bounds, joined, B, first, second, counts);
}

extern "C" int rn_qh_moments_device(int device, const double *d_pos, int64_t T, int32_t N, const double *anchor,
                                    const int64_t *bounds, const int32_t *joined, int64_t B, double *first, double *second,
                                    int64_t *counts, void *stream) {
  return qh_moments(device, Source::device(d_pos, stream), T, N, anchor, bounds, joined, B, first, second, counts);
}

extern "C" int rn_qh_chunk_frames(void) { return rn::kCovarianceChunkFrames; }

extern "C" int rn_qh_set_profiling(int enabled) { return g_timer.set_profiling(g_workspace.mutex, enabled); }

extern "C" int rn_qh_phase_times(double *millis) { return g_timer.phase_times(g_workspace.mutex, millis); }

extern "C" const char *rn_qh_last_error(void) { return g_error.text.c_str(); }
