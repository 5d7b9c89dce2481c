// What the two start-table reducers that read positions share (spectrum_vdos.hip, spectrum_mode_vdos.hip) on top of
// spectrum_segment_core.hpp: the plans entry with its staged lattices, the entry front end up to the cache lock and the
// staging of a call's inputs under it.  Each reducer keeps its kernels, its own conditions (the groups and labels; the
// vectors), its block sizes and its loop.  The step formula (minimum image, then the lattice) stays written out in both
// kernels: every shared __device__ form of its three lines that was tried changed the instruction stream of
// build_series_kernel (commuted operands) and the register allocation of project_steps_kernel.
#pragma once
#include <cmath>

#include "spectrum_segment_core.hpp"

namespace rn_spectrum {

// the core's plans and buffers and the staged copy of host lattices (outside the accounting, like `source`); in the
// entry, so on the entry's device
struct StepPlans : SegmentPlans {
  DeviceBuffer lattices;
};

// Everything both entries do before they take their cache's lock: the null pointers, the sizes, the start table, the
// masses (all RN_ERR_INVALID_ARGUMENT), then check_call (hipFFT, the device) and the wait for the producer's stream.
// A reducer checks its own array and count (labels and G; vectors and M) before this call, null pointer included,
// because they too must be refused before a missing device is.  positions: float64[S][N][3] from `pos`, lattices:
// float64[1 or S][3][3] from `lat`; the rest are host arrays.  RN_OK with bins == 0 means there is nothing to compute.
inline int begin_step_call(Source pos, Source lat, int64_t num_lattices, int64_t S, int32_t N, const double *masses,
                           int64_t W, const int64_t *starts, int64_t Q, const double *taper, int average, int device,
                           int64_t bins, const double *densities, int64_t *n, std::vector<double> *sqrt_mass) {
  for (const void *q : {(const void *)pos.data, (const void *)lat.data, (const void *)masses, (const void *)starts,
                        (const void *)taper, (const void *)densities})
    if (!q) return RN_ERR_INVALID_ARGUMENT;
  if (N < 1 || S < 1 || S > ((int64_t)1 << 40) || (num_lattices != 1 && num_lattices != S))
    return RN_ERR_INVALID_ARGUMENT;
  int rc = check_table(S, W, starts, Q, average, bins);
  if (rc != RN_OK) return rc;
  for (int32_t i = 0; i < N; ++i)
    if (!(std::isfinite(masses[i]) && masses[i] > 0.0)) return RN_ERR_INVALID_ARGUMENT;
  *n = W - 1;
  rc = check_call({pos.data, lat.data, taper, densities}, *n, bins, device);
  if (rc != RN_OK || bins == 0) return rc;
  if ((rc = pos.wait()) != RN_OK || (rc = lat.wait()) != RN_OK) return rc;
  sqrt_mass->resize(N);
  for (int32_t i = 0; i < N; ++i) (*sqrt_mass)[i] = std::sqrt(masses[i]);
  return RN_OK;
}

// Under the cache's lock: host positions -> s.source and host lattices -> s.lattices (device inputs are read in place),
// the taper -> s.tau, the start table -> s.starts.
inline int stage_step_call(StepPlans &s, Source pos, Source lat, int64_t num_lattices, int64_t S, int32_t N,
                           const double *taper, const int64_t *starts, int64_t Q, const double **d_pos,
                           const double **d_lat) {
  int rc;
  if ((rc = pos.on_device(s.source, (size_t)S * N * 3 * sizeof(double), d_pos)) != RN_OK) return rc;
  if ((rc = lat.on_device(s.lattices, (size_t)num_lattices * 9 * sizeof(double), d_lat)) != RN_OK) return rc;
  if ((rc = upload(s.tau, taper, (size_t)s.n)) != RN_OK) return rc;
  return upload(s.starts, starts, (size_t)Q);
}

}  // namespace rn_spectrum
