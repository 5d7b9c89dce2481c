// What the increment entries of a polarizability model share on the host (api.hip: PotGNN, api_interp.hip: the
// interpolation model): the atom-group table, the upload of the mode vectors, the walk over chunks of frames whose
// Jacobian rows overlap by one frame, and the argument checks of the group, mode and partial-Raman entries.  A model
// brings its own Jacobian rows, its own frames per chunk and its own ordering on the caller's stream.  Host only.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "host_runtime.hpp"
#include "kernels.hpp"

namespace rn {

// The atoms bucketed by group for launch_group_increments: csr = perm [N] (ascending atom index within a group) followed
// by gptr [G+1].  false on a label outside [0, G) or an empty group.
inline bool group_csr(const int32_t *labels, int N, int G, std::vector<int32_t> &csr) {
  std::vector<int32_t> ptr(G + 1, 0);
  for (int i = 0; i < N; ++i) {
    if (labels[i] < 0 || labels[i] >= G) return false;
    ++ptr[labels[i] + 1];
  }
  for (int g = 0; g < G; ++g) {
    if (ptr[g + 1] == 0) return false;
    ptr[g + 1] += ptr[g];
  }
  csr.assign((size_t)N + G + 1, 0);
  std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
  for (int i = 0; i < N; ++i) csr[fill[labels[i]]++] = i;
  std::copy(ptr.begin(), ptr.end(), csr.begin() + N);
  return true;
}

// The group table of a handle: the CSR of the last labels on the device, uploaded only when the labels change.
struct GroupTable {
  DeviceBuf csr;  // perm [N] | gptr [G+1]
  std::vector<int32_t> labels;
  int G = 0;
  const int *perm() const { return csr.as<int>(); }
  // labels host int32[N] in [0, G), every group used; otherwise the error of `h` names `entry` and RnInvalid is thrown.
  // `wait` (or null: nothing): the stream that is synchronised before an upload overwrites a permutation that work
  // enqueued earlier may still read.
  template <class H>
  void set(H *h, const char *entry, const int32_t *new_labels, int N, int new_G, const hipStream_t *wait) {
    std::vector<int32_t> table;
    if (!group_csr(new_labels, N, new_G, table)) {
      set_error(h, "%s: a label outside [0, G) or an empty group", entry);
      throw RnInvalid{};
    }
    if (G == new_G && labels.size() == (size_t)N && std::equal(new_labels, new_labels + N, labels.begin())) return;
    if (wait) HIP_TRY(hipStreamSynchronize(*wait));
    csr.upload(table.data(), table.size() * sizeof(int32_t));
    labels.assign(new_labels, new_labels + N);
    G = new_G;
  }
};

// The mode vectors of a mode-increments call on the device: D [M][N][3] | P [M][N][3] in `buf`, counted against `limit`.
struct ModeVectors {
  const double *disp, *proj;
  size_t bytes;  // what they took of the limit
};
inline ModeVectors upload_modes(DeviceBuf &buf, const double *disp, const double *proj, int M, int N, size_t limit,
                                hipStream_t wait) {
  const size_t entries = (size_t)M * N * 3, bytes = entries * sizeof(double);
  if (limit <= 2 * bytes) throw HipError{hipErrorOutOfMemory, "mode_increments: the modes do not fit the workspace limit"};
  HIP_TRY(hipStreamSynchronize(wait));  // (an earlier call may still read the old modes)
  buf.ensure(2 * bytes);
  double *d_disp = buf.as<double>(), *d_proj = d_disp + entries;
  HIP_TRY(hipMemcpy(d_disp, disp, bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_proj, proj, bytes, hipMemcpyHostToDevice));
  return ModeVectors{d_disp, d_proj, 2 * bytes};
}

// The loop every increment entry shares: the S - 1 steps of S frames go through in chunks of F steps whose Jacobian rows
// overlap by one frame -- the last frame's rows are carried into the next chunk.  jac holds (F + 1) * rows doubles.
// jacobian_rows(first, count, jac, extra) enqueues the rows of `count` frames from frame `first` on st;
// contract(t0, f) enqueues the contraction of the chunk's f steps from step t0 (its rows start at jac) on st.
// extra (or null): a second buffer of (F + 1) * extra_rows doubles that jacobian_rows fills and that is carried likewise
// (PotGNN's lattice rows).
template <class Rows, class Contract>
void walk_chunks(int64_t S, int64_t F, int64_t rows, double *jac, hipStream_t st, Rows jacobian_rows, Contract contract,
                 double *extra = nullptr, int64_t extra_rows = 0) {
  jacobian_rows((int64_t)0, (int64_t)1, jac, extra);
  for (int64_t t0 = 0; t0 < S - 1; t0 += F) {
    const int64_t f = std::min<int64_t>(F, S - 1 - t0);
    if (t0 > 0) {
      HIP_TRY(hipMemcpyAsync(jac, jac + F * rows, rows * sizeof(double), hipMemcpyDeviceToDevice, st));
      if (extra) HIP_TRY(hipMemcpyAsync(extra, extra + F * extra_rows, extra_rows * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    jacobian_rows(t0 + 1, f, jac + rows, extra ? extra + extra_rows : nullptr);
    contract(t0, f);
    HIP_TRY(hipGetLastError());
  }
}

// The argument checks of the entries, before guarded(): RN_OK, or the status to return at once with the text set.
template <class H>
int check_group_entry(H *h, int64_t S, const void *d_positions, const void *labels, const void *d_out, int G) {
  if (!h) return RN_ERR_INVALID_ARGUMENT;
  if (S >= 2 && d_positions && labels && d_out && G >= 1 && G <= kMaxGroups) return RN_OK;
  set_error(h, "invalid arguments to group_increments_device (S < 2, G outside 1..%d or a null pointer)", kMaxGroups);
  return RN_ERR_INVALID_ARGUMENT;
}

template <class H>
int check_mode_entry(H *h, int64_t S, const void *d_positions, const void *disp, const void *proj, const void *d_out,
                     int32_t M, int rest) {
  if (!h) return RN_ERR_INVALID_ARGUMENT;
  if (S >= 2 && d_positions && disp && proj && d_out && M >= 1 && M <= kMaxModes && (rest == 0 || rest == 1)) return RN_OK;
  set_error(h, "invalid arguments to mode_increments_device (S < 2, M outside 1..%d, rest not 0 or 1 or a null pointer)",
            kMaxModes);
  return RN_ERR_INVALID_ARGUMENT;
}

template <class H>  // disp / proj: host [M][N][3], after check_mode_entry
int check_mode_vectors(H *h, const double *disp, const double *proj, int32_t M, int N) {
  const size_t entries = (size_t)M * N * 3;
  if (all_finite(disp, entries) && all_finite(proj, entries)) return RN_OK;
  set_error(h, "mode_increments_device: a non-finite entry in disp or proj");
  return RN_ERR_INVALID_ARGUMENT;
}

template <class H>
int check_partial_raman_entry(H *h, const void *ref_positions, const void *displacements, int64_t M, const void *labels,
                              int G, const void *raman) {
  if (!h) return RN_ERR_INVALID_ARGUMENT;
  if (M >= 0 && ref_positions && labels && G >= 1 && G <= kMaxGroups && (M == 0 || (displacements && raman))) return RN_OK;
  set_error(h, "invalid arguments to partial_raman_tensors (G outside 1..%d or a null pointer)", kMaxGroups);
  return RN_ERR_INVALID_ARGUMENT;
}

}  // namespace rn
