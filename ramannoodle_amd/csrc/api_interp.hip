// Host orchestration + C ABI (include/rn_interp.h) of the interpolation polarizability model.
//
// A handle owns the model as the kernels read it (kernels.hpp: InterpModel; the tables padded to one Horner trip
// count) and the workspaces of its entries.  The evaluation is one launch per call; the Jacobian is two (the spline
// derivatives, then their product with the basis); the increment entries walk the frames in chunks whose Jacobian rows
// overlap by one frame, with the loop, group table, mode upload and argument checks the PotGNN entries of api.hip use
// (increments.hpp), and hand the rows to the same contractions (launch_group_increments, launch_mode_increments,
// launch_mode_rest) with sigma = 1.  All device work of an entry is enqueued on the caller's stream, in order.  The guard
// every entry runs in, the error types and the device buffer are host_runtime.hpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rn_interp.h"
#include "../../include/rn_potgnn.h"
#include "host_runtime.hpp"
#include "increments.hpp"
#include "kernels.hpp"

using namespace rn;

namespace {

std::string g_interp_create_error;

constexpr size_t kDefaultWorkspace = (size_t)1 << 30;
constexpr int64_t kHostChunk = 1 << 15;  // frames per staged chunk of the host entry

}  // namespace

struct rn_interp {
  mutable std::recursive_mutex lock;
  int device = 0;
  int N = 0, J = 0, order = 0, Pmax = 0;
  bool symmetric = false;
  DeviceBuf F, FT, ref, alpha_ref, poff, xs, coef, scale, ones;
  DeviceBuf g, jac, modes, io_pos, io_out, disp;
  GroupTable groups;
  std::string error;
  int device_index() const { return device; }
  static std::string &create_error() { return g_interp_create_error; }
  InterpModel model() const {
    return InterpModel{F.as<double>(),   FT.as<double>(),    ref.as<double>(), alpha_ref.as<double>(), xs.as<double>(),
                       coef.as<double>(), scale.as<double>(), poff.as<int>(),   (int64_t)3 * N,         J,
                       order,             Pmax};
  }
};

namespace {

// The create arguments, checked on the host; the text of the first violation in `why`.
bool check_model(int32_t N, const double *lattice, const double *ref_positions, const double *alpha_ref, int32_t J,
                 const double *basis, const int32_t *poff, const double *xs, const int32_t *orders, const double *coef,
                 std::string &why) {
  if (!lattice || !ref_positions || !alpha_ref || !basis || !poff || !xs || !orders || !coef) {
    why = "a null pointer";
    return false;
  }
  if (N < 1 || N > (1 << 28) || J < 1) {
    why = "N < 1 or J < 1";
    return false;
  }
  if (poff[0] != 0) {
    why = "piece_offsets[0] is not 0";
    return false;
  }
  size_t coefs = 0;
  for (int j = 0; j < J; ++j) {
    if (orders[j] < 1 || orders[j] > RN_INTERP_MAX_ORDER) {
      why = "DOF " + std::to_string(j) + ": order " + std::to_string(orders[j]) + " outside 1.." +
            std::to_string(RN_INTERP_MAX_ORDER);
      return false;
    }
    if (poff[j + 1] <= poff[j]) {
      why = "DOF " + std::to_string(j) + " has no piece";
      return false;
    }
    coefs += (size_t)(poff[j + 1] - poff[j]) * (orders[j] + 1) * 9;
  }
  if (!all_finite(lattice, 9) || !all_finite(ref_positions, (size_t)N * 3) || !all_finite(alpha_ref, 9) ||
      !all_finite(basis, (size_t)J * N * 3) || !all_finite(xs, (size_t)poff[J] + J) || !all_finite(coef, coefs)) {
    why = "a non-finite entry";
    return false;
  }
  for (int j = 0; j < J; ++j) {
    const double *x = xs + poff[j] + j;
    for (int i = 0; i < poff[j + 1] - poff[j]; ++i)
      if (!(x[i] < x[i + 1])) {
        why = "DOF " + std::to_string(j) + ": breakpoints do not ascend";
        return false;
      }
  }
  return true;
}

void build(rn_interp *h, int32_t N, const double *lattice, const double *ref_positions, const double *alpha_ref, int32_t J,
           const double *basis, const int32_t *poff, const double *xs, const int32_t *orders, const double *coef) {
  h->N = N;
  h->J = J;
  const size_t K3 = (size_t)3 * N;
  int order = 1, pmax = 1;
  for (int j = 0; j < J; ++j) {
    order = std::max(order, (int)orders[j]);
    pmax = std::max(pmax, (int)(poff[j + 1] - poff[j]));
  }
  h->order = order;
  h->Pmax = pmax;
  // F[j][3i+r] = sum_s L[r][s] b_j[i][s] (ascending s), and its transpose for the Jacobian's product
  std::vector<double> F((size_t)J * K3), FT((size_t)J * K3);
  for (int j = 0; j < J; ++j)
    for (int i = 0; i < N; ++i)
      for (int r = 0; r < 3; ++r) {
        const double *b = basis + ((size_t)j * N + i) * 3;
        const double v = (lattice[3 * r] * b[0] + lattice[3 * r + 1] * b[1]) + lattice[3 * r + 2] * b[2];
        F[(size_t)j * K3 + 3 * i + r] = v;
        FT[((size_t)3 * i + r) * J + j] = v;
      }
  // the tables padded to order + 1 coefficients per piece; the largest |c| and the largest asymmetry
  const size_t pieces = (size_t)poff[J], stride = (size_t)(order + 1) * 9;
  std::vector<double> padded(pieces * stride, 0.0);
  double largest = 0.0, skew = 0.0;
  const double *src = coef;
  for (int j = 0; j < J; ++j)
    for (int p = poff[j]; p < poff[j + 1]; ++p)
      for (int q = 0; q <= orders[j]; ++q, src += 9) {
        std::copy(src, src + 9, padded.begin() + p * stride + (size_t)q * 9);
        for (int e = 0; e < 9; ++e) largest = std::max(largest, std::fabs(src[e]));
        skew = std::max({skew, std::fabs(src[1] - src[3]), std::fabs(src[2] - src[6]), std::fabs(src[5] - src[7])});
      }
  h->symmetric = skew <= 1e-12 * largest;
  const std::vector<double> ones((size_t)std::max(J, 9), 1.0);
  h->F.upload(F.data(), F.size() * sizeof(double));
  h->FT.upload(FT.data(), FT.size() * sizeof(double));
  h->ref.upload(ref_positions, K3 * sizeof(double));
  h->alpha_ref.upload(alpha_ref, 9 * sizeof(double));
  h->poff.upload(poff, ((size_t)J + 1) * sizeof(int32_t));
  h->xs.upload(xs, (pieces + J) * sizeof(double));
  h->coef.upload(padded.data(), padded.size() * sizeof(double));
  h->scale.upload(ones.data(), (size_t)J * sizeof(double));
  h->ones.upload(ones.data(), 9 * sizeof(double));
}

// Jacobian rows of s frames -> jac [s][6][K3], in blocks of at most `block` frames (the rows of h->g).
void jacobian_rows(rn_interp *h, const double *d_pos, int64_t s, int64_t block, double *jac, hipStream_t st) {
  const InterpModel m = h->model();
  for (int64_t f0 = 0; f0 < s; f0 += block) {
    const int64_t f = std::min(block, s - f0);
    launch_interp_jacobian(d_pos + f0 * m.K3, f, m, h->g.as<double>(), jac + f0 * 6 * m.K3, st);
    HIP_TRY(hipGetLastError());
  }
}

bool needs_symmetry(rn_interp *h, const char *entry) {
  if (h->symmetric) return true;
  set_error(h, "%s: the Jacobian has six components and needs symmetric tables; this model's are not", entry);
  return false;
}

// The chunk walk of both increment entries (increments.hpp: walk_chunks) with as many steps F per chunk as `limit` bytes
// hold; contract(jac, pos, f, out) launches the contraction of a chunk's f steps on st, the caller's stream.
template <class Contract>
void chunked_increments(rn_interp *h, const double *d_pos, int64_t S, size_t limit, int out_channels, double *d_out,
                        hipStream_t st, Contract contract) {
  const size_t rows = (size_t)6 * 3 * h->N, grow = (size_t)6 * h->J;
  const size_t per = (rows + grow) * sizeof(double), carry = rows * sizeof(double);
  if (limit < per + carry) throw HipError{hipErrorOutOfMemory, "increments: one step does not fit the workspace limit"};
  const int64_t F = (int64_t)std::min<size_t>((limit - carry) / per, (size_t)(S - 1));
  h->g.ensure((size_t)F * grow * sizeof(double));
  h->jac.ensure((size_t)(F + 1) * rows * sizeof(double));
  double *jac = h->jac.as<double>();
  const int64_t n3 = (int64_t)3 * h->N;
  walk_chunks(
      S, F, (int64_t)rows, jac, st,
      [&](int64_t first, int64_t count, double *to, double *) { jacobian_rows(h, d_pos + first * n3, count, F, to, st); },
      [&](int64_t t0, int64_t f) { contract(jac, d_pos + t0 * n3, f, d_out + t0 * out_channels * 9); });
}

}  // namespace

extern "C" {

int rn_interp_create(int32_t N, const double *lattice, const double *ref_positions, const double *alpha_ref, int32_t J,
                     const double *basis_cart, const int32_t *piece_offsets, const double *breakpoints,
                     const int32_t *orders, const double *coefficients, int device, rn_interp **handle) {
  if (!handle) return RN_ERR_INVALID_ARGUMENT;
  *handle = nullptr;
  std::string why;
  if (!check_model(N, lattice, ref_positions, alpha_ref, J, basis_cart, piece_offsets, breakpoints, orders, coefficients,
                   why)) {
    set_error<rn_interp>(nullptr, "invalid arguments to rn_interp_create: %s", why.c_str());
    return RN_ERR_INVALID_ARGUMENT;
  }
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) {
    set_error<rn_interp>(nullptr, "rn_interp_create: no device %d", device);
    return RN_ERR_NO_DEVICE;
  }
  rn_interp *h = nullptr;
  try {
    h = new rn_interp;
  } catch (const std::bad_alloc &) {
    return RN_ERR_OUT_OF_MEMORY;
  }
  h->device = device;
  const int rc = guarded(h, [&]() {
    build(h, N, lattice, ref_positions, alpha_ref, J, basis_cart, piece_offsets, breakpoints, orders, coefficients);
  });
  if (rc != RN_OK) {
    g_interp_create_error = h->error;
    delete h;
    return rc;
  }
  *handle = h;
  return RN_OK;
}

void rn_interp_destroy(rn_interp *h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  delete h;
}

const char *rn_interp_last_error(const rn_interp *h) {
  if (!h) return g_interp_create_error.c_str();
  std::lock_guard<std::recursive_mutex> lock(h->lock);
  return h->error.c_str();
}

int rn_interp_set_mask(rn_interp *h, const uint8_t *mask) {
  if (!h) return RN_ERR_INVALID_ARGUMENT;
  if (!mask) {
    set_error(h, "invalid arguments to set_mask (a null pointer)");
    return RN_ERR_INVALID_ARGUMENT;
  }
  return guarded(h, [&]() {
    std::vector<double> scale(h->J);
    for (int j = 0; j < h->J; ++j) scale[j] = mask[j] ? 0.0 : 1.0;
    HIP_TRY(hipDeviceSynchronize());  // (earlier work may still read the old mask)
    h->scale.upload(scale.data(), scale.size() * sizeof(double));
  });
}

int rn_interp_is_symmetric(const rn_interp *h) {
  if (!h) return RN_ERR_INVALID_ARGUMENT;
  return h->symmetric ? 1 : 0;
}

int rn_interp_calc_polarizabilities(rn_interp *h, const double *positions, int64_t S, double *alpha) {
  if (!h) return RN_ERR_INVALID_ARGUMENT;
  if (S < 0 || (S > 0 && (!positions || !alpha))) {
    set_error(h, "invalid arguments to calc_polarizabilities (S < 0 or a null pointer)");
    return RN_ERR_INVALID_ARGUMENT;
  }
  if (S == 0) return RN_OK;
  return guarded(h, [&]() {
    const int64_t n3 = (int64_t)3 * h->N, block = std::min(S, kHostChunk);
    HIP_TRY(hipDeviceSynchronize());  // (the staging buffers are filled from the null stream)
    h->io_pos.ensure((size_t)block * n3 * sizeof(double));
    h->io_out.ensure((size_t)block * 9 * sizeof(double));
    for (int64_t f0 = 0; f0 < S; f0 += block) {
      const int64_t f = std::min(block, S - f0);
      HIP_TRY(hipMemcpy(h->io_pos.p, positions + f0 * n3, (size_t)f * n3 * sizeof(double), hipMemcpyHostToDevice));
      launch_interp_alpha(h->io_pos.as<double>(), f, h->model(), h->io_out.as<double>(), nullptr);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpy(alpha + f0 * 9, h->io_out.p, (size_t)f * 9 * sizeof(double), hipMemcpyDeviceToHost));
    }
  });
}

int rn_interp_forward_device(rn_interp *h, const double *d_positions, int64_t S, double *d_alpha, void *stream) {
  if (!h) return RN_ERR_INVALID_ARGUMENT;
  if (S < 1 || !d_positions || !d_alpha) {
    set_error(h, "invalid arguments to forward_device (S < 1 or a null pointer)");
    return RN_ERR_INVALID_ARGUMENT;
  }
  return guarded(h, [&]() {
    launch_interp_alpha(d_positions, S, h->model(), d_alpha, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
  });
}

int rn_interp_jacobian_device(rn_interp *h, const double *d_positions, int64_t S, double *d_jac, void *stream) {
  if (!h) return RN_ERR_INVALID_ARGUMENT;
  if (S < 1 || !d_positions || !d_jac) {
    set_error(h, "invalid arguments to jacobian_device (S < 1 or a null pointer)");
    return RN_ERR_INVALID_ARGUMENT;
  }
  if (!needs_symmetry(h, "jacobian_device")) return RN_ERR_INVALID_ARGUMENT;
  return guarded(h, [&]() {
    const size_t grow = (size_t)6 * h->J * sizeof(double);
    const int64_t block = (int64_t)std::min<size_t>((size_t)S, std::max<size_t>(1, (kDefaultWorkspace / 4) / grow));
    h->g.ensure((size_t)block * grow);
    jacobian_rows(h, d_positions, S, block, d_jac, (hipStream_t)stream);
  });
}

int rn_interp_group_increments_device(rn_interp *h, const double *d_positions, int64_t S, const int32_t *labels, int G,
                                      size_t workspace_limit, double *d_out, void *stream) {
  if (const int rc = check_group_entry(h, S, d_positions, labels, d_out, G)) return rc;
  if (!needs_symmetry(h, "group_increments_device")) return RN_ERR_INVALID_ARGUMENT;
  return guarded(h, [&]() {
    hipStream_t st = (hipStream_t)stream;
    const int N = h->N;
    h->groups.set(h, "group_increments_device", labels, N, G, &st);
    const int *perm = h->groups.perm(), *gptr = perm + N;
    const double *sigma = h->ones.as<double>();
    chunked_increments(h, d_positions, S, workspace_limit ? workspace_limit : kDefaultWorkspace, G, d_out, st,
                       [&](const double *jac, const double *pos, int64_t f, double *out) {
                         launch_group_increments(jac, (int64_t)6 * N * 3, pos, nullptr, 0.0, f, N, perm, gptr, G, sigma,
                                                 out, st);
                       });
  });
}

int rn_interp_mode_increments_device(rn_interp *h, const double *d_positions, int64_t S, const double *disp,
                                     const double *proj, int32_t M, int rest, size_t workspace_limit, double *d_out,
                                     void *stream) {
  if (const int rc = check_mode_entry(h, S, d_positions, disp, proj, d_out, M, rest)) return rc;
  if (!needs_symmetry(h, "mode_increments_device")) return RN_ERR_INVALID_ARGUMENT;
  if (const int rc = check_mode_vectors(h, disp, proj, M, h->N)) return rc;
  return guarded(h, [&]() {
    hipStream_t st = (hipStream_t)stream;
    const size_t limit = workspace_limit ? workspace_limit : kDefaultWorkspace;
    const int N = h->N, channels = M + rest;
    const ModeVectors modes = upload_modes(h->modes, disp, proj, M, N, limit, st);
    const double *sigma = h->ones.as<double>();
    chunked_increments(h, d_positions, S, limit - modes.bytes, channels, d_out, st,
                       [&](const double *jac, const double *pos, int64_t f, double *out) {
                         launch_mode_increments(jac, pos, f, N, modes.disp, modes.proj, M, sigma, channels, out, st);
                         if (rest) launch_mode_rest(jac, pos, f, N, M, sigma, channels, out, st);
                       });
  });
}

int rn_interp_partial_raman_tensors(rn_interp *h, const double *ref_positions, const double *displacements, int64_t M,
                                    const int32_t *labels, int G, double *raman) {
  if (const int rc = check_partial_raman_entry(h, ref_positions, displacements, M, labels, G, raman)) return rc;
  if (!needs_symmetry(h, "partial_raman_tensors")) return RN_ERR_INVALID_ARGUMENT;
  return guarded(h, [&]() {
    const int N = h->N;
    const hipStream_t null_stream = nullptr;
    h->groups.set(h, "partial_raman_tensors", labels, N, G, &null_stream);
    if (M == 0) return;
    const size_t n3 = (size_t)N * 3;
    HIP_TRY(hipDeviceSynchronize());  // (the staging buffers are filled from the null stream)
    h->io_pos.upload(ref_positions, n3 * sizeof(double));
    h->disp.upload(displacements, (size_t)M * n3 * sizeof(double));
    h->io_out.ensure((size_t)M * G * 9 * sizeof(double));
    h->g.ensure((size_t)6 * h->J * sizeof(double));
    h->jac.ensure(6 * n3 * sizeof(double));
    jacobian_rows(h, h->io_pos.as<double>(), 1, 1, h->jac.as<double>(), nullptr);
    // R[m][g] = 2 sum_{i in g} J_i . d_{m,i}: the kernel's 1/2 (J + J) . (2 d)
    const int *perm = h->groups.perm();
    launch_group_increments(h->jac.as<double>(), 0, nullptr, h->disp.as<double>(), 2.0, M, N, perm, perm + N, G,
                            h->ones.as<double>(), h->io_out.as<double>(), nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(raman, h->io_out.p, (size_t)M * G * 9 * sizeof(double), hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
