// Atom-group contraction of polarizability Jacobians (rn_potgnn_group_increments_device,
// rn_potgnn_group_increments_cells_device, rn_potgnn_partial_raman_tensors).
//   group_increment_kernel  one wave per (step t, group g):
//     dv_c = sum_{i in g} 1/2 (J_c(a_t)_i + J_c(b_t)_i) . dx_{t,i}         c = 0..5 (xx, yy, zz, xy, xz, yz)
//     out[t][g][3r+s] = sigma[3r+s] dv_{map(r,s)}                           (symmetric 3x3, sigma de-standardises)
//   with, for a trajectory, a_t / b_t = frames t / t+1 and dx the minimum image of x_{t+1} - x_t in fractional
//   coordinates; for phonons, one Jacobian (stride 0) and dx = scale * d_t (scale 2: R = 2 J . d).
// The group's atoms come from a CSR permutation (perm, gptr) built on the host; each lane sums its atoms in
// ascending CSR order and the wave reduces by a fixed xor butterfly.  No atomics: the same inputs give the
// same bits, whatever the chunking of the caller.
//   cell_increment_kernel   one wave per step t (variable-cell trajectories): the share of the deforming cell,
//     dv_c = 1/2 (J_L,c(t) + J_L,c(t+1)) : (L_{t+1} - L_t)                 J_L,c = d vec6_c / d L  [3][3]
//     out[t][G][3r+s] = sigma[3r+s] dv_{map(r,s)}                           (the channel after the G atom groups)
//   Nine lanes, one per output entry, each a serial sum of nine products: nothing to reduce, nothing atomic.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace rn {

constexpr int kGroupLanes = 64;

__global__ __launch_bounds__(kGroupLanes) void group_increment_kernel(
    const double *__restrict__ jac, int64_t jac_stride, const double *__restrict__ pos,
    const double *__restrict__ disp, double disp_scale, int N, const int *__restrict__ perm,
    const int *__restrict__ gptr, int out_groups, const double *__restrict__ sigma, double *__restrict__ out) {
  const int64_t t = blockIdx.x;
  const int g = blockIdx.y, lane = threadIdx.x;
  const double *ja = jac + t * jac_stride;
  const double *jb = ja + jac_stride;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = gptr[g] + lane; k < gptr[g + 1]; k += kGroupLanes) {
    const int i = perm[k];
    double dx[3];
    if (disp) {
      const double *d = disp + (t * N + i) * 3;
#pragma unroll
      for (int r = 0; r < 3; ++r) dx[r] = disp_scale * d[r];
    } else {
      const double *x0 = pos + (t * N + i) * 3, *x1 = x0 + (int64_t)N * 3;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double step = x1[r] - x0[r];
        dx[r] = step - rint(step);
      }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const double *a = ja + ((int64_t)c * N + i) * 3, *b = jb + ((int64_t)c * N + i) * 3;
      double dot = 0.0;
#pragma unroll
      for (int r = 0; r < 3; ++r) dot = fma(0.5 * (a[r] + b[r]), dx[r], dot);
      acc[c] += dot;
    }
  }
#pragma unroll
  for (int off = kGroupLanes / 2; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < 6; ++c) acc[c] += __shfl_xor(acc[c], off);
  }
  if (lane < 9) {
    constexpr int map[9] = {0, 3, 4, 3, 1, 5, 4, 5, 2};
    double v = acc[0];
#pragma unroll
    for (int c = 1; c < 6; ++c)
      if (map[lane] == c) v = acc[c];
    out[(t * out_groups + g) * 9 + lane] = sigma[lane] * v;
  }
}

__global__ __launch_bounds__(kGroupLanes) void cell_increment_kernel(
    const double *__restrict__ jl, const double *__restrict__ lat, int channel, int out_groups,
    const double *__restrict__ sigma, double *__restrict__ out) {
  const int64_t t = blockIdx.x;
  const int lane = threadIdx.x;
  if (lane >= 9) return;
  constexpr int map[9] = {0, 3, 4, 3, 1, 5, 4, 5, 2};
  const double *ja = jl + (t * 6 + map[lane]) * 9, *jb = ja + 54;
  const double *l0 = lat + t * 9, *l1 = l0 + 9;
  double v = 0.0;
#pragma unroll
  for (int j = 0; j < 9; ++j) v = fma(0.5 * (ja[j] + jb[j]), l1[j] - l0[j], v);
  out[(t * out_groups + channel) * 9 + lane] = sigma[lane] * v;
}

void launch_group_increments(const double *jac, int64_t jac_stride, const double *pos, const double *disp,
                             double disp_scale, int64_t steps, int N, const int *perm, const int *gptr, int G,
                             const double *sigma, double *out, hipStream_t st, int out_groups) {
  if (steps <= 0 || G <= 0) return;
  group_increment_kernel<<<dim3((unsigned)steps, (unsigned)G), kGroupLanes, 0, st>>>(
      jac, jac_stride, pos, disp, disp_scale, N, perm, gptr, out_groups > 0 ? out_groups : G, sigma, out);
}

void launch_cell_increments(const double *jl, const double *lat, int64_t steps, int channel, int out_groups,
                            const double *sigma, double *out, hipStream_t st) {
  if (steps <= 0) return;
  cell_increment_kernel<<<(unsigned)steps, kGroupLanes, 0, st>>>(jl, lat, channel, out_groups, sigma, out);
}

}  // namespace rn
