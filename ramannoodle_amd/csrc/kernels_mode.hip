// Phonon-mode contraction of polarizability Jacobians (rn_potgnn_mode_contract_device,
// rn_potgnn_mode_increments_device): the mode channels of ModeMDRamanSpectrum.
//
// Definition.  Jacobian rows J_c(t)[j] = d vec6_c / d x_j of frames t = 0..steps (float64 [frame][6][3N], component
// order (xx, yy, zz, xy, xz, yz) of kernels_group.hip, j = 3 i + r), fractional wrapped positions x_t [frame][3N],
// D[m][3N] (the fractional displacement of a unit amplitude of mode m) and P[m][3N] (the mode's dual):
//   dx_t[j]        = x_{t+1}[j] - x_t[j] - rint(x_{t+1}[j] - x_t[j])
//   a_c[t][m]      = sum_j 1/2 (J_c(t)[j] + J_c(t+1)[j]) D[m][j]                  c = 0..5
//   q[t][m]        = sum_j P[m][j] dx_t[j]
//   out[t][m][3r+s] = sigma[3r+s] a_{map(r,s)}[t][m] q[t][m],   map = {0,3,4,3,1,5,4,5,2}
// and, for the rest channel M, out[t][M] = total[t] - sum_{m<M} out[t][m] (ascending m) with total[t] the one-group
// increment of group_increment_kernel.  out is [t][out_channels][9]; channels past M (+ rest) are not touched.
//
// mode_increment_kernel: seven float64 tall-skinny products (steps x 3N by 3N x modes: six a_c and q) on the matrix pipe.
// Tiles: a workgroup (4 waves) owns kTileSteps = 16 steps x kTileModes = 64 modes and walks the 3N columns in ascending
// k-tiles of kTileCols = 32 (8 k-steps of v_mfma_f64_16x16x4_f64); a wave holds 16 modes x 16 steps in seven
// accumulators.  Per k-tile, thread (series s = thread / 32 < 7, column = thread % 32) loads its column of the tile's 17
// frames -- series 0..5: row c of the Jacobian, series 6: the positions -- and writes the 16 trapezoid means
// 1/2 (J(t) + J(t+1)) or minimum-image steps to LDS, [series][step][column] with a row stride of 34 doubles: an operand
// read (eight bytes a lane) is served in two groups of 32 lanes, sixteen steps x two quads, whose doubles then start at
// banks 4 l15 + 2 quad of the 64 and touch every bank once; the staging writes are contiguous along the column.
// So a workgroup reads each Jacobian row once per step tile, plus the one frame of overlap.  D and P are the
// instruction's first operand, read from global memory once per k-tile (8 + 8 doubles per lane, L2-resident), the staged
// series the second, read from LDS; a D value is used by six products.  Result register j of lane (l15, quad) is mode
// 4 j + quad at step l15 (the layout of project_steps_kernel and rowgemm_f64_mfma_kernel).  The frames of the next
// k-tile are requested before the products of this one.  The remainders of 3N, of the modes and of the steps to the
// tiles are zeros in LDS / registers; loads are unconditional from clamped addresses: nothing is read past an array.
// The epilogue multiplies a_c q sigma and stores the nine entries of (step, mode).
// The sum over j has one order: k-tiles ascending, k-steps ascending, the instruction's own order within a k-step.  A
// step reads only its own two frames, so the result does not depend on how the caller chunks the frames; there are no
// atomics: repeated calls are bit-identical.
//
// mode_rest_kernel: one wave per step.  total[t] exactly as group_increment_kernel sums one group of all atoms (lane
// l takes atoms l, l + 64, ..., then the fixed xor butterfly), then lanes 0..8 subtract the ascending sum over the
// step's mode channels, which the kernel above has written (same stream).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"

namespace rn {

namespace {

constexpr int kTileSteps = 16;              // steps per tile
constexpr int kTileModes = 64;              // modes per tile: 16 per wave
constexpr int kTileCols = 32;               // columns of 3N per k-tile
constexpr int kTileStride = kTileCols + 2;  // LDS row stride in doubles (see the head of this file)
constexpr int kKSteps = kTileCols / 4;      // k-steps of the 16x16x4 instruction per k-tile
constexpr int kSeries = 7;                  // six Jacobian rows and the positions
constexpr int kModeThreads = 256;
constexpr int kRestLanes = 64;

typedef double f64x4_t __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(kModeThreads)
    mode_increment_kernel(const double *__restrict__ jac, const double *__restrict__ pos, int64_t steps, int64_t K3,
                          const double *__restrict__ disp, const double *__restrict__ proj, int M,
                          const double *__restrict__ sigma, int out_channels, double *__restrict__ out) {
  __shared__ double tile[kSeries * kTileSteps * kTileStride];  // [series][step][column], row stride 34
  const int64_t t0 = (int64_t)blockIdx.x * kTileSteps;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, quad = lane >> 4;
  const int mode0 = blockIdx.y * kTileModes + wave * 16;  // the wave's first mode
  // frames t0 .. t0 + 16, no further than the last frame `steps`: frames - 1 steps
  const int frames = (int)std::min<int64_t>(kTileSteps + 1, steps + 1 - t0);
  const bool mode_live = mode0 + l15 < M;  // the mode whose rows of D and P this lane holds (first operand: row l15)
  const int64_t mrow = (int64_t)(mode_live ? mode0 + l15 : 0) * K3;
  const double *drow = disp + mrow, *prow = proj + mrow;

  // Staging: thread (series, column) keeps its column of the tile's 17 frames in registers.  Loads are unconditional,
  // from a clamped address, with the zero selected afterwards (project_steps_kernel says why).
  const int series = threadIdx.x / kTileCols, stage_col = threadIdx.x % kTileCols;
  const bool stager = series < kSeries;
  const double *source = series < 6 ? jac + t0 * 6 * K3 + (int64_t)series * K3 : pos + t0 * K3;
  const int64_t frame_stride = series < 6 ? 6 * K3 : K3;
  double staged[kTileSteps + 1];
  auto load_tile = [&](int64_t c0) {
    const double *first = source + (c0 + stage_col < K3 ? c0 + stage_col : 0), *p = first;
#pragma unroll
    for (int j = 0; j <= kTileSteps; ++j) {
      staged[j] = *(j < frames ? p : first);
      p += frame_stride;
    }
  };
  if (stager) load_tile(0);

  f64x4_t acc[kSeries];
#pragma unroll
  for (int s = 0; s < kSeries; ++s) acc[s] = f64x4_t{0.0, 0.0, 0.0, 0.0};

  for (int64_t c0 = 0; c0 < K3; c0 += kTileCols) {
    const int cols = (int)std::min<int64_t>(kTileCols, K3 - c0);
    // the wave's rows of D and P for this k-tile: [mode0 + l15][c0 + 4 ks + quad], zero past the modes or the columns
    double ad[kKSteps], ap[kKSteps];
#pragma unroll
    for (int ks = 0; ks < kKSteps; ++ks) {
      const int col = 4 * ks + quad;
      const bool in = mode_live && col < cols;
      const int64_t at = col < cols ? c0 + col : 0;
      const double d = drow[at], p = prow[at];
      ad[ks] = in ? d : 0.0;
      ap[ks] = in ? p : 0.0;
    }
    if (stager) {
      double *dst = tile + series * (kTileSteps * kTileStride) + stage_col;
#pragma unroll
      for (int j = 0; j < kTileSteps; ++j) {
        const bool in = j < frames - 1 && stage_col < cols;
        double v;
        if (series < 6) {
          v = 0.5 * (staged[j] + staged[j + 1]);
        } else {
          v = staged[j + 1] - staged[j];
          v -= rint(v);
        }
        dst[j * kTileStride] = in ? v : 0.0;
      }
    }
    __syncthreads();
    if (stager && c0 + kTileCols < K3) load_tile(c0 + kTileCols);
    // second operand: lane (l15, quad) holds step l15, column 4 ks + quad of each series
    const double *b = tile + l15 * kTileStride + quad;
#pragma unroll
    for (int ks = 0; ks < kKSteps; ++ks) {
#pragma unroll
      for (int s = 0; s < 6; ++s)
        acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(ad[ks], b[s * (kTileSteps * kTileStride) + 4 * ks], acc[s], 0, 0, 0);
      acc[6] = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[ks], b[6 * (kTileSteps * kTileStride) + 4 * ks], acc[6], 0, 0, 0);
    }
    __syncthreads();  // the next k-tile's series are written over these
  }

  const int64_t t = t0 + l15;
  if (t >= steps) return;
  double sg[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) sg[e] = sigma[e];
  constexpr int map[9] = {0, 3, 4, 3, 1, 5, 4, 5, 2};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int mode = mode0 + 4 * j + quad;
    if (mode >= M) continue;
    double *o = out + (t * out_channels + mode) * 9;
    const double q = acc[6][j];
#pragma unroll
    for (int e = 0; e < 9; ++e) o[e] = sg[e] * (acc[map[e]][j] * q);
  }
}

__global__ void __launch_bounds__(kRestLanes)
    mode_rest_kernel(const double *__restrict__ jac, const double *__restrict__ pos, int N, int M,
                     const double *__restrict__ sigma, int out_channels, double *__restrict__ out) {
  const int64_t t = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t K3 = (int64_t)3 * N;
  const double *ja = jac + t * 6 * K3, *jb = ja + 6 * K3;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = lane; i < N; i += kRestLanes) {
    const double *x0 = pos + (t * N + i) * 3, *x1 = x0 + K3;
    double dx[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double step = x1[r] - x0[r];
      dx[r] = step - rint(step);
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
  for (int off = kRestLanes / 2; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < 6; ++c) acc[c] += __shfl_xor(acc[c], off);
  }
  if (lane < 9) {
    constexpr int map[9] = {0, 3, 4, 3, 1, 5, 4, 5, 2};
    double v = acc[0];
#pragma unroll
    for (int c = 1; c < 6; ++c)
      if (map[lane] == c) v = acc[c];
    double *row = out + t * out_channels * 9 + lane;
    double sum = 0.0;
    for (int m = 0; m < M; ++m) sum += row[(int64_t)m * 9];
    row[(int64_t)M * 9] = sigma[lane] * v - sum;
  }
}

}  // namespace

void launch_mode_increments(const double *jac, const double *pos, int64_t steps, int N, const double *disp,
                            const double *proj, int M, const double *sigma, int out_channels, double *out,
                            hipStream_t st) {
  if (steps <= 0 || M <= 0) return;
  const unsigned tiles_t = (unsigned)((steps + kTileSteps - 1) / kTileSteps);
  const unsigned tiles_m = (unsigned)((M + kTileModes - 1) / kTileModes);
  mode_increment_kernel<<<dim3(tiles_t, tiles_m), kModeThreads, 0, st>>>(jac, pos, steps, (int64_t)3 * N, disp, proj, M,
                                                                        sigma, out_channels, out);
}

void launch_mode_rest(const double *jac, const double *pos, int64_t steps, int N, int M, const double *sigma,
                      int out_channels, double *out, hipStream_t st) {
  if (steps <= 0) return;
  mode_rest_kernel<<<(unsigned)steps, kRestLanes, 0, st>>>(jac, pos, N, M, sigma, out_channels, out);
}

}  // namespace rn
