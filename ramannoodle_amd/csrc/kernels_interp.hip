// The interpolation polarizability model (include/rn_interp.h): per-degree-of-freedom splines about a reference
// structure, evaluated for a batch of frames, and its analytic Jacobian.
//
// Definition (all float64).  x_t [frame][3N] fractional positions, x_ref [3N], F [J][3N] the Cartesian basis vectors
// with the lattice folded in (F[j][3i+r] = sum_s L[r][s] b_j[i][s]), and per DOF j a piecewise polynomial s_j with
// breakpoints x_0 < .. < x_P and Taylor coefficients c[p][q][9] about x_p (q = 0..K, K the model's highest order; a
// DOF of lower order has zero leading coefficients, and 0 u + c is exact):
//   d = x - x_ref,  m = d - floor(d),  w = m > 0.5 ? m - 1 : m          (exactly +0.5 stays, -0.5 becomes +0.5)
//   a[t][j]  = sum_k w[t][k] F[j][k]
//   p        = #{i in 1..P-1 : x_i <= a}                                 (the end pieces extend beyond the knots)
//   s_j(a)   = Horner in u = a - x_p over c[p][K..0]
//   alpha[t] = alpha_ref + sum_j scale_j s_j(a[t][j])                    scale_j = 1 - mask_j, nine components
//   jac[t][c][k] = sum_j scale_j s'_{j,c}(a[t][j]) F[j][k]               c = (xx, yy, zz, xy, xz, yz), kernels_group.hip
//
// interp_alpha_kernel: the tall-skinny product frames x 3N by 3N x J on the matrix pipe with the spline evaluation
// and the sum over the DOFs in its epilogue; the amplitudes never reach HBM.  A workgroup (4 waves) owns kSub tiles of
// kTileFrames = 16 frames (kSub = 1; 2 or 4 for calls of at least 8192 or 16384 frames, see launch_alpha) and walks
// all DOFs itself in ascending tiles of kTileDofs = 64, 16 per wave; inside a DOF tile it walks the 3N columns in
// ascending k-tiles of kTileCols = 32 (8 k-steps of v_mfma_f64_16x16x4_f64, each applied to the kSub frame tiles: a
// value of F serves all of them).
//   Second operand: the wrapped displacements.  Per k-tile, thread (row = thread / 32, column = thread % 32) loads
//   its column of frames row, row + 8, ... and of x_ref, wraps by the rule above and writes LDS [frame][column] with
//   the row stride of 34 doubles of kernels_mode.hip (an operand read of sixteen frames x two quads then touches
//   every bank once).  Loads are unconditional from clamped addresses; remainders of the frames and of 3N are zeros.
//   First operand: the wave's rows of F, [dof0 + l15][c0 + 4 ks + quad], read from global memory (L2-resident),
//   zero past the DOFs or the columns.  Both operands of the next k-tile are requested before the products of this one.
//   Result register j of tile s of lane (l15, quad) is DOF 4 j + quad at frame 16 s + l15 (mode_increment_kernel's).
//   Epilogue of a DOF tile: per register the piece search (branch-free, trip count = the model's largest piece count,
//   loads from clamped indices), Horner on the nine components, times scale_j, added into nine per-lane sums for
//   that frame.  With kJac the derivative's six components, times scale_j, are also written to g [frame][6][J].
//   After the last DOF tile: per lane the sum is over its DOFs in ascending order; the four quads are summed by the
//   xor butterfly (16, then 32), the four waves through LDS as ((w0 + w1) + w2) + w3, alpha_ref is added last and
//   nine doubles are stored per frame.  No atomics: repeated calls are bit-identical, and a frame's result does not
//   depend on the other frames of the call (a frame's sums read only its own column of the tile).
//
// interp_rows_kernel: jac rows = g x F, (frames * 6) x J by J x 3N, again on v_mfma_f64_16x16x4_f64.  This is a twin
// of the float64 row product of kernels_gemm.hip, not a reuse: that kernel keeps the weights of its whole reduction dimension
// in registers (K = 4 KQ, a template parameter: the embedding widths) and carries the network's epilogues; here the
// reduction dimension is J, unbounded, and the second operand is the model's own transposed matrix FT [3N][J].  A workgroup owns 16 rows
// x 64 columns (16 per wave) and walks J in ascending k-tiles of 32; the first operand is g [row0 + l15][4 ks + quad],
// the second FT [col0 + l15][4 ks + quad], both read from global memory from clamped addresses with zeros selected
// past the edges, so result register j of lane (l15, quad) is row 4 j + quad at column l15 and sixteen lanes store 128
// contiguous bytes.  One order of summation (k-tiles ascending, k-steps ascending), no atomics.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"

namespace rn {

namespace {

constexpr int kTileFrames = 16;
constexpr int kTileDofs = 64;               // 16 per wave
constexpr int kTileCols = 32;               // columns of 3N per k-tile
constexpr int kTileStride = kTileCols + 2;  // LDS row stride in doubles (kernels_mode.hip)
constexpr int kKSteps = kTileCols / 4;
constexpr int kThreads = 256;

typedef double f64x4_t __attribute__((ext_vector_type(4)));

template <int KO, bool kJac, int kSub>
__global__ void __launch_bounds__(kThreads)
    interp_alpha_kernel(const double *__restrict__ pos, int64_t S, InterpModel m, double *__restrict__ alpha,
                        double *__restrict__ g) {
  constexpr int kFrames = kSub * kTileFrames;  // frames of this workgroup: kSub instruction tiles of 16
  constexpr int kStaged = kFrames / 8;         // frames a thread stages per k-tile: rows srow, srow + 8, ...
  __shared__ double tile[kFrames * kTileStride];
  __shared__ double red[4 * kFrames * 9];
  const int64_t t0 = (int64_t)blockIdx.x * kFrames;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, quad = lane >> 4;
  const int frames = (int)std::min<int64_t>(kFrames, S - t0);
  const int64_t K3 = m.K3;
  const int J = m.J;
  const int srow = threadIdx.x / kTileCols, scol = threadIdx.x % kTileCols;
  const double *xbase = pos + t0 * K3;

  double sum[kSub][9];
#pragma unroll
  for (int s = 0; s < kSub; ++s)
#pragma unroll
    for (int e = 0; e < 9; ++e) sum[s][e] = 0.0;

  // The operands of a k-tile are requested one k-tile ahead (the first k-tile of the next DOF tile included) and kept
  // raw in registers; the zeros of the remainders are selected when they are used, so no wait precedes the products.
  double raw_a[kKSteps], raw_x[kStaged], raw_r;
  auto request = [&](int dof0, int64_t c0) {
    const int cols = (int)std::min<int64_t>(kTileCols, K3 - c0);
    const int row = dof0 + wave * 16 + l15;
    const double *frow = m.F + (int64_t)(row < J ? row : 0) * K3;
#pragma unroll
    for (int ks = 0; ks < kKSteps; ++ks) raw_a[ks] = frow[4 * ks + quad < cols ? c0 + 4 * ks + quad : 0];
    const int64_t at = scol < cols ? c0 + scol : 0;
    raw_r = m.ref[at];
#pragma unroll
    for (int i = 0; i < kStaged; ++i) raw_x[i] = xbase[(int64_t)(srow + 8 * i < frames ? srow + 8 * i : 0) * K3 + at];
  };
  request(0, 0);

  for (int dof0 = 0; dof0 < J; dof0 += kTileDofs) {
    const int wdof0 = dof0 + wave * 16;
    const bool row_live = wdof0 + l15 < J;  // the DOF whose row of F this lane holds (first operand: row l15)
    f64x4_t acc[kSub];
#pragma unroll
    for (int s = 0; s < kSub; ++s) acc[s] = f64x4_t{0.0, 0.0, 0.0, 0.0};
    for (int64_t c0 = 0; c0 < K3; c0 += kTileCols) {
      const int cols = (int)std::min<int64_t>(kTileCols, K3 - c0);
      double a[kKSteps];
#pragma unroll
      for (int ks = 0; ks < kKSteps; ++ks) a[ks] = row_live && 4 * ks + quad < cols ? raw_a[ks] : 0.0;
#pragma unroll
      for (int i = 0; i < kStaged; ++i) {
        const double d = raw_x[i] - raw_r;
        const double f = d - floor(d);
        const double w = f > 0.5 ? f - 1.0 : f;
        tile[(srow + 8 * i) * kTileStride + scol] = srow + 8 * i < frames && scol < cols ? w : 0.0;
      }
      __syncthreads();
      if (c0 + kTileCols < K3) {
        request(dof0, c0 + kTileCols);
      } else if (dof0 + kTileDofs < J) {
        request(dof0 + kTileDofs, 0);
      }
      const double *b = tile + l15 * kTileStride + quad;  // frame 16 s + l15, column 4 ks + quad
#pragma unroll
      for (int ks = 0; ks < kKSteps; ++ks)
#pragma unroll
        for (int s = 0; s < kSub; ++s)
          acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], b[s * (kTileFrames * kTileStride) + 4 * ks], acc[s], 0, 0, 0);
      __syncthreads();  // the next k-tile is written over this one
    }

#pragma unroll
    for (int s = 0; s < kSub; ++s) {
#pragma unroll 1  // (one register's tables at a time: unrolled, the four sets of coefficients cost the occupancy)
      for (int j = 0; j < 4; ++j) {
        const int dof = wdof0 + 4 * j + quad;
        const bool live = dof < J;
        const int dc = live ? dof : 0;
        // (zero for a DOF past the model: its row of F was zeros)
        const double am = j == 0 ? acc[s][0] : j == 1 ? acc[s][1] : j == 2 ? acc[s][2] : acc[s][3];
        const int base = m.poff[dc], P = m.poff[dc + 1] - base;
        const double *xb = m.xs + base + dc;  // x_0 .. x_P
        int p = 0;
        for (int i = 1; i < m.Pmax; ++i) p += (i < P) & (xb[i < P ? i : P] <= am);
        const double u = am - xb[p];
        const double *c = m.coef + (int64_t)(base + p) * ((KO + 1) * 9);
        const double sc = live ? m.scale[dc] : 0.0;
#pragma unroll
        for (int e = 0; e < 9; ++e) {
          double v = c[KO * 9 + e];
#pragma unroll
          for (int q = KO - 1; q >= 0; --q) v = fma(v, u, c[q * 9 + e]);
          sum[s][e] += sc * v;
        }
        if constexpr (kJac) {
          constexpr int comp[6] = {0, 4, 8, 1, 2, 5};
          if (live && 16 * s + l15 < frames) {
            double *go = g + (t0 + 16 * s + l15) * 6 * (int64_t)J + dof;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
              double v = (double)KO * c[KO * 9 + comp[k]];
#pragma unroll
              for (int q = KO - 1; q >= 1; --q) v = fma(v, u, (double)q * c[q * 9 + comp[k]]);
              go[(int64_t)k * J] = sc * v;
            }
          }
        }
      }
    }
  }

  if (!alpha) return;  // (uniform: the Jacobian entries want g only)
#pragma unroll
  for (int s = 0; s < kSub; ++s)
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      double v = sum[s][e];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (quad == 0) red[(wave * kFrames + 16 * s + l15) * 9 + e] = v;
    }
  __syncthreads();
  for (int at = threadIdx.x; at < kFrames * 9; at += kThreads) {
    const int f = at / 9, e = at % 9;
    if (f < frames) {
      const double *r = red + at;
      const double total = ((r[0] + r[kFrames * 9]) + r[2 * kFrames * 9]) + r[3 * kFrames * 9];
      alpha[(t0 + f) * 9 + e] = m.alpha_ref[e] + total;
    }
  }
}

__global__ void __launch_bounds__(kThreads)
    interp_rows_kernel(const double *__restrict__ g, int64_t R, int J, const double *__restrict__ FT, int64_t K3,
                       double *__restrict__ jac) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, quad = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * 16;
  const int64_t col0 = (int64_t)blockIdx.y * 64 + wave * 16;
  const bool row_live = r0 + l15 < R, col_live = col0 + l15 < K3;
  const double *grow = g + (row_live ? r0 + l15 : 0) * J;
  const double *frow = FT + (col_live ? col0 + l15 : 0) * J;
  f64x4_t acc = f64x4_t{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < J; k0 += kTileCols) {
    const int ks_live = std::min(kTileCols, J - k0);
    double a[kKSteps], b[kKSteps];
#pragma unroll
    for (int ks = 0; ks < kKSteps; ++ks) {
      const int k = 4 * ks + quad;
      const int at = k < ks_live ? k0 + k : 0;
      const double av = grow[at], bv = frow[at];
      a[ks] = row_live && k < ks_live ? av : 0.0;
      b[ks] = col_live && k < ks_live ? bv : 0.0;
    }
#pragma unroll
    for (int ks = 0; ks < kKSteps; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], b[ks], acc, 0, 0, 0);
  }
  if (!col_live) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t row = r0 + 4 * j + quad;
    if (row < R) jac[row * K3 + col0 + l15] = acc[j];
  }
}

template <bool kJac, int kSub>
void launch_alpha_tiles(const double *pos, int64_t S, const InterpModel &m, double *alpha, double *g, hipStream_t st) {
  constexpr int frames = kSub * kTileFrames;
  const unsigned blocks = (unsigned)((S + frames - 1) / frames);
  switch (m.order) {
    case 1: interp_alpha_kernel<1, kJac, kSub><<<blocks, kThreads, 0, st>>>(pos, S, m, alpha, g); break;
    case 2: interp_alpha_kernel<2, kJac, kSub><<<blocks, kThreads, 0, st>>>(pos, S, m, alpha, g); break;
    case 3: interp_alpha_kernel<3, kJac, kSub><<<blocks, kThreads, 0, st>>>(pos, S, m, alpha, g); break;
    case 4: interp_alpha_kernel<4, kJac, kSub><<<blocks, kThreads, 0, st>>>(pos, S, m, alpha, g); break;
    default: interp_alpha_kernel<5, kJac, kSub><<<blocks, kThreads, 0, st>>>(pos, S, m, alpha, g); break;
  }
}

// Frames per workgroup.  A workgroup of one instruction tile (16 frames) fetches every row of F for 16 frames; with
// two or four tiles a fetched value serves as many products.  Measured at 256 atoms, 768 cubic DOFs
// (profiles/interpolation_model.txt): one tile 8.6 M frames/s at 10 000 frames, two tiles 10.9 M there, four tiles
// 11.8 M at 40 000; but four tiles at 2 000 frames (32 workgroups for 256 CUs) took 1.15 ms where one tile takes
// 0.52 ms.  So the wider workgroups are taken only when they still give every one of the chip's 256 CUs a workgroup.
// The arithmetic of a frame is the same in all three: the choice changes no bit of the result.
constexpr int64_t kChipWorkgroups = 256;

template <bool kJac>
void launch_alpha(const double *pos, int64_t S, const InterpModel &m, double *alpha, double *g, hipStream_t st) {
  if (S >= 4 * kTileFrames * kChipWorkgroups) {
    launch_alpha_tiles<kJac, 4>(pos, S, m, alpha, g, st);
  } else if (S >= 2 * kTileFrames * kChipWorkgroups) {
    launch_alpha_tiles<kJac, 2>(pos, S, m, alpha, g, st);
  } else {
    launch_alpha_tiles<kJac, 1>(pos, S, m, alpha, g, st);
  }
}

}  // namespace

void launch_interp_alpha(const double *pos, int64_t S, const InterpModel &m, double *alpha, hipStream_t st) {
  if (S <= 0) return;
  launch_alpha<false>(pos, S, m, alpha, nullptr, st);
}

void launch_interp_jacobian(const double *pos, int64_t S, const InterpModel &m, double *g, double *jac, hipStream_t st) {
  if (S <= 0) return;
  launch_alpha<true>(pos, S, m, nullptr, g, st);
  const int64_t R = S * 6;
  interp_rows_kernel<<<dim3((unsigned)((R + 15) / 16), (unsigned)((m.K3 + 63) / 64)), kThreads, 0, st>>>(g, R, m.J, m.FT,
                                                                                                       m.K3, jac);
}

}  // namespace rn
