// Band moments of MD runs (include/rn_bandmodes.h; the definition is band_moments_host of ramannoodle_amd/bandmodes.py):
// the cross-spectral matrix of the mass-weighted minimum-image steps (and, when alpha is given, of the six components of
// the polarizability differences), summed over the bins of a band,
//   moments[b][j][l] = 1/Q sum_q sum_m bw[b][m] Re(X_q[m][j] conj X_q[m][l]),   X_q[m][j] = sum_t taper[t] x[starts[q] + t][j] e^{-2 pi i m t / n}.
// Only the U bins that have a nonzero weight in some row are transformed.  Row rho = 2 i + part of the transform is
// active bin i, part 0 its real part (cos) and part 1 its imaginary part (-sin); rows and columns are padded with zeros
// to Rp and Kp, multiples of 64, so that V[segment][Rp][Kp] holds whole tiles and the update reads no remainder.
//
// band_phase_kernel: table[r] = (cos, -sin)(2 pi r / n) for the n distinct phases r = 0 .. n - 1, with sincospi of the
// once-rounded 2 r / n.
//
// band_transform_kernel: the product [Rp x n] . [n x Kp] of one segment on v_mfma_f64_16x16x4_f64 with the time as the
// contraction dimension.  A workgroup (4 waves) owns kTile = 64 rows x 64 columns of one segment; wave v holds rows
// 16 v .. 16 v + 15 against the 64 columns: four accumulators of the instruction.  It walks the time in ascending
// k-tiles of kSteps = 16 (4 k-steps of the instruction).
// First operand: lane (l15, quad) holds row 16 v + l15, time 4 ks + quad and makes that value itself, in registers, as
// the amp cos(omega t + phi) operand of kernels_harmonic.hip is made: taper[t] * table[r][part] with r = (m t) mod n
// kept in integers (r advances by (4 m) mod n per k-step, with one conditional subtraction), so the phase is exact for
// any n.  The operand never exists as a matrix in memory; each of its values feeds four instructions.  The table and
// taper values of the next k-tile are requested before the products of this one.
// Second operand: the same time of column 16 c + l15 from an LDS tile [time][column] with a row stride of 80 doubles:
// as in kernels_covariance.hip an operand read (eight bytes a lane) is served in two groups of 32 lanes, two times
// (quads) x sixteen columns, whose doubles start at banks 2 l15 and 2 l15 + 32 of the 64 and touch every bank once; the
// staging writes are contiguous along the columns.  Thread (quarter = thread / 64, column = thread % 64) loads what its
// column needs of 5 consecutive frames (4 steps and the frame after them) and writes 4 series values: column j = 3 i + r
// < K is sqrt(m_i) ((f[t+1] - f[t]) - rint(f[t+1] - f[t])) @ lattice, component r, from the three fractional coordinates
// of atom i (project_steps_kernel's step); column K + c is component c (xx, yy, zz, xy, yz, xz) of the symmetric part
// of alpha[t+1] - alpha[t] (two entries of each frame).  Neither series ever exists in HBM.  The frames of the next
// k-tile are requested before the products of this one.
// The remainders of n, of the rows and of the columns are zeros in LDS / in the first operand; loads are unconditional
// from clamped addresses (a column past K' reads column 0, a frame past the segment's last reads that last one, a row
// past 2 U reads bin 0), with the zero selected afterwards: nothing is read past an array.  Result register j of lane
// (l15, quad) is row 4 j + quad, column l15 (tools/mfma_f64_layout_probe.hip).
//
// band_update_kernel: the weighted symmetric rank update sum_rows w[b][row] V[row][j] V[row][l] over the rows of a block
// of segments (the weight row w[b][Rp] repeats per segment and carries bw / Q, zero for the padding), on the same
// instruction, with kernels_covariance.hip's tiling: pairs (I, J), I >= J, of 64-column tiles; the rows are cut into
// chunks of kBandChunkRows = 512 (kernels.hpp), a workgroup owns one pair of one chunk of one weight row, stages
// k-tiles of 16 rows of both tiles in LDS (side 0 multiplied by the weight) and writes its 64 x 64 partial sum to a
// workspace, [chunk][b][pair][64][64].  V is padded, so every chunk is whole k-tiles and no load needs a clamp.
// band_reduce_kernel: one workgroup per (pair, b) adds the chunks in ascending order, from zero, adds that to what the
// earlier blocks of segments left in moments (accumulate = 1) and writes element (r, c) and, through a transposing LDS
// tile, its mirror: each matrix is symmetric bit for bit.
// No atomics anywhere: the order of every sum depends on the shapes and the number of segments per block alone.
// RN_BM_CONSTANT_OPERAND (a timing variant, tools/band_modes_timing.py): the first operand is 0.5, with no table, no
// taper and no phase arithmetic.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"

namespace rn {

namespace {

constexpr int kTile = 64;             // rows and columns per tile
constexpr int kSteps = 16;            // times (transform) or rows (update) per k-tile
constexpr int kStride = kTile + 16;   // LDS row stride in doubles (see the head of this file)
constexpr int kKSteps = kSteps / 4;   // k-steps of the 16x16x4 instruction per k-tile
constexpr int kThreads = 256;
constexpr int kQuarterSteps = kSteps / 4;  // steps a stager of the transform owns per k-tile
constexpr int kHalfRows = kSteps / 2;      // rows a stager of the update owns per k-tile
constexpr int kPlane = kSteps * kStride;
constexpr int kMirrorStride = kTile + 1;

typedef double f64x4_t __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(kThreads) band_phase_kernel(int64_t n, double *__restrict__ table) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= n) return;
  double s, c;
  sincospi((2.0 * (double)r) / (double)n, &s, &c);
  table[2 * r] = c;
  table[2 * r + 1] = -s;
}

struct BandLattice {
  double l[9];  // row-major: rows = lattice vectors
};

// row_bins: int32 [Rp], the bin m of row rho (the same for both parts), -1 for the padding.  V: [count][Rp][Kp].
__global__ void __launch_bounds__(kThreads)
    band_transform_kernel(const double *__restrict__ pos, const double *__restrict__ alpha, BandLattice lattice,
                          const double *__restrict__ sqrt_mass, int64_t K, int64_t Kc, int64_t n,
                          const int64_t *__restrict__ starts, int64_t q0, const double *__restrict__ taper,
                          const double *__restrict__ table, const int *__restrict__ row_bins, int row_tiles,
                          int column_tiles, int64_t Rp, int64_t Kp, double *__restrict__ V) {
  __shared__ double tile[kPlane];  // [time][column], row stride 80
  const int column_tile = blockIdx.x % column_tiles;
  const int row_tile = (blockIdx.x / column_tiles) % row_tiles;
  const int64_t segment = (blockIdx.x / column_tiles) / row_tiles;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, quad = lane >> 4;
  const int64_t frame0 = starts[q0 + segment];  // the segment reads frames frame0 .. frame0 + n

  // staging: thread (quarter, column) keeps what its column needs of 5 frames in registers: three sources, a frame stride
  const int quarter = threadIdx.x >> 6, stage_col = threadIdx.x & 63;
  const int64_t column = (int64_t)column_tile * kTile + stage_col;
  const bool column_live = column < Kc, of_alpha = column_live && column >= K;
  const int64_t atom = column_live && !of_alpha ? column / 3 : 0;
  const int direction = column_live && !of_alpha ? (int)(column - 3 * atom) : 0;
  constexpr int first_entry[6] = {0, 4, 8, 1, 5, 2}, second_entry[6] = {0, 4, 8, 3, 7, 6};  // (a, b) and (b, a) of 3 a + b
  const int component = of_alpha ? (int)(column - K) : 0;
  const double *source[3];
  int64_t frame_stride;
  if (of_alpha) {  // (alpha is not null here: Kc > K only with alpha)
    source[0] = alpha + frame0 * 9 + first_entry[component];
    source[1] = alpha + frame0 * 9 + second_entry[component];
    source[2] = source[0];
    frame_stride = 9;
  } else {
    source[0] = pos + frame0 * K + 3 * atom;
    source[1] = source[0] + 1;
    source[2] = source[0] + 2;
    frame_stride = K;
  }
  const double scale = sqrt_mass[atom];
  const double l0 = lattice.l[direction], l1 = lattice.l[3 + direction], l2 = lattice.l[6 + direction];
  double staged[kQuarterSteps + 1][3];
  auto load_tile = [&](int64_t t0) {  // frames t0 + 4 quarter .. + 4 of the segment
#pragma unroll
    for (int j = 0; j <= kQuarterSteps; ++j) {
      const int64_t t = t0 + quarter * kQuarterSteps + j;
      const int64_t at = (t < n ? t : n) * frame_stride;
#pragma unroll
      for (int s = 0; s < 3; ++s) staged[j][s] = source[s][at];
    }
  };
  load_tile(0);

  // first operand: this lane's row, its bin and the phase index r = (m t) mod n of its time, t = 4 ks + quad
  const int64_t row = (int64_t)row_tile * kTile + 16 * wave + l15;
  const int bin = row_bins[row];
  const bool row_live = bin >= 0;
  const int64_t m = row_live ? bin : 0;
  const int part = (int)(row & 1);
  const int64_t advance = (4 * m) % n;
  int64_t phase = (m * quad) % n;
  double wave_value[kKSteps], taper_value[kKSteps];
  auto load_operand = [&](int64_t t0) {
#pragma unroll
    for (int ks = 0; ks < kKSteps; ++ks) {
#ifdef RN_BM_CONSTANT_OPERAND
      taper_value[ks] = 1.0;
      wave_value[ks] = 0.5;
#else
      const int64_t t = t0 + 4 * ks + quad;
      taper_value[ks] = taper[t < n ? t : n - 1];
      wave_value[ks] = table[2 * phase + part];
      phase += advance;
      phase -= phase >= n ? n : 0;
#endif
    }
  };
  load_operand(0);

  f64x4_t acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = f64x4_t{0.0, 0.0, 0.0, 0.0};

  for (int64_t t0 = 0; t0 < n; t0 += kSteps) {
    double av[kKSteps];
#pragma unroll
    for (int ks = 0; ks < kKSteps; ++ks)
      av[ks] = row_live && t0 + 4 * ks + quad < n ? taper_value[ks] * wave_value[ks] : 0.0;
    {
      double *dst = tile + (quarter * kQuarterSteps) * kStride + stage_col;
#pragma unroll
      for (int j = 0; j < kQuarterSteps; ++j) {
        const int64_t t = t0 + quarter * kQuarterSteps + j;
        double d0 = staged[j + 1][0] - staged[j][0], d1 = staged[j + 1][1] - staged[j][1];
        double d2 = staged[j + 1][2] - staged[j][2];
        const double symmetric = 0.5 * (d0 + d1);
        d0 -= rint(d0);
        d1 -= rint(d1);
        d2 -= rint(d2);
        const double step = scale * (d0 * l0 + d1 * l1 + d2 * l2);
        const double v = of_alpha ? symmetric : step;
        dst[j * kStride] = column_live && t < n ? v : 0.0;
      }
    }
    __syncthreads();
    if (t0 + kSteps < n) {
      load_tile(t0 + kSteps);
      load_operand(t0 + kSteps);
    }
    const double *b = tile + quad * kStride + l15;
#pragma unroll
    for (int ks = 0; ks < kKSteps; ++ks)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[ks], b[4 * ks * kStride + 16 * c], acc[c], 0, 0, 0);
    __syncthreads();  // the next k-tile's series are written over these
  }

  double *out = V + (segment * Rp + (int64_t)row_tile * kTile + 16 * wave) * Kp + (int64_t)column_tile * kTile;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) out[(4 * j + quad) * Kp + 16 * c + l15] = acc[c][j];
}

// V [rows][Kp], rows a multiple of 64; weights [B][Rp]; ws [chunk][b][pair][64][64]
__global__ void __launch_bounds__(kThreads)
    band_update_kernel(const double *__restrict__ V, int64_t rows, int64_t Rp, int64_t Kp,
                       const double *__restrict__ weights, int pairs, double *__restrict__ ws) {
  __shared__ double tile[2 * kPlane];  // [side][row][column], row stride 80
  const int chunk = blockIdx.x / pairs, pair = blockIdx.x % pairs;
  const int64_t b = blockIdx.y;
  int I, J;
  lower_pair(pair, I, J);
  const int64_t row0 = (int64_t)chunk * kBandChunkRows;
  const int64_t nrows = std::min<int64_t>(kBandChunkRows, rows - row0);  // a multiple of 16
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, quad = lane >> 4;

  // staging: thread (side, half, column) keeps its column of 8 rows, and their weights, in registers
  const int side = threadIdx.x >> 7, half = (threadIdx.x >> 6) & 1, stage_col = threadIdx.x & 63;
  const double *source = V + row0 * Kp + (int64_t)(side ? J : I) * kTile + stage_col;
  const double *weight_row = weights + b * Rp;
  double staged[kHalfRows], staged_weight[kHalfRows];
  auto load_tile = [&](int64_t t0) {  // rows t0 + 8 half .. + 7 of the chunk
#pragma unroll
    for (int j = 0; j < kHalfRows; ++j) {
      const int64_t t = t0 + half * kHalfRows + j;
      staged[j] = source[t * Kp];
      staged_weight[j] = weight_row[(row0 + t) % Rp];
    }
  };
  load_tile(0);

  f64x4_t acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = f64x4_t{0.0, 0.0, 0.0, 0.0};

  for (int64_t t0 = 0; t0 < nrows; t0 += kSteps) {
    {
      double *dst = tile + side * kPlane + (half * kHalfRows) * kStride + stage_col;
#pragma unroll
      for (int j = 0; j < kHalfRows; ++j) dst[j * kStride] = side ? staged[j] : staged_weight[j] * staged[j];
    }
    __syncthreads();
    if (t0 + kSteps < nrows) load_tile(t0 + kSteps);
    const double *a = tile + quad * kStride + 16 * wave + l15;  // side 0: tile I, weighted
    const double *bb = tile + kPlane + quad * kStride + l15;     // side 1: tile J
#pragma unroll
    for (int ks = 0; ks < kKSteps; ++ks) {
      const double av = a[4 * ks * kStride];
#pragma unroll
      for (int c = 0; c < 4; ++c)
        acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bb[4 * ks * kStride + 16 * c], acc[c], 0, 0, 0);
    }
    __syncthreads();  // the next k-tile's rows are written over these
  }

  double *out = ws + (((int64_t)chunk * gridDim.y + b) * pairs + pair) * (kTile * kTile);
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) out[(16 * wave + 4 * j + quad) * kTile + 16 * c + l15] = acc[c][j];
}

// moments [B][Kc][Kc]
__global__ void __launch_bounds__(kThreads)
    band_reduce_kernel(const double *__restrict__ ws, int chunks, int pairs, int64_t Kc, int accumulate,
                       double *__restrict__ moments) {
  __shared__ double mirror[kTile * kMirrorStride];
  const int pair = blockIdx.x;
  const int64_t b = blockIdx.y, B = gridDim.y;
  int I, J;
  lower_pair(pair, I, J);
  double *out = moments + b * Kc * Kc;
  const int64_t row0 = (int64_t)I * kTile, col0 = (int64_t)J * kTile;
  for (int q = 0; q < kTile * kTile / kThreads; ++q) {
    const int e = threadIdx.x + kThreads * q;
    const int r = e / kTile, c = e % kTile;
    const double *p = ws + (b * pairs + pair) * (kTile * kTile) + e;
    double sum = 0.0;
    for (int chunk = 0; chunk < chunks; ++chunk) {
      sum += *p;
      p += B * pairs * (kTile * kTile);
    }
    const bool mine = row0 + r < Kc && col0 + c < Kc && (I != J || c <= r);
    if (mine && accumulate) sum = out[(row0 + r) * Kc + col0 + c] + sum;
    mirror[r * kMirrorStride + c] = sum;
    if (mine) out[(row0 + r) * Kc + col0 + c] = sum;
  }
  __syncthreads();
  for (int q = 0; q < kTile * kTile / kThreads; ++q) {
    const int e = threadIdx.x + kThreads * q;
    const int r = e / kTile, c = e % kTile;  // of the mirrored tile: row in J, column in I
    if (col0 + r < Kc && row0 + c < Kc && (I != J || c > r)) out[(col0 + r) * Kc + row0 + c] = mirror[c * kMirrorStride + r];
  }
}

}  // namespace

int64_t band_padded(int64_t count) { return (count + kTile - 1) / kTile * kTile; }

int band_pairs(int64_t Kc) {
  const int64_t tiles = (Kc + kTile - 1) / kTile;
  return (int)(tiles * (tiles + 1) / 2);
}

int64_t band_chunks(int64_t rows) { return (rows + kBandChunkRows - 1) / kBandChunkRows; }

size_t band_partial_doubles(int64_t Kc, int64_t B, int64_t rows) {
  return (size_t)band_chunks(rows) * (size_t)B * (size_t)band_pairs(Kc) * (kTile * kTile);
}

int64_t band_transform_workgroups(int64_t Kc, int64_t Rp, int64_t count) {
  const int64_t tiles = (band_padded(Kc) / kTile) * (Rp / kTile);
  return count > INT32_MAX / tiles ? -1 : tiles * count;
}

void launch_band_phases(int64_t n, double *table, hipStream_t st) {
  band_phase_kernel<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, st>>>(n, table);
}

void launch_band_transform(const double *pos, const double *alpha, const double *lattice, const double *sqrt_mass,
                           int64_t K, int64_t Kc, int64_t n, const int64_t *starts, int64_t q0, int64_t count,
                           const double *taper, const double *table, const int *row_bins, int64_t Rp, double *V,
                           hipStream_t st) {
  BandLattice cell;
  std::copy_n(lattice, 9, cell.l);
  const int64_t Kp = band_padded(Kc);
  const int row_tiles = (int)(Rp / kTile), column_tiles = (int)(Kp / kTile);
  band_transform_kernel<<<(unsigned)band_transform_workgroups(Kc, Rp, count), kThreads, 0, st>>>(
      pos, alpha, cell, sqrt_mass, K, Kc, n, starts, q0, taper, table, row_bins, row_tiles, column_tiles, Rp, Kp, V);
}

void launch_band_update(const double *V, int64_t rows, int64_t Rp, int64_t Kc, const double *weights, int64_t B,
                        int accumulate, double *ws, double *moments, hipStream_t st) {
  const int pairs = band_pairs(Kc);
  const int chunks = (int)band_chunks(rows);
  band_update_kernel<<<dim3((unsigned)(chunks * pairs), (unsigned)B), kThreads, 0, st>>>(V, rows, Rp, band_padded(Kc),
                                                                                        weights, pairs, ws);
  band_reduce_kernel<<<dim3((unsigned)pairs, (unsigned)B), kThreads, 0, st>>>(ws, chunks, pairs, Kc, accumulate, moments);
}

}  // namespace rn
