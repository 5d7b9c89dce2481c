// Harmonic trajectories (include/rn_harmonic.h; the definition is synthesize_host of ramannoodle_amd/harmonic.py): the
// wrapped fractional positions of atoms that move along harmonic modes,
//   out[r][t][j] = wrap(ref[j] + sum_m amp[r][m] cos(omega_dt[m] (t0 + t) + phase[r][m]) D[m][j]),   wrap(y) = y - floor(y).
//
// harmonic_synthesis_kernel: the product [frames x modes] . [modes x K] (K = 3N) on v_mfma_f64_16x16x4_f64 with the modes
// as the contraction dimension.  A workgroup (4 waves) owns kFrames = 64 frames of one run against kColumns = 128
// columns; wave v holds frames 16 v .. 16 v + 15 against the 128 columns: eight accumulators of the instruction.  It
// walks the modes in ascending k-tiles of kModes = 16 (4 k-steps of the instruction).
// First operand: lane (l15, quad) holds frame 16 v + l15, mode 4 ks + quad, and makes that value itself, in registers:
// theta = omega_dt[m] * (double)(t0 + t) + phase[r][m] as one rounded product and one rounded sum (rounded_angle, compiled
// with contraction off: an fma would round once, and at t0 = 2^40 one ulp of theta is 5e-4 rad; __dmul_rn and __dadd_rn
// are plain operators here and do contract), so theta has the bits of the host statement, then amp[r][m] * cos(theta)
// with the accurate library cosine.  The operand never exists in memory; each of its values feeds eight instructions.
// omega_dt, amp and phase of a k-tile go through LDS ([3][16], loaded by threads 0 .. 47, read as broadcasts).
// Second operand: the same mode of column 16 c + l15, from an LDS tile [mode][column] of D with a row stride of 144
// doubles: as in kernels_covariance.hip an operand read (eight bytes a lane) is served in two groups of 32 lanes, two
// modes (quads) x sixteen columns, whose doubles start at banks 2 l15 and 2 l15 + 32 of the 64 and touch every bank
// once; the staging writes are contiguous along the columns.  Thread (half = thread / 128, column = thread % 128) loads
// its column of 8 consecutive modes of D (global memory, L2-resident: every workgroup of a column tile reads the same
// rows); the rows of the next k-tile are requested before the products of this one.  Result register j of lane (l15,
// quad) is frame 4 j + quad, column l15 (the layout of mode_increment_kernel, tools/mfma_f64_layout_probe.hip).
// The remainders of M and K are zeros in LDS and in the first operand; loads are unconditional from clamped addresses (a
// column past K reads column 0, a mode past M reads mode M - 1), with the zero selected afterwards: nothing is read past
// an array.  Frames past T are computed and not stored.
// Epilogue: in two halves of 64 columns a wave puts its 16 x 64 results into its own LDS rows (row stride 80) and reads
// them back a frame at a time, lane = column: it adds ref, wraps and stores 512 contiguous bytes of the frame.
// No atomics: the sum over the modes runs in ascending k-steps of four from zero, an order that depends on M alone, and
// a frame's value depends on its absolute index t0 + t, not on where the frame lies in a tile or a call.
// RN_HT_CONSTANT_COSINE (a timing variant, tools/harmonic_trajectory_timing.py): the cosine is replaced by 0.5.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"

namespace rn {

namespace {

constexpr int kFrames = 64;                 // frames per workgroup: 16 per wave
constexpr int kColumns = 128;               // columns per workgroup
constexpr int kModes = 16;                  // modes per k-tile
constexpr int kStride = kColumns + 16;      // LDS row stride of the D tile in doubles (see the head of this file)
constexpr int kKSteps = kModes / 4;         // k-steps of the 16x16x4 instruction per k-tile
constexpr int kHalfModes = kModes / 2;      // modes a stager owns per k-tile
constexpr int kColumnBlocks = kColumns / 16;  // accumulators per wave
constexpr int kThreads = 256;
constexpr int kEpilogueColumns = 64;        // columns per epilogue pass: one per lane
constexpr int kEpilogueStride = kEpilogueColumns + 16;
constexpr int kTileDoubles = kModes * kStride;
constexpr int kEpilogueDoubles = (kThreads / 64) * 16 * kEpilogueStride;
constexpr int kSharedDoubles = kTileDoubles > kEpilogueDoubles ? kTileDoubles : kEpilogueDoubles;

typedef double f64x4_t __attribute__((ext_vector_type(4)));

// omega_dt * time + phase with two roundings
__device__ inline double rounded_angle(double omega_dt, double time, double phase) {
#pragma clang fp contract(off)
  const double product = omega_dt * time;
  return product + phase;
}

__global__ void __launch_bounds__(kThreads)
    harmonic_synthesis_kernel(const double *__restrict__ ref, const double *__restrict__ D,
                              const double *__restrict__ omega_dt, const double *__restrict__ amp,
                              const double *__restrict__ phase, int64_t K, int M, int64_t T, int64_t t0, int column_tiles,
                              int64_t frame_tiles, double *__restrict__ out) {
  __shared__ double tile[kSharedDoubles];      // D [mode][column], row stride 144; the epilogue's rows afterwards
  __shared__ double parameters[3 * kModes];    // omega_dt, amp, phase of the k-tile's modes
  const int column_tile = blockIdx.x % column_tiles;
  const int64_t frame_tile = (blockIdx.x / column_tiles) % frame_tiles, run = (blockIdx.x / column_tiles) / frame_tiles;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, quad = lane >> 4;

  // staging: thread (half, column) keeps its column of 8 modes of D in registers; threads 0 .. 47 a parameter each
  const int half = threadIdx.x >> 7, stage_col = threadIdx.x & (kColumns - 1);
  const int64_t column = (int64_t)column_tile * kColumns + stage_col;
  const bool column_live = column < K;
  const double *source = D + (column_live ? column : 0);
  const int which = threadIdx.x / kModes, stage_mode = threadIdx.x % kModes;  // which < 3: a parameter stager
  const double *parameter_source =
      which == 0 ? omega_dt : (which == 1 ? amp + run * M : phase + run * M);  // (which >= 3: read, not used)
  double staged[kHalfModes], staged_parameter = 0.0;
  auto load_tile = [&](int k0) {  // modes k0 + 8 half .. + 7 of this thread's column
#pragma unroll
    for (int j = 0; j < kHalfModes; ++j) {
      const int m = k0 + half * kHalfModes + j;
      staged[j] = source[(int64_t)(m < M ? m : M - 1) * K];
    }
    const int m = k0 + stage_mode;
    staged_parameter = parameter_source[m < M ? m : M - 1];
  };
  load_tile(0);

  // this lane's frame of the first operand: the absolute index is exact in a double (t0 + T <= 2^53)
  const int64_t frame0 = frame_tile * kFrames + 16 * wave;
  const double time = (double)(t0 + frame0 + l15);

  f64x4_t acc[kColumnBlocks];
#pragma unroll
  for (int c = 0; c < kColumnBlocks; ++c) acc[c] = f64x4_t{0.0, 0.0, 0.0, 0.0};

  for (int k0 = 0; k0 < M; k0 += kModes) {
    {
      double *dst = tile + (half * kHalfModes) * kStride + stage_col;
#pragma unroll
      for (int j = 0; j < kHalfModes; ++j) {
        const int m = k0 + half * kHalfModes + j;
        dst[j * kStride] = column_live && m < M ? staged[j] : 0.0;
      }
      if (which < 3) parameters[which * kModes + stage_mode] = staged_parameter;
    }
    __syncthreads();
    if (k0 + kModes < M) load_tile(k0 + kModes);
    const double *b = tile + quad * kStride + l15;
#pragma unroll
    for (int ks = 0; ks < kKSteps; ++ks) {
      const int k = 4 * ks + quad;
      const double theta = rounded_angle(parameters[k], time, parameters[2 * kModes + k]);
#ifdef RN_HT_CONSTANT_COSINE
      const double cosine = theta == theta ? 0.5 : 0.0;
#else
      const double cosine = cos(theta);
#endif
      const double av = k0 + k < M ? parameters[kModes + k] * cosine : 0.0;
#pragma unroll
      for (int c = 0; c < kColumnBlocks; ++c)
        acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b[4 * ks * kStride + 16 * c], acc[c], 0, 0, 0);
    }
    __syncthreads();  // the next k-tile's rows (after the last one: the epilogue's) are written over these
  }

  double *rows = tile + wave * 16 * kEpilogueStride;  // this wave's 16 frames x 64 columns
  double *const out_run = out + run * T * K;
#pragma unroll
  for (int h = 0; h < kColumns / kEpilogueColumns; ++h) {
#pragma unroll
    for (int c = 0; c < kEpilogueColumns / 16; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) rows[(4 * j + quad) * kEpilogueStride + 16 * c + l15] = acc[h * (kEpilogueColumns / 16) + c][j];
    __syncthreads();
    const int64_t out_column = (int64_t)column_tile * kColumns + h * kEpilogueColumns + lane;
    const bool live = out_column < K;
    const double origin = ref[live ? out_column : 0];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t t = frame0 + i;
      const double y = origin + rows[i * kEpilogueStride + lane];
      if (live && t < T) out_run[t * K + out_column] = y - floor(y);
    }
    __syncthreads();  // the second half's results are written over these
  }
}

}  // namespace

int64_t harmonic_workgroups(int64_t K, int64_t R, int64_t T) {
  const int64_t column_tiles = (K + kColumns - 1) / kColumns, frame_tiles = (T + kFrames - 1) / kFrames;
  const int64_t limit = INT32_MAX;
  if (frame_tiles > limit / column_tiles || R > limit / (column_tiles * frame_tiles)) return -1;
  return column_tiles * frame_tiles * R;
}

void launch_harmonic_synthesis(const double *ref, const double *D, const double *omega_dt, const double *amp,
                               const double *phase, int64_t K, int M, int64_t R, int64_t T, int64_t t0, double *out,
                               hipStream_t st) {
  const int column_tiles = (int)((K + kColumns - 1) / kColumns);
  const int64_t frame_tiles = (T + kFrames - 1) / kFrames;
  harmonic_synthesis_kernel<<<(unsigned)harmonic_workgroups(K, R, T), kThreads, 0, st>>>(
      ref, D, omega_dt, amp, phase, K, M, T, t0, column_tiles, frame_tiles, out);
}

}  // namespace rn
