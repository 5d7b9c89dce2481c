// Nearest reference row and farthest-point selection (include/rn_select.h; the definition is nearest_host and
// select_farthest_host of ramannoodle_amd/selection.py).  With x' = (x - center) scale, d2(x, r) = |x' - r'|^2.
//
// select_search_kernel: the products x'.r' on v_mfma_f64_16x16x4_f64, in the manner of covariance_chunk_kernel.  A
// workgroup (4 waves) owns one tile of kSelectTile = 64 rows of X and one ascending range of whole tiles of R
// (blockIdx.y); it walks the range tile by tile and the columns in k-tiles of kCols = 16 (4 k-steps of the
// instruction).  Per k-tile, thread (side = thread / 128: X or R; row = thread / 2 % 64; half = thread % 2) loads the 8
// consecutive columns 8 half .. 8 half + 7 of its row, applies (v - center) scale and writes them to LDS: the
// transformed operands never exist in HBM.  LDS is [side][column][row] with a row stride of 80 doubles (the operand
// reads of covariance_chunk_kernel: every bank once).  The columns of the next k-tile are requested before the products
// of this one.  The remainders of D and of the rows are zeros in LDS; loads are unconditional from clamped addresses (a
// column past D reads column 0, a row past the array reads row 0), with the zero selected afterwards: nothing is read
// past an array.  Wave v holds rows 16 v .. 16 v + 15 of the tile of X against the 64 rows of the tile of R: four
// accumulators.  First operand: lane (l15, quad) holds column 4 ks + quad of row 16 v + l15 of X; second operand: the
// same column of row 16 c + l15 of R; result register j of lane (l15, quad) is (row 4 j + quad of X, row l15 of R).
// After the last k-tile of a tile of R a lane compares key = |r'|^2 - 2 x'.r' of its 16 results with the running (key,
// index) of its four rows of X, strictly less: a lane meets its rows of R in ascending order, so equal keys keep the
// lowest index.  |x'|^2 is the same for every row of R and left out.  A key is the same sequence of operations
// whichever lane, tile or range its row of R lies in: exact duplicates tie bit for bit.  At the end the sixteen lanes
// of a quad are merged by butterfly shuffles under a total order (key, then index), and lane l15 = 0 writes
// partials[range][row].
// select_merge_kernel: eight lanes per row of X walk the ranges in ascending order (strictly less: the lowest index),
// then recompute the winner's d2 from differences: lane l of the eight sums the columns l, l + 8, .. in ascending order
// and the eight sums are added by a butterfly (4, 2, 1), the same bits on every lane.
//
// select_pick_kernel: one launch per pick.  Every workgroup reduces the partials of the launch before it (thread t
// walks the entries t, t + 256, .. in ascending order, then an LDS tree under the total order value descending, index
// ascending: every workgroup finds the same pick); workgroup 0 records it; then the workgroup updates mind of its slice
// of kSelectSliceRows = 128 rows (eight lanes a row, as above) and writes its slice's highest (mind, row) to the other
// partial buffer.  A picked row gets mind = -1, below every distance, so it is not picked again while others remain.
// No workgroup waits for another, and there are no atomics: launch order on the stream is the only synchronisation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>

#include "kernels.hpp"

namespace rn {

namespace {

constexpr int kTile = kSelectTile;
constexpr int kCols = 16;               // columns per k-tile
constexpr int kStride = kTile + 16;     // LDS row stride in doubles
constexpr int kKSteps = kCols / 4;      // k-steps of the 16x16x4 instruction per k-tile
constexpr int kHalfCols = kCols / 2;    // columns a stager owns per k-tile
constexpr int kThreads = 256;
constexpr int kPlane = kCols * kStride;  // doubles of one side
constexpr int kTargetWorkgroups = 256;   // what the split of a long reference aims at: one workgroup per compute unit

typedef double f64x4_t __attribute__((ext_vector_type(4)));

__device__ inline bool lower_key(double value, int64_t index, double other_value, int64_t other_index) {
  // is (other) ahead of (this) in a search: a smaller key, or the same key at a lower index; "none" (-1) is never ahead
  return other_index >= 0 && (index < 0 || other_value < value || (other_value == value && other_index < index));
}

__device__ inline bool higher_value(double value, int64_t index, double other_value, int64_t other_index) {
  // is (other) ahead of (this) in a pick: a larger value, or the same value at a lower index
  return other_index >= 0 && (index < 0 || other_value > value || (other_value == value && other_index < index));
}

// d2 of two rows by the eight lanes l8 = 0..7 of a group, all of which must be active; the same bits on each of them
__device__ inline double row_distance8(const double *__restrict__ a, const double *__restrict__ b,
                                       const double *__restrict__ scale, int64_t D, int l8) {
  double sum = 0.0;
  for (int64_t c = l8; c < D; c += 8) {
    const double t = (a[c] - b[c]) * scale[c];
    sum = fma(t, t, sum);
  }
  sum += __shfl_xor(sum, 4);
  sum += __shfl_xor(sum, 2);
  sum += __shfl_xor(sum, 1);
  return sum;
}

__global__ void __launch_bounds__(kThreads)
    select_norms_kernel(const double *__restrict__ R, int64_t M, int64_t D, const double *__restrict__ params,
                        double *__restrict__ norms) {
  const int64_t row = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (row >= M) return;
  const double *r = R + row * D;
  double sum = 0.0;
  for (int64_t c = 0; c < D; ++c) {
    const double t = (r[c] - params[c]) * params[D + c];
    sum = fma(t, t, sum);
  }
  norms[row] = sum;
}

__global__ void __launch_bounds__(kThreads)
    select_search_kernel(const double *__restrict__ X, int64_t S, const double *__restrict__ R, int64_t M, int64_t D,
                         const double *__restrict__ params, const double *__restrict__ norms, int exclude_self,
                         int64_t tiles_per_split, SelectBest *__restrict__ partials) {
  __shared__ double tile[2 * kPlane];  // [side][column][row], row stride 80
  const int64_t x_tile = blockIdx.x, split = blockIdx.y;
  const int64_t r_tiles = (M + kTile - 1) / kTile;
  const int64_t tile0 = split * tiles_per_split, tile1 = std::min(tile0 + tiles_per_split, r_tiles);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, quad = lane >> 4;
  const double *center = params, *scale = params + D;

  // staging: thread (side, row, half) keeps its 8 columns of the next k-tile in registers
  const int side = threadIdx.x >> 7, stage_row = (threadIdx.x & 127) >> 1, half = threadIdx.x & 1;
  const int64_t k_tiles = (D + kCols - 1) / kCols;
  double staged[kHalfCols];
  auto load_tile = [&](int64_t r_tile, int64_t k_tile) {
    const int64_t row = (side ? r_tile : x_tile) * kTile + stage_row;
    const bool row_live = row < (side ? M : S);
    const double *source = (side ? R : X) + (row_live ? row : 0) * D;
#pragma unroll
    for (int j = 0; j < kHalfCols; ++j) {
      const int64_t c = k_tile * kCols + half * kHalfCols + j;
      const bool live = row_live && c < D;
      const int64_t cc = c < D ? c : 0;
      const double v = (source[cc] - center[cc]) * scale[cc];
      staged[j] = live ? v : 0.0;
    }
  };

  SelectBest best[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) best[j] = SelectBest{std::numeric_limits<double>::infinity(), -1};
  f64x4_t acc[4];

  if (tile0 < tile1) load_tile(tile0, 0);
  for (int64_t r_tile = tile0; r_tile < tile1; ++r_tile) {
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = f64x4_t{0.0, 0.0, 0.0, 0.0};
    for (int64_t k_tile = 0; k_tile < k_tiles; ++k_tile) {
      {
        double *dst = tile + side * kPlane + (half * kHalfCols) * kStride + stage_row;
#pragma unroll
        for (int j = 0; j < kHalfCols; ++j) dst[j * kStride] = staged[j];
      }
      __syncthreads();
      if (k_tile + 1 < k_tiles) load_tile(r_tile, k_tile + 1);
      else if (r_tile + 1 < tile1) load_tile(r_tile + 1, 0);
      const double *a = tile + quad * kStride + 16 * wave + l15;  // side 0: X
      const double *b = tile + kPlane + quad * kStride + l15;     // side 1: R
#pragma unroll
      for (int ks = 0; ks < kKSteps; ++ks) {
        const double av = a[4 * ks * kStride];
#pragma unroll
        for (int c = 0; c < 4; ++c)
          acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b[4 * ks * kStride + 16 * c], acc[c], 0, 0, 0);
      }
      __syncthreads();  // the next k-tile is written over this one
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t r = r_tile * kTile + 16 * c + l15;
      const double norm = norms[r < M ? r : 0];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t x_row = x_tile * kTile + 16 * wave + 4 * j + quad;
        const double key = norm - 2.0 * acc[c][j];
        const bool valid = r < M && !(exclude_self && r == x_row);
        if (valid && (best[j].index < 0 || key < best[j].value)) best[j] = SelectBest{key, r};
      }
    }
  }

#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int mask = 1; mask < 16; mask <<= 1) {
      const double other_value = __shfl_xor(best[j].value, mask);
      const int64_t other_index = __shfl_xor((long long)best[j].index, mask);
      if (lower_key(best[j].value, best[j].index, other_value, other_index)) best[j] = SelectBest{other_value, other_index};
    }
    const int64_t x_row = x_tile * kTile + 16 * wave + 4 * j + quad;
    if (l15 == 0 && x_row < S) partials[split * S + x_row] = best[j];
  }
}

__global__ void __launch_bounds__(kThreads)
    select_merge_kernel(const double *__restrict__ X, int64_t S, const double *__restrict__ R, int64_t D,
                        const double *__restrict__ params, const SelectBest *__restrict__ partials, int64_t splits,
                        double *__restrict__ dist2, int64_t *__restrict__ index) {
  const int l8 = threadIdx.x & 7;
  const int64_t row = (int64_t)blockIdx.x * (kThreads / 8) + (threadIdx.x >> 3);
  const int64_t s = row < S ? row : 0;  // (every lane stays for the shuffles)
  SelectBest best = partials[s];
  for (int64_t split = 1; split < splits; ++split) {
    const SelectBest other = partials[split * S + s];
    if (other.index >= 0 && (best.index < 0 || other.value < best.value)) best = other;
  }
  const double d2 = row_distance8(X + s * D, R + (best.index < 0 ? 0 : best.index) * D, params + D, D, l8);
  if (l8 == 0 && row < S) {
    dist2[row] = best.index < 0 ? std::numeric_limits<double>::infinity() : d2;
    index[row] = best.index;
  }
}

// columns [D]: one workgroup a column
__global__ void __launch_bounds__(kThreads)
    select_column_mean_kernel(const double *__restrict__ X, int64_t S, int64_t D, double *__restrict__ mean) {
  __shared__ double sums[kThreads];
  const int64_t column = blockIdx.x;
  double sum = 0.0;
  for (int64_t s = threadIdx.x; s < S; s += kThreads) sum += X[s * D + column];
  sums[threadIdx.x] = sum;
  __syncthreads();
  for (int width = kThreads / 2; width > 0; width >>= 1) {
    if ((int)threadIdx.x < width) sums[threadIdx.x] += sums[threadIdx.x + width];
    __syncthreads();
  }
  if (threadIdx.x == 0) mean[column] = sums[0] / (double)S;
}

__global__ void __launch_bounds__(kThreads)
    select_distance_to_kernel(const double *__restrict__ X, int64_t S, int64_t D, const double *__restrict__ params,
                              const double *__restrict__ point, double *__restrict__ mind) {
  const int l8 = threadIdx.x & 7;
  const int64_t row = (int64_t)blockIdx.x * (kThreads / 8) + (threadIdx.x >> 3);
  const double d2 = row_distance8(X + (row < S ? row : 0) * D, point, params + D, D, l8);
  if (l8 == 0 && row < S) mind[row] = d2;
}

__global__ void __launch_bounds__(kThreads) select_fill_kernel(double *__restrict__ mind, int64_t S, double value) {
  const int64_t row = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (row < S) mind[row] = value;
}

// the highest candidate of the workgroup's threads, in every thread (`shared`: kThreads entries; ends with a barrier)
__device__ inline SelectBest highest_of_workgroup(SelectBest mine, SelectBest *shared) {
  shared[threadIdx.x] = mine;
  __syncthreads();
  for (int width = kThreads / 2; width > 0; width >>= 1) {
    if ((int)threadIdx.x < width) {
      const SelectBest a = shared[threadIdx.x], b = shared[threadIdx.x + width];
      if (higher_value(a.value, a.index, b.value, b.index)) shared[threadIdx.x] = b;
    }
    __syncthreads();
  }
  const SelectBest result = shared[0];
  __syncthreads();  // (before the array is used again)
  return result;
}

__global__ void __launch_bounds__(kThreads)
    select_argmax_kernel(const double *__restrict__ mind, int64_t S, SelectBest *__restrict__ partials) {
  __shared__ SelectBest shared[kThreads];
  SelectBest mine{0.0, -1};
  const int64_t row = (int64_t)blockIdx.x * kSelectSliceRows + threadIdx.x;
  if (threadIdx.x < kSelectSliceRows && row < S) mine = SelectBest{mind[row], row};
  const SelectBest top = highest_of_workgroup(mine, shared);
  if (threadIdx.x == 0) partials[blockIdx.x] = top;
}

__global__ void __launch_bounds__(kThreads)
    select_pick_kernel(const double *__restrict__ X, int64_t S, int64_t D, const double *__restrict__ params,
                       double *__restrict__ mind, const SelectBest *__restrict__ partials_in, int64_t slices,
                       SelectBest *__restrict__ partials_out, int64_t forced, int first_of_none, int last, int64_t step,
                       int64_t *__restrict__ picks, double *__restrict__ pick_dist2) {
  __shared__ SelectBest shared[kThreads];
  SelectBest pick{std::numeric_limits<double>::infinity(), forced};
  if (forced < 0) {  // (uniform over the grid)
    SelectBest mine{0.0, -1};
    for (int64_t i = threadIdx.x; i < slices; i += kThreads) {
      const SelectBest other = partials_in[i];
      if (higher_value(mine.value, mine.index, other.value, other.index)) mine = other;
    }
    pick = highest_of_workgroup(mine, shared);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    picks[step] = pick.index;
    pick_dist2[step] = first_of_none ? std::numeric_limits<double>::infinity() : pick.value;
  }
  if (last || pick.index < 0) return;  // (uniform over the grid)

  const int l8 = threadIdx.x & 7, group = threadIdx.x >> 3;
  const double *chosen = X + pick.index * D;
  SelectBest mine{0.0, -1};
#pragma unroll
  for (int i = 0; i < kSelectSliceRows / (kThreads / 8); ++i) {
    const int64_t row = (int64_t)blockIdx.x * kSelectSliceRows + group + (kThreads / 8) * i;
    const int64_t s = row < S ? row : 0;  // (every lane stays for the shuffles)
    const double d2 = row_distance8(X + s * D, chosen, params + D, D, l8);
    if (l8 == 0 && row < S) {
      double m = first_of_none ? d2 : fmin(mind[row], d2);
      if (row == pick.index) m = -1.0;
      mind[row] = m;
      if (higher_value(mine.value, mine.index, m, row)) mine = SelectBest{m, row};
    }
  }
  const SelectBest top = highest_of_workgroup(mine, shared);
  if (threadIdx.x == 0) partials_out[blockIdx.x] = top;
}

}  // namespace

void select_splits(int64_t S, int64_t M, int64_t *splits, int64_t *tiles_per_split) {
  const int64_t x_tiles = std::max<int64_t>(1, (S + kTile - 1) / kTile), r_tiles = std::max<int64_t>(1, (M + kTile - 1) / kTile);
  const int64_t wanted = std::min(r_tiles, std::max<int64_t>(1, (kTargetWorkgroups + x_tiles - 1) / x_tiles));
  *tiles_per_split = (r_tiles + wanted - 1) / wanted;
  *splits = (r_tiles + *tiles_per_split - 1) / *tiles_per_split;
}

void launch_select_norms(const double *R, int64_t M, int64_t D, const double *params, double *norms, hipStream_t st) {
  select_norms_kernel<<<(unsigned)((M + kThreads - 1) / kThreads), kThreads, 0, st>>>(R, M, D, params, norms);
}

void launch_select_search(const double *X, int64_t S, const double *R, int64_t M, int64_t D, const double *params,
                          const double *norms, int exclude_self, SelectBest *partials, hipStream_t st) {
  int64_t splits, tiles_per_split;
  select_splits(S, M, &splits, &tiles_per_split);
  select_search_kernel<<<dim3((unsigned)((S + kTile - 1) / kTile), (unsigned)splits), kThreads, 0, st>>>(
      X, S, R, M, D, params, norms, exclude_self, tiles_per_split, partials);
}

void launch_select_merge(const double *X, int64_t S, const double *R, int64_t M, int64_t D, const double *params,
                         const SelectBest *partials, double *dist2, int64_t *index, hipStream_t st) {
  int64_t splits, tiles_per_split;
  select_splits(S, M, &splits, &tiles_per_split);
  const int rows = kThreads / 8;
  select_merge_kernel<<<(unsigned)((S + rows - 1) / rows), kThreads, 0, st>>>(X, S, R, D, params, partials, splits, dist2,
                                                                              index);
}

void launch_select_column_mean(const double *X, int64_t S, int64_t D, double *mean, hipStream_t st) {
  select_column_mean_kernel<<<(unsigned)D, kThreads, 0, st>>>(X, S, D, mean);
}

void launch_select_distance_to(const double *X, int64_t S, int64_t D, const double *params, const double *point,
                               double *mind, hipStream_t st) {
  const int rows = kThreads / 8;
  select_distance_to_kernel<<<(unsigned)((S + rows - 1) / rows), kThreads, 0, st>>>(X, S, D, params, point, mind);
}

void launch_select_fill(double *mind, int64_t S, double value, hipStream_t st) {
  select_fill_kernel<<<(unsigned)((S + kThreads - 1) / kThreads), kThreads, 0, st>>>(mind, S, value);
}

int64_t select_slices(int64_t S) { return (S + kSelectSliceRows - 1) / kSelectSliceRows; }

void launch_select_argmax(const double *mind, int64_t S, SelectBest *partials, hipStream_t st) {
  select_argmax_kernel<<<(unsigned)select_slices(S), kThreads, 0, st>>>(mind, S, partials);
}

void launch_select_pick(const double *X, int64_t S, int64_t D, const double *params, double *mind,
                        const SelectBest *partials_in, SelectBest *partials_out, int64_t forced, int first_of_none, int last,
                        int64_t step, int64_t *picks, double *pick_dist2, hipStream_t st) {
  const int64_t slices = select_slices(S);
  select_pick_kernel<<<(unsigned)slices, kThreads, 0, st>>>(X, S, D, params, mind, partials_in, slices, partials_out, forced,
                                                            first_of_none, last, step, picks, pick_dist2);
}

}  // namespace rn
