// Structure descriptors: desc[s][c] = (1 / E) sum_e edge[s][e][c] for the Fe real columns of the final edge embedding
// (include/rn_potgnn.h: rn_potgnn_descriptors), float64 [S][Fe].
//
// edge_pool_kernel: one workgroup (256 threads) per frame, which reads the frame's rows once, as one contiguous block,
// in 16-byte loads (32 bytes of a pair row).  A row is cut into groups of kCols columns -- four floats, two doubles, or
// the eight columns [hi x 8][lo x 8] of a split-f16 pair row, x = hi + lo (the decoding of read_stage, forward.hip) --
// and a row has G = FeP / kCols of them.  Thread t owns group t % G of the rows t / G, t / G + 256 / G, ..: consecutive
// threads read consecutive 16 (32) bytes, whole rows, and every thread keeps to its columns, so it adds its rows in
// ascending order into kCols float64 sums.  The 256 / G partial sums of a column are then added through LDS by one
// thread, in ascending order of their first row.  Padded columns (c >= Fe) are read with their rows and left out of the
// result.  The order of every sum depends on (E, FeP) alone: a frame's descriptor has the same bits whatever batch,
// chunk or lane it was evaluated in, and in whatever order the pipeline keeps its rows only up to rounding (the narrow
// pipeline's rows are in destination order, the same for every frame).  No atomics.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace rn {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxCols = 8;

template <EdgeRows ROWS>
struct Group;
template <>
struct Group<EdgeRows::kFloat32> {
  static constexpr int kCols = 4;
  static constexpr int kBytes = 16;
  __device__ static void add(const char *p, double *sums) {
    const float4 v = *reinterpret_cast<const float4 *>(p);
    sums[0] += (double)v.x, sums[1] += (double)v.y, sums[2] += (double)v.z, sums[3] += (double)v.w;
  }
};
template <>
struct Group<EdgeRows::kFloat64> {
  static constexpr int kCols = 2;
  static constexpr int kBytes = 16;
  __device__ static void add(const char *p, double *sums) {
    const double2 v = *reinterpret_cast<const double2 *>(p);
    sums[0] += v.x, sums[1] += v.y;
  }
};
template <>
struct Group<EdgeRows::kPairs> {
  static constexpr int kCols = 8;
  static constexpr int kBytes = 32;
  __device__ static void add(const char *p, double *sums) {
    union Halves {
      uint4 raw;
      _Float16 h[8];
    } hi, lo;
    hi.raw = *reinterpret_cast<const uint4 *>(p);
    lo.raw = *reinterpret_cast<const uint4 *>(p + 16);
#pragma unroll
    for (int k = 0; k < 8; ++k) sums[k] += (double)((float)hi.h[k] + (float)lo.h[k]);
  }
};

template <EdgeRows ROWS>
__global__ void __launch_bounds__(kThreads)
    edge_pool_kernel(const char *__restrict__ edge, int E, int Fe, int FeP, double *__restrict__ desc) {
  using G = Group<ROWS>;
  __shared__ double partial[kThreads * kMaxCols];
  const int groups = FeP / G::kCols;             // of a row
  const int rows_per_pass = kThreads / groups;   // >= 1: the launcher refuses FeP > 256 kCols
  const int group = threadIdx.x % groups, first_row = threadIdx.x / groups;
  const char *frame = edge + (size_t)blockIdx.x * E * groups * G::kBytes;
  double sums[G::kCols];
#pragma unroll
  for (int k = 0; k < G::kCols; ++k) sums[k] = 0.0;
  if (first_row < rows_per_pass)
#pragma unroll 4  // (four rows' loads in flight; the additions keep their order)
    for (int row = first_row; row < E; row += rows_per_pass) G::add(frame + ((size_t)row * groups + group) * G::kBytes, sums);
#pragma unroll
  for (int k = 0; k < G::kCols; ++k) partial[threadIdx.x * G::kCols + k] = sums[k];
  __syncthreads();
  for (int c = threadIdx.x; c < Fe; c += kThreads) {
    double sum = 0.0;
    for (int j = 0; j < rows_per_pass; ++j) sum += partial[(j * groups + c / G::kCols) * G::kCols + c % G::kCols];
    desc[(size_t)blockIdx.x * Fe + c] = sum / (double)E;
  }
}

}  // namespace

bool edge_pool_supported(EdgeRows rows, int FeP) {
  const int cols = rows == EdgeRows::kFloat32 ? 4 : rows == EdgeRows::kFloat64 ? 2 : 8;
  return FeP >= cols && FeP % cols == 0 && FeP / cols <= kThreads;
}

void launch_edge_pool(const void *edge, EdgeRows rows, int S, int E, int Fe, int FeP, double *desc, hipStream_t st) {
  if (S == 0 || E == 0) return;
  const char *p = static_cast<const char *>(edge);
  if (rows == EdgeRows::kFloat32) edge_pool_kernel<EdgeRows::kFloat32><<<S, kThreads, 0, st>>>(p, E, Fe, FeP, desc);
  else if (rows == EdgeRows::kFloat64) edge_pool_kernel<EdgeRows::kFloat64><<<S, kThreads, 0, st>>>(p, E, Fe, FeP, desc);
  else edge_pool_kernel<EdgeRows::kPairs><<<S, kThreads, 0, st>>>(p, E, Fe, FeP, desc);
}

}  // namespace rn
