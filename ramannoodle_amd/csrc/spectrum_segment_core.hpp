// What the segment reducers share (spectrum_segments.hip: segments on a hop grid; spectrum_ensemble.hip: segments from a
// start table, whole and by atom group; spectrum_vdos.hip: the density of states, which takes the plans and the back
// half; spectrum_mode_vdos.hip: the density of states by mode; spectrum_modes.hip: the self-spectra of many channels of
// increments; spectrum_mode_matrix.hip: their band-summed pair spectra, which takes the channel builder, the table
// check and the upload helper): the two power kernels of the whole spectra, the plans and work buffers of one (device, n, series per segment, segments per block, rows per block), the workspace arithmetic
// that chooses the two block sizes, the loop that fits plans of those sizes into a workspace limit (get_segment_plans,
// for any block chooser), and the pipeline from the transformed segments to the host rows; for the start-table reducers
// also the check of the table and the upload helper, and the table builder of the whole spectra, which
// spectrum_replicates.hip (replicate combinations of the segments' spectra) takes with the plans and the back half.
// A reducer brings its segment builder (and, but for the whole spectra, its own power kernels) and its own PlanCache,
// so the caches stay apart.  What only the two reducers that read positions share is in spectrum_steps.hpp.
//
// A segment is `series` zero-padded real series of length L (6 components; 6 G for G atom groups) and yields `rows` rows
// (K configurations; K G(G+1)/2 for the atom-group form).  Per block of B segments:
//   segment builder: x[B][series][L] -> series * B batched forward FFTs of length L -> the power kernel:
//     average = 0: p[r][f] = P_r(f) for a sub-block of the block's rows r = (segment, row of the segment)
//     average = 1: pbar[r][f] += P_r(f) / Q over the block's segments, in segment order, no atomics
//   -> (per sub-block of rows, or once on pbar after the last block) batched inverse of length L -> positive lags, scaled
//   by 1/L, in place -> batched forward of length n (stride L, in place) -> real bins 1..bins, copied to the host rows.
// When the rows of pbar do not fit (rows > R), they go through in blocks of R; if the segments do not fit one block either
// (Q > B), they are transformed again for every block of rows.
#pragma once
#include <utility>
#include <vector>

#include "spectrum_common.hpp"

namespace rn_spectrum {

constexpr int kPowerThreads = 256;
constexpr int kRowTile = 16;                              // rows per thread of the power kernels (blockIdx.y)
constexpr int64_t kMaxSegments = 4096;                    // segments per block (gridDim.y of the builder)
constexpr int64_t kMaxRows = 32768;                       // rows per block (gridDim.y of the slot kernels)
constexpr size_t kMaxBlockBytes = (size_t)512 << 20;      // x and p are each kept below this
constexpr int64_t kMaxTableSegments = (int64_t)1 << 31;   // starts of a start table

// Re(X_j conj X_l) of the 21 pairs at one frequency of one segment
__device__ inline void pair_powers(const hipfftDoubleComplex *__restrict__ x, int64_t L, int64_t b, int64_t f,
                                   double *cv) {
  hipfftDoubleComplex v[kComponents];
#pragma unroll
  for (int c = 0; c < kComponents; ++c) v[c] = x[(b * kComponents + c) * L + f];
  int p = 0;
#pragma unroll
  for (int j = 0; j < kComponents; ++j)
#pragma unroll
    for (int l = j; l < kComponents; ++l) cv[p++] = v[j].x * v[l].x + v[j].y * v[l].y;
}

__device__ inline double contract(const double *wk, const double *cv) {
  double acc = 0.0;
#pragma unroll
  for (int p = 0; p < kPairs; ++p) acc = fma(wk[p], cv[p], acc);
  return acc;
}

// average = 0.  Slot j of the sub-block (rows r0 .. r0+count-1 of the segment block, row r = b K + k): P_bk(f); slots
// >= count are zeroed.  Each thread writes one frequency of kRowTile rows and recomputes the pair powers when b changes.
static __global__ void __launch_bounds__(kPowerThreads)
    segment_power_kernel(const hipfftDoubleComplex *__restrict__ x, int64_t L, const double *__restrict__ w, int64_t K,
                         int64_t r0, int count, int slots, hipfftDoubleComplex *__restrict__ p) {
  __shared__ double ws[kRowTile * kPairs];
  const int j0 = blockIdx.y * kRowTile;
  const int nr = std::min(kRowTile, count - j0);  // (may be <= 0: a tile of zeroed slots)
  for (int i = threadIdx.x; i < nr * kPairs; i += blockDim.x)
    ws[i] = w[((r0 + j0 + i / kPairs) % K) * kPairs + i % kPairs];
  __syncthreads();
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= L) return;
  double cv[kPairs];
  int64_t held = -1;
  for (int i = 0; i < kRowTile && j0 + i < slots; ++i) {
    double v = 0.0;
    if (i < nr) {
      const int64_t b = (r0 + j0 + i) / K;
      if (b != held) pair_powers(x, L, b, f, cv);
      held = b;
      v = contract(ws + i * kPairs, cv);
    }
    p[(int64_t)(j0 + i) * L + f] = make_double2(v, 0.0);
  }
}

// average = 1.  Slot i (configuration k0 + i, i < kc): pbar[i][f] (+)= sum over the block's `count` segments, in order, of
// P_bk(f) * inv_q; `first` starts the sum at zero; slots >= kc are zeroed.  One thread owns its (k, f) for the whole call.
static __global__ void __launch_bounds__(kPowerThreads)
    segment_mean_power_kernel(const hipfftDoubleComplex *__restrict__ x, int64_t L, int count,
                              const double *__restrict__ w, int64_t k0, int kc, int slots, double inv_q, int first,
                              hipfftDoubleComplex *__restrict__ pbar) {
  __shared__ double ws[kRowTile * kPairs];
  const int i0 = blockIdx.y * kRowTile;
  const int nr = std::min(kRowTile, kc - i0);
  for (int i = threadIdx.x; i < nr * kPairs; i += blockDim.x) ws[i] = w[(k0 + i0) * kPairs + i];
  __syncthreads();
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= L) return;
  double acc[kRowTile];
#pragma unroll
  for (int i = 0; i < kRowTile; ++i) acc[i] = (first || i >= nr) ? 0.0 : pbar[(int64_t)(i0 + i) * L + f].x;
  for (int b = 0; b < (nr > 0 ? count : 0); ++b) {
    // A compiler barrier: the tile's 16 x 21 weights are read from LDS in every iteration.  Without it the compiler hoists
    // the 336 loop-invariant doubles out of this loop (kernel-resource-usage of the gfx950 build: 256 VGPRs, 980 bytes
    // of scratch per lane, 1 wave per SIMD); with it 122 VGPRs, no scratch, 4 waves per SIMD.
    asm volatile("" ::: "memory");
    double cv[kPairs];
    pair_powers(x, L, b, f, cv);
#pragma unroll
    for (int i = 0; i < kRowTile; ++i)
      if (i < nr) acc[i] = fma(contract(ws + i * kPairs, cv), inv_q, acc[i]);
  }
#pragma unroll
  for (int i = 0; i < kRowTile; ++i)
    if (i0 + i < slots) pbar[(int64_t)(i0 + i) * L + f] = make_double2(acc[i], 0.0);
}

// The builder of the whole spectra from a start table (spectrum_ensemble.hip, spectrum_replicates.hip):
// build_segments_kernel of spectrum_segments.hip with the segment's first step read from starts[q0 + b]
static __global__ void build_segments_at_kernel(const double *__restrict__ alpha, const double *__restrict__ tau,
                                                int64_t n, int64_t L, const int64_t *__restrict__ starts, int64_t q0,
                                                int count, hipfftDoubleComplex *__restrict__ x) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (t >= L) return;
  double s[kComponents] = {0, 0, 0, 0, 0, 0};
  if (t < n && b < count) {
    const double *a0 = alpha + (starts[q0 + b] + t) * 9, *a1 = a0 + 9;
    const double w = tau[t];
    double d[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) d[i] = w * (a1[i] - a0[i]);
    symmetric_components(d, s);
  }
#pragma unroll
  for (int c = 0; c < kComponents; ++c) x[((int64_t)b * kComponents + c) * L + t] = make_double2(s[c], 0.0);
}

constexpr int kFormSize = kComponents * kComponents;

// What the power kernels of the atom-group and the channel reducers share (spectrum_ensemble.hip, spectrum_modes.hip).
// The forms M_k of the tile's `nr` rows (row r0 + i has k = (r / pairs) % K) from the packed weights: diagonal as is,
// off-diagonal halved, as partial_contract_kernel unpacks them
__device__ inline void load_forms(const double *__restrict__ w, int64_t r0, int nr, int pairs, int64_t K, double *ms) {
  for (int i = threadIdx.x; i < nr * kPairs; i += blockDim.x) {
    const int row = i / kPairs, q = i % kPairs;
    const int64_t k = ((r0 + row) / pairs) % K;
    int a, b;
    upper_pair(q, kComponents, a, b);
    const double v = w[k * kPairs + q];
    ms[row * kFormSize + a * kComponents + b] = a == b ? v : 0.5 * v;
    ms[row * kFormSize + b * kComponents + a] = a == b ? v : 0.5 * v;
  }
}

__device__ inline void load_group(const hipfftDoubleComplex *__restrict__ x, int64_t L, hipfftDoubleComplex *v) {
#pragma unroll
  for (int c = 0; c < kComponents; ++c) v[c] = x[c * L];
}

// sum_{c,e} m[c][e] Re(a_c conj b_e), summed as partial_contract_kernel sums it
__device__ inline double contract_groups(const double *m, const hipfftDoubleComplex *a, const hipfftDoubleComplex *b) {
  double v = 0.0;
#pragma unroll
  for (int c = 0; c < kComponents; ++c) {
    double row = 0.0;
#pragma unroll
    for (int e = 0; e < kComponents; ++e) row = fma(m[c * kComponents + e], a[c].x * b[e].x + a[c].y * b[e].y, row);
    v += row;
  }
  return v;
}

constexpr int64_t kMaxChannels = 65535;  // channels per block (gridDim.z of the builder)

// The builder of the channel reducers (spectrum_modes.hip, spectrum_mode_matrix.hip).  Segment b of the block, slot
// cl = blockIdx.z (channel c0 + cl of the C + 1, channel C being the sum of the C): x[b][cl][j][t] for t < n; zero for
// n <= t < L, for b >= count and for cl >= cc
static __global__ void build_channel_segments_kernel(const double *__restrict__ incr, const double *__restrict__ tau,
                                                     int64_t n, int64_t L, int64_t C,
                                                     const int64_t *__restrict__ starts, int64_t q0, int count,
                                                     int64_t c0, int cc, int Cb, hipfftDoubleComplex *__restrict__ x) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y, cl = blockIdx.z;
  if (t >= L) return;
  double s[kComponents] = {0, 0, 0, 0, 0, 0};
  if (t < n && b < count && cl < cc) {
    const double *a = incr + (starts[q0 + b] + t) * C * 9;
    double d[9];
    if (c0 + cl < C) {
#pragma unroll
      for (int i = 0; i < 9; ++i) d[i] = a[(c0 + cl) * 9 + i];
    } else {  // the summed channel
#pragma unroll
      for (int i = 0; i < 9; ++i) d[i] = 0.0;
      for (int64_t c = 0; c < C; ++c)
#pragma unroll
        for (int i = 0; i < 9; ++i) d[i] += a[c * 9 + i];
    }
    const double w = tau[t];
#pragma unroll
    for (int i = 0; i < 9; ++i) d[i] *= w;
    symmetric_components(d, s);
  }
#pragma unroll
  for (int j = 0; j < kComponents; ++j)
    x[(((int64_t)b * Cb + cl) * kComponents + j) * L + t] = make_double2(s[j], 0.0);
}

// plans + work buffers of one (device, n, series, B, R)
struct SegmentPlans {
  int device = -1;
  int64_t n = 0, L = 0;
  int series = 0;    // real series per segment
  int B = 0, R = 0;  // segments per block, rows per block
  DeviceBuffer x, p, out, source, tau, w, starts;
  size_t fixed_bytes = 0;  // x + p + out + the plans' work areas
  FftPlan plan_x, plan_inv, plan_n;
};

// the bytes of B segments' series and R rows' slots and bins, besides the plans' work areas
inline size_t segment_buffer_bytes(int64_t L, int64_t bins, int series, int64_t B, int64_t R) {
  const size_t cz = sizeof(hipfftDoubleComplex);
  return (size_t)B * series * L * cz + (size_t)R * L * cz + (size_t)R * bins * sizeof(double);
}

// (Entry: SegmentPlans, or a reducer's extension of it)
template <class Entry>
int make_segment_plans(PlanCache<Entry> &cache, int device, int64_t n, int series, int B, int R, Entry **out) {
  const int64_t L = padded_length(n), bins = num_bins(n);
  Entry &s = cache.emplace_front();
  s.device = device;
  s.n = n;
  s.L = L;
  s.series = series;
  s.B = B;
  s.R = R;
  const size_t cz = sizeof(hipfftDoubleComplex);
  int rc = RN_OK;
  if (s.x.ensure((size_t)B * series * L * cz) != RN_OK || s.p.ensure((size_t)R * L * cz) != RN_OK ||
      s.out.ensure((size_t)R * bins * sizeof(double)) != RN_OK)
    rc = RN_ERR_OUT_OF_MEMORY;
  else if (!s.plan_x.make((int)L, series * B) || !s.plan_inv.make((int)L, R) || !s.plan_n.make((int)n, R, (int)L))
    rc = RN_ERR_HIP;
  if (rc != RN_OK) {
    cache.drop_front();
    return rc;
  }
  s.fixed_bytes = segment_buffer_bytes(L, bins, series, B, R) + s.plan_x.work_bytes() + s.plan_inv.work_bytes() +
                  s.plan_n.work_bytes();
  *out = &s;
  return RN_OK;
}

inline int64_t balanced(int64_t total, int64_t most) {  // the block size of `total` items in ceil(total / most) even blocks
  const int64_t blocks = (total + most - 1) / most;
  return (total + blocks - 1) / blocks;
}

// B segments per block and R rows per block for `avail` bytes: half each, the rest to whichever can still use it.  A
// segment has `rows` rows.
inline bool choose_segment_blocks(size_t avail, int64_t L, int64_t bins, int series, int64_t Q, int64_t rows, int average,
                                  int *B, int *R) {
  const size_t cz = sizeof(hipfftDoubleComplex);
  const size_t per_segment = (size_t)series * L * cz, per_row = (size_t)L * cz + (size_t)bins * sizeof(double);
  if (avail < per_segment + per_row) return false;
  const int64_t bcap = std::min<int64_t>({Q, kMaxSegments, std::max<int64_t>(1, (int64_t)(kMaxBlockBytes / per_segment))});
  const int64_t rows_most = std::min<int64_t>(kMaxRows, std::max<int64_t>(1, (int64_t)(kMaxBlockBytes / ((size_t)L * cz))));
  auto rcap = [&](int64_t b) { return std::min<int64_t>(rows_most, average ? rows : b * rows); };
  int64_t b = std::max<int64_t>(1, std::min<int64_t>(bcap, (int64_t)(avail / 2 / per_segment)));
  int64_t r = std::max<int64_t>(1, std::min<int64_t>(rcap(b), (int64_t)((avail - b * per_segment) / per_row)));
  b = std::min<int64_t>(bcap, (int64_t)((avail - r * per_row) / per_segment));
  r = std::min<int64_t>(rcap(b), (int64_t)((avail - b * per_segment) / per_row));
  if (b < 1 || r < 1) return false;
  b = balanced(Q, b);
  r = balanced(average ? rows : b * rows, r);
  *B = (int)b;
  *R = (int)r;
  return true;
}

// Finds or creates the entry whose blocks fit `limit` beside `base` bytes (the taper, the weights, a start table, a
// reducer's own arrays).  choose(avail, &series, &B, &R) sets the block sizes for `avail` bytes, or returns false when
// not one block fits; it is asked again, with less, while the plans' work areas do not fit beside the buffers.
template <class Entry, class Choose>
int get_segment_plans(PlanCache<Entry> &cache, int device, int64_t n, size_t limit, size_t base, Choose choose,
                      Entry **out) {
  const int64_t L = padded_length(n), bins = num_bins(n);
  if (limit <= base) return RN_ERR_OUT_OF_MEMORY;
  size_t avail = limit - base;
  for (int attempt = 0; attempt < 4; ++attempt) {
    int series = 0, B = 0, R = 0;
    if (!choose(avail, &series, &B, &R)) return RN_ERR_OUT_OF_MEMORY;
    Entry *s = cache.find([&](const Entry &e) {
      return e.device == device && e.n == n && e.series == series && e.B == B && e.R == R;
    });
    if (!s) {
      int rc = make_segment_plans(cache, device, n, series, B, R, &s);
      if (rc != RN_OK) return rc;
    }
    if (s->fixed_bytes + base <= limit) {
      cache.trim();
      *out = s;
      return RN_OK;
    }
    // the plans' work areas do not fit beside the buffers: they shrink with the blocks, so set their bytes aside
    const size_t work = s->fixed_bytes - segment_buffer_bytes(L, bins, series, B, R);
    cache.drop_front();
    if (limit - base <= work) return RN_ERR_OUT_OF_MEMORY;
    avail = std::min(avail - 1, limit - base - work);
  }
  return RN_ERR_OUT_OF_MEMORY;
}

// ... with choose_segment_blocks: Q segments of `series` series and `rows` rows each
template <class Entry>
int get_segment_plans(PlanCache<Entry> &cache, int device, int64_t n, int series, int64_t Q, int64_t rows, int average,
                      size_t limit, size_t base, Entry **out) {
  const int64_t L = padded_length(n), bins = num_bins(n);
  auto choose = [&](size_t avail, int *s, int *B, int *R) {
    *s = series;
    return choose_segment_blocks(avail, L, bins, series, Q, rows, average, B, R);
  };
  return get_segment_plans(cache, device, n, limit, base, choose, out);
}

// host[count] -> buffer, sized to fit exactly (a buffer that `workspace_limit` counts); a blocking copy
template <class T>
int upload(DeviceBuffer &buffer, const T *host, size_t count) {
  if (int rc = buffer.ensure(count * sizeof(T))) return rc;
  return hipMemcpy(buffer.ptr, host, count * sizeof(T), hipMemcpyHostToDevice) == hipSuccess ? RN_OK : RN_ERR_HIP;
}

// the taper (host [n]) and the weights (host [K][21]) of a call -> s.tau, s.w
inline int upload_taper_and_weights(SegmentPlans &s, const double *taper, const double *weights, int64_t K) {
  if (int rc = upload(s.tau, taper, (size_t)s.n)) return rc;
  return upload(s.w, weights, (size_t)K * kPairs);
}

// The checks of a start table, after an entry's own pointers and sizes and before any device work: W frames per
// segment of a series of `frames` frames, Q starts, each with 0 <= starts[q] <= frames - W.
inline int check_table(int64_t frames, int64_t W, const int64_t *starts, int64_t Q, int average, int64_t bins) {
  if (W < 3 || W > frames || Q < 1 || Q > kMaxTableSegments) return RN_ERR_INVALID_ARGUMENT;
  if (bins != num_bins(W - 1) || (average != 0 && average != 1)) return RN_ERR_INVALID_ARGUMENT;
  for (int64_t q = 0; q < Q; ++q)
    if (starts[q] < 0 || starts[q] > frames - W) return RN_ERR_INVALID_ARGUMENT;
  return RN_OK;
}

// slots of s.p (powers, `count` of them real) -> out: host float64[count][bins]
inline int segment_rows_to_host(SegmentPlans &s, int count, double *out) {
  const int64_t n = s.n, L = s.L, bins = num_bins(n);
  auto *p = s.p.as<hipfftDoubleComplex>();
  if (!s.plan_inv.exec(p, HIPFFT_BACKWARD)) return RN_ERR_HIP;
  slot_lags_kernel<<<dim3(blocks_of_256(n), (unsigned)s.R), 256>>>(p, n, L, 1.0 / (double)L);
  if (!s.plan_n.exec(p, HIPFFT_FORWARD)) return RN_ERR_HIP;
  slot_bins_kernel<<<dim3(blocks_of_256(bins), (unsigned)count), 256>>>(p, L, bins, count, s.out.as<double>());
  if (hipGetLastError() != hipSuccess) return RN_ERR_HIP;
  if (hipMemcpy(out, s.out.ptr, (size_t)count * bins * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
    return RN_ERR_HIP;
  return RN_OK;
}

// Q segments of `rows` rows each -> out: host float64[rows][bins] (average) or [Q][rows][bins]; null stream.
//   build(q0, count):                  launches the builder of segments q0 .. q0+count-1 into s.x (B slots; the rest zeroed)
//   mean_power(count, r0, rc, first):  launches pbar[i] (+)= the mean's share of rows r0 .. r0+rc-1 over `count` segments
//   row_power(r0, rc):                 launches p[j] = row r0 + j of the block (row r = b * rows + row of the segment)
template <class Build, class MeanPower, class RowPower>
int run_segments(SegmentPlans &s, int64_t Q, int64_t rows, int average, Build build, MeanPower mean_power,
                 RowPower row_power, double *out) {
  const int64_t bins = num_bins(s.n);
  const int B = s.B, R = s.R;
  int rc;
  int64_t held = -1;  // the first segment of the block whose transforms x holds
  auto transform_block = [&](int64_t q0, int count) -> int {
    if (held == q0) return RN_OK;
    build(q0, count);
    if (!s.plan_x.exec(s.x.ptr, HIPFFT_FORWARD)) return RN_ERR_HIP;
    held = q0;
    return RN_OK;
  };
  if (average) {
    for (int64_t r0 = 0; r0 < rows; r0 += R) {
      const int count_r = (int)std::min<int64_t>(R, rows - r0);
      for (int64_t q0 = 0; q0 < Q; q0 += B) {
        const int count = (int)std::min<int64_t>(B, Q - q0);
        if ((rc = transform_block(q0, count)) != RN_OK) return rc;
        mean_power(count, r0, count_r, q0 == 0);
      }
      if ((rc = segment_rows_to_host(s, count_r, out + r0 * bins)) != RN_OK) return rc;
    }
    return RN_OK;
  }
  for (int64_t q0 = 0; q0 < Q; q0 += B) {
    const int count = (int)std::min<int64_t>(B, Q - q0);
    if ((rc = transform_block(q0, count)) != RN_OK) return rc;
    const int64_t block_rows = count * rows;
    for (int64_t r0 = 0; r0 < block_rows; r0 += R) {
      const int count_r = (int)std::min<int64_t>(R, block_rows - r0);
      row_power(r0, count_r);
      if ((rc = segment_rows_to_host(s, count_r, out + (q0 * rows + r0) * bins)) != RN_OK) return rc;
    }
  }
  return RN_OK;
}

// the launches of the whole spectra's two power kernels for run_segments (weights in s.w, K configurations)
inline auto whole_mean_power(SegmentPlans &s, int64_t Q) {
  return [&s, Q](int count, int64_t k0, int kc, bool first) {
    const unsigned gl = (unsigned)((s.L + kPowerThreads - 1) / kPowerThreads);
    const unsigned tiles = (unsigned)((s.R + kRowTile - 1) / kRowTile);
    segment_mean_power_kernel<<<dim3(gl, tiles), kPowerThreads>>>(s.x.as<hipfftDoubleComplex>(), s.L, count,
                                                                  s.w.as<const double>(), k0, kc, s.R, 1.0 / (double)Q,
                                                                  first, s.p.as<hipfftDoubleComplex>());
  };
}
inline auto whole_row_power(SegmentPlans &s, int64_t K) {
  return [&s, K](int64_t r0, int rc) {
    const unsigned gl = (unsigned)((s.L + kPowerThreads - 1) / kPowerThreads);
    const unsigned tiles = (unsigned)((s.R + kRowTile - 1) / kRowTile);
    segment_power_kernel<<<dim3(gl, tiles), kPowerThreads>>>(s.x.as<hipfftDoubleComplex>(), s.L, s.w.as<const double>(),
                                                             K, r0, rc, s.R, s.p.as<hipfftDoubleComplex>());
  };
}

}  // namespace rn_spectrum
