// On-device reduction of a polarizability time series to segment-averaged (Welch) and time-resolved MD Raman spectra:
// MDRamanSpectrum.measure_segments / measure_segments_polarized before the laser / Bose-Einstein corrections.
//
// The series alpha[0..S-1] is cut into Q = (S - W) / H + 1 segments of W steps (n = W - 1 differences), segment q starting
// at step q H.  Its tapered differences d_q[t] = tau[t] (alpha[qH + t + 1] - alpha[qH + t]) give the six components
// (xx, yy, zz, xy, yz, xz) of their symmetric part, and row (q, k) is rn_md_raman_polarized's I_k(f) of d_q: with X_c the
// zero-padded transform of component c (length L >= 2n - 1),
//   P_qk(f) = sum_{j<=l} W_k[p(j,l)] Re(X_j(f) conj X_l(f))
// is the transform of the contracted symmetrised cross-correlation (Wiener-Khinchin), and everything after it -- the
// inverse transform, the positive lags, the length-n transform, the real bins -- is linear.  So the mean over the segments
// is taken on P, before the inverse transform: the averaged spectrum costs 6 Q forward transforms and 2 K more, whatever Q.
// Per block of B segments:
//   segment builder: x[B][6][L] from alpha (read in place: overlapping segments re-read it through the caches) -> 6 B
//   batched forward FFTs of length L -> the power / contraction kernel, one thread per frequency and tile of rows:
//     average = 0: p[r][f] = P_qk(f) for a sub-block of the block's rows r = (q, k)
//     average = 1: pbar[k][f] += P_qk(f) / Q over the block's segments, in segment order, no atomics
//   -> (per sub-block of rows, or once on pbar after the last block) batched inverse of length L -> positive lags, scaled
//   by 1/L, in place -> batched forward of length n (stride L, in place) -> real bins 1..bins, copied to the host rows.
// When K rows of pbar do not fit (K > R), the configurations go through in blocks of R; if the segments do not fit one
// block either (Q > B), they are transformed again for every block of configurations: 6 Q ceil(K / R) forward transforms.
// Each tile of 16 rows reads the block's x once, so x is read ceil(R / 16) times per block (from L2 / Infinity Cache while
// the block is small, from HBM beyond that).  The 2 K transforms of the back half exceed the 42 Q of a loop over
// rn_md_raman_polarized when K > 21 Q: the averaged entry then wins on the rows it does not copy, not on transforms.
// float64 throughout; hipFFT is loaded once for the library (spectrum_common.hpp).  Plans and work buffers are cached per
// (device, n, segments per block, rows per block) in a cache of their own, apart from the caches of the other three
// reducers.  All work runs on the null stream (after a synchronise of the caller's stream in the _device entry).
#include "spectrum_common.hpp"

namespace {
using namespace rn_spectrum;

constexpr int kPowerThreads = 256;
constexpr int kRowTile = 16;                              // rows per thread of the power kernels (blockIdx.y)
constexpr int64_t kMaxSegments = 4096;                    // segments per block (gridDim.y of the builder)
constexpr int64_t kMaxRows = 32768;                       // rows per block (gridDim.y of the slot kernels)
constexpr size_t kMaxBlockBytes = (size_t)512 << 20;      // x and p are each kept below this

// segment b of the block (segments q0 .. q0+count-1): x[b][c][t] = tau[t] * component c of the symmetric part of
// alpha[(q0+b)H + t + 1] - alpha[(q0+b)H + t] for t < n; zero for n <= t < L and for b >= count
__global__ void build_segments_kernel(const double *__restrict__ alpha, const double *__restrict__ tau, int64_t n,
                                      int64_t L, int64_t hop, int64_t q0, int count,
                                      hipfftDoubleComplex *__restrict__ x) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (t >= L) return;
  double s[kComponents] = {0, 0, 0, 0, 0, 0};
  if (t < n && b < count) {
    const double *a0 = alpha + ((q0 + b) * hop + t) * 9, *a1 = a0 + 9;
    const double w = tau[t];
    double d[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) d[i] = w * (a1[i] - a0[i]);
    symmetric_components(d, s);
  }
#pragma unroll
  for (int c = 0; c < kComponents; ++c) x[((int64_t)b * kComponents + c) * L + t] = make_double2(s[c], 0.0);
}

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
__global__ void __launch_bounds__(kPowerThreads)
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
__global__ void __launch_bounds__(kPowerThreads)
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

// plans + work buffers of one (device, n, B, R)
struct SegmentPlans {
  int device = -1;
  int64_t n = 0, L = 0;
  int B = 0, R = 0;  // segments per block, rows per block
  DeviceBuffer x, p, out, alpha, tau, w;
  size_t fixed_bytes = 0;  // x + p + out + the plans' work areas
  FftPlan plan_x, plan_inv, plan_n;
};
PlanCache<SegmentPlans> g_segment_cache;  // apart from the other three spectrum caches

// the bytes of B segments' components and R rows' slots and bins, besides the plans' work areas
size_t buffer_bytes(int64_t L, int64_t bins, int64_t B, int64_t R) {
  const size_t cz = sizeof(hipfftDoubleComplex);
  return (size_t)B * kComponents * L * cz + (size_t)R * L * cz + (size_t)R * bins * sizeof(double);
}

int make_plans(int device, int64_t n, int B, int R, SegmentPlans **out) {
  const int64_t L = padded_length(n), bins = num_bins(n);
  SegmentPlans &s = g_segment_cache.emplace_front();
  s.device = device;
  s.n = n;
  s.L = L;
  s.B = B;
  s.R = R;
  const size_t cz = sizeof(hipfftDoubleComplex);
  int rc = RN_OK;
  if (s.x.ensure((size_t)B * kComponents * L * cz) != RN_OK || s.p.ensure((size_t)R * L * cz) != RN_OK ||
      s.out.ensure((size_t)R * bins * sizeof(double)) != RN_OK)
    rc = RN_ERR_OUT_OF_MEMORY;
  else if (!s.plan_x.make((int)L, kComponents * B) || !s.plan_inv.make((int)L, R) || !s.plan_n.make((int)n, R, (int)L))
    rc = RN_ERR_HIP;
  if (rc != RN_OK) {
    g_segment_cache.drop_front();
    return rc;
  }
  s.fixed_bytes = buffer_bytes(L, bins, B, R) + s.plan_x.work_bytes() + s.plan_inv.work_bytes() + s.plan_n.work_bytes();
  *out = &s;
  return RN_OK;
}

int64_t balanced(int64_t total, int64_t most) {  // the block size of `total` items in ceil(total / most) even blocks
  const int64_t blocks = (total + most - 1) / most;
  return (total + blocks - 1) / blocks;
}

// B segments per block and R rows per block for `avail` bytes: half each, the rest to whichever can still use it
bool choose_blocks(size_t avail, int64_t L, int64_t bins, int64_t Q, int64_t K, int average, int *B, int *R) {
  const size_t cz = sizeof(hipfftDoubleComplex);
  const size_t per_segment = (size_t)kComponents * L * cz, per_row = (size_t)L * cz + (size_t)bins * sizeof(double);
  if (avail < per_segment + per_row) return false;
  const int64_t bcap = std::min<int64_t>({Q, kMaxSegments, std::max<int64_t>(1, (int64_t)(kMaxBlockBytes / per_segment))});
  const int64_t rows_most = std::min<int64_t>(kMaxRows, std::max<int64_t>(1, (int64_t)(kMaxBlockBytes / ((size_t)L * cz))));
  auto rcap = [&](int64_t b) { return std::min<int64_t>(rows_most, average ? K : b * K); };
  int64_t b = std::max<int64_t>(1, std::min<int64_t>(bcap, (int64_t)(avail / 2 / per_segment)));
  int64_t r = std::max<int64_t>(1, std::min<int64_t>(rcap(b), (int64_t)((avail - b * per_segment) / per_row)));
  b = std::min<int64_t>(bcap, (int64_t)((avail - r * per_row) / per_segment));
  r = std::min<int64_t>(rcap(b), (int64_t)((avail - b * per_segment) / per_row));
  if (b < 1 || r < 1) return false;
  b = balanced(Q, b);
  r = balanced(average ? K : b * K, r);
  *B = (int)b;
  *R = (int)r;
  return true;
}

// finds or creates the entry whose blocks fit `limit` beside the taper and K configurations' weights
int get_plans(int device, int64_t n, int64_t Q, int64_t K, int average, size_t limit, SegmentPlans **out) {
  const int64_t L = padded_length(n), bins = num_bins(n);
  const size_t base = (size_t)n * sizeof(double) + (size_t)K * kPairs * sizeof(double);
  if (limit <= base) return RN_ERR_OUT_OF_MEMORY;
  size_t avail = limit - base;
  for (int attempt = 0; attempt < 4; ++attempt) {
    int B = 0, R = 0;
    if (!choose_blocks(avail, L, bins, Q, K, average, &B, &R)) return RN_ERR_OUT_OF_MEMORY;
    SegmentPlans *s = g_segment_cache.find(
        [&](const SegmentPlans &e) { return e.device == device && e.n == n && e.B == B && e.R == R; });
    if (!s) {
      int rc = make_plans(device, n, B, R, &s);
      if (rc != RN_OK) return rc;
    }
    if (s->fixed_bytes + base <= limit) {
      g_segment_cache.trim();
      *out = s;
      return RN_OK;
    }
    // the plans' work areas do not fit beside the buffers: they shrink with the blocks, so set their bytes aside
    const size_t work = s->fixed_bytes - buffer_bytes(L, bins, B, R);
    g_segment_cache.drop_front();
    if (limit - base <= work) return RN_ERR_OUT_OF_MEMORY;
    avail = std::min(avail - 1, limit - base - work);
  }
  return RN_ERR_OUT_OF_MEMORY;
}

// slots of s.p (powers, `count` of them real) -> out: host float64[count][bins]
int rows_to_host(SegmentPlans &s, int count, double *out) {
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

// d_alpha: device float64[S][9] -> out: host float64[K][bins] (average) or [Q][K][bins]; null stream
int segments_on_device(SegmentPlans &s, const double *d_alpha, int64_t Q, int64_t hop, const double *taper,
                       const double *weights, int64_t K, int average, double *out) {
  const int64_t n = s.n, L = s.L, bins = num_bins(n);
  const int B = s.B, R = s.R;
  int rc;
  if ((rc = s.tau.ensure((size_t)n * sizeof(double))) != RN_OK) return rc;
  if ((rc = s.w.ensure((size_t)K * kPairs * sizeof(double))) != RN_OK) return rc;
  if (hipMemcpy(s.tau.ptr, taper, (size_t)n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(s.w.ptr, weights, (size_t)K * kPairs * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
    return RN_ERR_HIP;
  auto *x = s.x.as<hipfftDoubleComplex>(), *p = s.p.as<hipfftDoubleComplex>();
  const auto *w = s.w.as<const double>();
  const unsigned gl = (unsigned)((L + kPowerThreads - 1) / kPowerThreads);
  const unsigned tiles = (unsigned)((R + kRowTile - 1) / kRowTile);
  int64_t held = -1;  // the first segment of the block whose transforms x holds
  auto transform_block = [&](int64_t q0, int count) -> int {
    if (held == q0) return RN_OK;
    build_segments_kernel<<<dim3(blocks_of_256(L), (unsigned)B), 256>>>(d_alpha, s.tau.as<const double>(), n, L, hop,
                                                                        q0, count, x);
    if (!s.plan_x.exec(x, HIPFFT_FORWARD)) return RN_ERR_HIP;
    held = q0;
    return RN_OK;
  };
  if (average) {
    for (int64_t k0 = 0; k0 < K; k0 += R) {
      const int kc = (int)std::min<int64_t>(R, K - k0);
      for (int64_t q0 = 0; q0 < Q; q0 += B) {
        const int count = (int)std::min<int64_t>(B, Q - q0);
        if ((rc = transform_block(q0, count)) != RN_OK) return rc;
        segment_mean_power_kernel<<<dim3(gl, tiles), kPowerThreads>>>(x, L, count, w, k0, kc, R, 1.0 / (double)Q,
                                                                      q0 == 0, p);
      }
      if ((rc = rows_to_host(s, kc, out + k0 * bins)) != RN_OK) return rc;
    }
    return RN_OK;
  }
  for (int64_t q0 = 0; q0 < Q; q0 += B) {
    const int count = (int)std::min<int64_t>(B, Q - q0);
    if ((rc = transform_block(q0, count)) != RN_OK) return rc;
    const int64_t rows = count * K;
    for (int64_t r0 = 0; r0 < rows; r0 += R) {
      const int rc_count = (int)std::min<int64_t>(R, rows - r0);
      segment_power_kernel<<<dim3(gl, tiles), kPowerThreads>>>(x, L, w, K, r0, rc_count, R, p);
      if ((rc = rows_to_host(s, rc_count, out + (q0 * K + r0) * bins)) != RN_OK) return rc;
    }
  }
  return RN_OK;
}

// both entries: alpha (float64[S][3][3]) from `src`; taper (host [W-1]), weights (host [K][21]) -> intensities (host)
int md_raman_segments(Source src, int64_t S, int64_t W, int64_t hop, const double *taper, const double *weights,
                      int64_t K, int average, int device, size_t workspace_limit, double *intensities, int64_t bins) {
  for (const void *q : {(const void *)src.data, (const void *)taper, (const void *)weights, (const void *)intensities})
    if (!q) return RN_ERR_INVALID_ARGUMENT;
  if (K < 1 || K > ((int64_t)1 << 40)) return RN_ERR_INVALID_ARGUMENT;
  if (W < 3 || W > S || hop < 1) return RN_ERR_INVALID_ARGUMENT;
  if (bins != num_bins(W - 1) || (average != 0 && average != 1)) return RN_ERR_INVALID_ARGUMENT;
  const int64_t n = W - 1, Q = (S - W) / hop + 1;
  int rc = check_call({src.data, taper, weights, intensities}, n, bins, device);
  if (rc != RN_OK || bins == 0) return rc;
  if ((rc = src.wait()) != RN_OK) return rc;
  const size_t limit = workspace_limit ? workspace_limit : kDefaultWorkspace;
  std::lock_guard<std::mutex> lock(g_segment_cache.mutex);
  SegmentPlans *s = nullptr;
  const double *d_alpha = nullptr;
  if ((rc = get_plans(device, n, Q, K, average, limit, &s)) != RN_OK) return rc;
  if ((rc = src.on_device(s->alpha, (size_t)S * 9 * sizeof(double), &d_alpha)) != RN_OK) return rc;
  return segments_on_device(*s, d_alpha, Q, hop, taper, weights, K, average, intensities);
}

}  // namespace

extern "C" int rn_md_raman_segments(const double *alpha, int64_t S, int64_t segment_steps, int64_t hop,
                                    const double *taper, const double *weights, int64_t K, int average, int device,
                                    size_t workspace_limit, double *intensities, int64_t num_bins) {
  return md_raman_segments(Source::host(alpha), S, segment_steps, hop, taper, weights, K, average, device,
                           workspace_limit, intensities, num_bins);
}

extern "C" int rn_md_raman_segments_device(const double *d_alpha, int64_t S, int64_t segment_steps, int64_t hop,
                                           const double *taper, const double *weights, int64_t K, int average,
                                           int device, size_t workspace_limit, double *intensities, int64_t num_bins,
                                           void *stream) {
  return md_raman_segments(Source::device(d_alpha, stream), S, segment_steps, hop, taper, weights, K, average, device,
                           workspace_limit, intensities, num_bins);
}
