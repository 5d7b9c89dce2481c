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
// (device, n, segments per block, rows per block) in a cache of their own, apart from the caches of the other
// reducers.  All work runs on the null stream (after a synchronise of the caller's stream in the _device entry).
// The power kernels, the plans, the block sizes and the pipeline are spectrum_segment_core.hpp's, shared with the
// start-table reducers of spectrum_ensemble.hip; this file keeps the builder of segments on a hop grid.
#include "spectrum_segment_core.hpp"

namespace {
using namespace rn_spectrum;

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

PlanCache<SegmentPlans> g_segment_cache;  // apart from the other spectrum caches

// d_alpha: device float64[S][9] -> out: host float64[K][bins] (average) or [Q][K][bins]; null stream
int segments_on_device(SegmentPlans &s, const double *d_alpha, int64_t Q, int64_t hop, const double *taper,
                       const double *weights, int64_t K, int average, double *out) {
  if (int rc = upload_taper_and_weights(s, taper, weights, K)) return rc;
  auto build = [&](int64_t q0, int count) {
    build_segments_kernel<<<dim3(blocks_of_256(s.L), (unsigned)s.B), 256>>>(
        d_alpha, s.tau.as<const double>(), s.n, s.L, hop, q0, count, s.x.as<hipfftDoubleComplex>());
  };
  return run_segments(s, Q, K, average, build, whole_mean_power(s, Q), whole_row_power(s, K), out);
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
  const size_t base = (size_t)n * sizeof(double) + (size_t)K * kPairs * sizeof(double);  // the taper and the weights
  rc = get_segment_plans(g_segment_cache, device, n, kComponents, Q, K, average, limit, base, &s);
  if (rc != RN_OK) return rc;
  if ((rc = src.on_device(s->source, (size_t)S * 9 * sizeof(double), &d_alpha)) != RN_OK) return rc;
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
