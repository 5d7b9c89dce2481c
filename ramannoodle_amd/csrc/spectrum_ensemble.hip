// On-device segment (Welch) MD Raman spectra from a table of segment starts, whole and by atom group: what
// MDRamanEnsemble / PartialMDRamanSpectrum.measure_segments reduce before the laser / Bose-Einstein corrections.
//
// rn_md_raman_segments_at is rn_md_raman_segments with segment q starting at step starts[q] instead of q * hop: the
// caller lays the table so that no segment crosses a run boundary of a concatenated series, and the mean over the
// segments of several runs is one call.  Only the builder differs (it reads the table); the power kernels, the blocks
// and the pipeline are spectrum_segment_core.hpp's, so with starts[q] = q * hop the arithmetic, its order and the
// result are rn_md_raman_segments' own.
//
// rn_md_raman_partial_segments is the Welch form of rn_md_raman_partial.  Increment t belongs to the step from frame t
// to frame t + 1, so a segment of W frames starting at frame a uses increments a .. a + W - 2 (n = W - 1 of them).  Per
// block of B segments:
//   builder: x[B][G][6][L], the tapered components of the symmetric part of each group's increments, zero-padded -> 6 G B
//   batched forward FFTs of length L -> the power kernel; with M_k the 6x6 form of configuration k (unpacked as
//   rn_md_raman_partial does) and a row r = (k, pair g <= h) in rn_md_raman_partial's order,
//     P_qr(f) = sum_{c,c'} M_k[c][c'] Re(X_{q,g,c}(f) conj X_{q,h,c'}(f)),
//     average = 0: p[j][f] = P_qr(f) for a sub-block of the block's rows (q, r)
//     average = 1: pbar[r][f] += P_qr(f) / Q over the block's segments, in segment order, no atomics
//   -> inverse -> positive lags -> length-n transform -> bins (the core's back half): 6 G Q forward transforms and
//   2 K G(G+1)/2 more for the mean, against Q (6 G + 2 K G(G+1)/2) for Q calls of rn_md_raman_partial.
// A thread of the power kernels owns one frequency of a tile of kPairTile rows.  At G = 16 a frequency has 96 complex
// inputs, so nothing is kept across rows but the first group's six values while consecutive rows share it: the thread
// loops over its rows, loads the two groups' values (from L1 / L2: a tile re-reads what its neighbours read) and
// contracts them with the row's form from LDS (all lanes read one address: a broadcast, no bank conflict).
// float64 throughout.  Both entry pairs share one plan cache, apart from the caches of the other four reducers, keyed
// by (device, n, series per segment, segments per block, rows per block).  All work runs on the null stream (after a
// synchronise of the caller's stream in the _device entries).
#include "kernels.hpp"
#include "spectrum_segment_core.hpp"

namespace {
using namespace rn_spectrum;
using rn::kMaxGroups;

constexpr int kPairTile = 8;  // rows per thread of the atom-group power kernels (blockIdx.y)

// segment b of the block, group g = blockIdx.z: x[b][g][c][t] = tau[t] * component c of the symmetric part of
// incr[starts[q0+b] + t][g] for t < n; zero for n <= t < L and for b >= count
__global__ void build_group_segments_kernel(const double *__restrict__ incr, const double *__restrict__ tau, int64_t n,
                                            int64_t L, int G, const int64_t *__restrict__ starts, int64_t q0, int count,
                                            hipfftDoubleComplex *__restrict__ x) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y, g = blockIdx.z;
  if (t >= L) return;
  double s[kComponents] = {0, 0, 0, 0, 0, 0};
  if (t < n && b < count) {
    const double *a = incr + ((starts[q0 + b] + t) * G + g) * 9;
    const double w = tau[t];
    double d[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) d[i] = w * a[i];
    symmetric_components(d, s);
  }
#pragma unroll
  for (int c = 0; c < kComponents; ++c)
    x[(((int64_t)b * G + g) * kComponents + c) * L + t] = make_double2(s[c], 0.0);
}

// average = 0.  Slot j of the sub-block (rows r0 .. r0+count-1 of the segment block, row r = (b K + k) pairs + pair):
// P_br(f); slots >= count are zeroed.  Each thread writes one frequency of kPairTile rows.
__global__ void __launch_bounds__(kPowerThreads)
    group_segment_power_kernel(const hipfftDoubleComplex *__restrict__ x, int64_t L, int G, const double *__restrict__ w,
                               int64_t K, int64_t r0, int count, int slots, hipfftDoubleComplex *__restrict__ p) {
  __shared__ double ms[kPairTile * kFormSize];
  const int pairs = G * (G + 1) / 2;
  const int j0 = blockIdx.y * kPairTile;
  const int nr = std::min(kPairTile, count - j0);  // (may be <= 0: a tile of zeroed slots)
  load_forms(w, r0 + j0, nr, pairs, K, ms);
  __syncthreads();
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= L) return;
  for (int i = 0; i < kPairTile && j0 + i < slots; ++i) {
    double v = 0.0;
    if (i < nr) {
      const int64_t r = r0 + j0 + i;
      const int64_t b = r / ((int64_t)pairs * K);
      int g, h;
      upper_pair((int)(r % pairs), G, g, h);
      hipfftDoubleComplex vg[kComponents], vh[kComponents];
      load_group(x + ((b * G + g) * kComponents) * L + f, L, vg);
      load_group(x + ((b * G + h) * kComponents) * L + f, L, vh);
      v = contract_groups(ms + i * kFormSize, vg, vh);
    }
    p[(int64_t)(j0 + i) * L + f] = make_double2(v, 0.0);
  }
}

// average = 1.  Slot i (row r0 + i = (k, pair), i < rc): pbar[i][f] (+)= sum over the block's `count` segments, in order,
// of P_br(f) * inv_q; `first` starts the sum at zero; slots >= rc are zeroed.  One thread owns its (row, f) for the whole
// call.  The rows' groups depend on the tile alone (scalar registers).
__global__ void __launch_bounds__(kPowerThreads)
    group_segment_mean_power_kernel(const hipfftDoubleComplex *__restrict__ x, int64_t L, int count, int G,
                                    const double *__restrict__ w, int64_t K, int64_t r0, int rc, int slots, double inv_q,
                                    int first, hipfftDoubleComplex *__restrict__ pbar) {
  __shared__ double ms[kPairTile * kFormSize];
  const int pairs = G * (G + 1) / 2;
  const int i0 = blockIdx.y * kPairTile;
  const int nr = std::min(kPairTile, rc - i0);
  load_forms(w, r0 + i0, nr, pairs, K, ms);
  __syncthreads();
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= L) return;
  int64_t og[kPairTile], oh[kPairTile];  // where the row's two groups begin within a segment of x
  double acc[kPairTile];
#pragma unroll
  for (int i = 0; i < kPairTile; ++i) {
    int g = 0, h = 0;
    if (i < nr) upper_pair((int)((r0 + i0 + i) % pairs), G, g, h);
    og[i] = (int64_t)g * kComponents * L;
    oh[i] = (int64_t)h * kComponents * L;
    acc[i] = (first || i >= nr) ? 0.0 : pbar[(int64_t)(i0 + i) * L + f].x;
  }
  const int64_t segment = (int64_t)G * kComponents * L;
  for (int b = 0; b < (nr > 0 ? count : 0); ++b) {
    // A compiler barrier, as in segment_mean_power_kernel: the tile's 8 x 36 form entries are read from LDS in every
    // iteration instead of being hoisted out of the loop into registers (and from there into scratch).
    asm volatile("" ::: "memory");
    const hipfftDoubleComplex *xb = x + b * segment + f;
    hipfftDoubleComplex vg[kComponents], vh[kComponents];
#pragma unroll
    for (int i = 0; i < kPairTile; ++i)
      if (i < nr) {
        if (i == 0 || og[i] != og[i - 1]) load_group(xb + og[i], L, vg);  // consecutive pairs share their first group
        load_group(xb + oh[i], L, vh);
        acc[i] = fma(contract_groups(ms + i * kFormSize, vg, vh), inv_q, acc[i]);
      }
  }
#pragma unroll
  for (int i = 0; i < kPairTile; ++i)
    if (i0 + i < slots) pbar[(int64_t)(i0 + i) * L + f] = make_double2(acc[i], 0.0);
}

PlanCache<SegmentPlans> g_ensemble_cache;  // apart from the caches of the other four reducers

// the bytes of a call besides its blocks: the taper, the weights and the start table
size_t base_bytes(int64_t n, int64_t K, int64_t Q) {
  return (size_t)n * sizeof(double) + (size_t)K * kPairs * sizeof(double) + (size_t)Q * sizeof(int64_t);
}

// both whole-spectrum entries: alpha (float64[S][3][3]) from `src`; starts (host [Q]), taper (host [W-1]), weights (host
// [K][21]) -> intensities (host)
int md_raman_segments_at(Source src, int64_t S, int64_t W, const int64_t *starts, int64_t Q, const double *taper,
                         const double *weights, int64_t K, int average, int device, size_t workspace_limit,
                         double *intensities, int64_t bins) {
  for (const void *q : {(const void *)src.data, (const void *)starts, (const void *)taper, (const void *)weights,
                        (const void *)intensities})
    if (!q) return RN_ERR_INVALID_ARGUMENT;
  if (K < 1 || K > ((int64_t)1 << 40)) return RN_ERR_INVALID_ARGUMENT;
  int rc = check_table(S, W, starts, Q, average, bins);
  if (rc != RN_OK) return rc;
  const int64_t n = W - 1;
  rc = check_call({src.data, taper, weights, intensities}, n, bins, device);
  if (rc != RN_OK || bins == 0) return rc;
  if ((rc = src.wait()) != RN_OK) return rc;
  const size_t limit = workspace_limit ? workspace_limit : kDefaultWorkspace;
  std::lock_guard<std::mutex> lock(g_ensemble_cache.mutex);
  SegmentPlans *sp = nullptr;
  const double *d_alpha = nullptr;
  rc = get_segment_plans(g_ensemble_cache, device, n, kComponents, Q, K, average, limit, base_bytes(n, K, Q), &sp);
  if (rc != RN_OK) return rc;
  SegmentPlans &s = *sp;
  if ((rc = src.on_device(s.source, (size_t)S * 9 * sizeof(double), &d_alpha)) != RN_OK) return rc;
  if ((rc = upload_taper_and_weights(s, taper, weights, K)) != RN_OK) return rc;
  if ((rc = upload(s.starts, starts, (size_t)Q)) != RN_OK) return rc;
  auto build = [&](int64_t q0, int count) {
    build_segments_at_kernel<<<dim3(blocks_of_256(s.L), (unsigned)s.B), 256>>>(
        d_alpha, s.tau.as<const double>(), s.n, s.L, s.starts.as<const int64_t>(), q0, count,
        s.x.as<hipfftDoubleComplex>());
  };
  return run_segments(s, Q, K, average, build, whole_mean_power(s, Q), whole_row_power(s, K), intensities);
}

// both atom-group entries: increments (float64[N][G][9]) from `src` -> intensities (host, packed pairs)
int md_raman_partial_segments(Source src, int64_t N, int G, int64_t W, const int64_t *starts, int64_t Q,
                              const double *taper, const double *weights, int64_t K, int average, int device,
                              size_t workspace_limit, double *intensities, int64_t bins) {
  for (const void *q : {(const void *)src.data, (const void *)starts, (const void *)taper, (const void *)weights,
                        (const void *)intensities})
    if (!q) return RN_ERR_INVALID_ARGUMENT;
  if (G < 1 || G > kMaxGroups || N < 1 || N > (int64_t)1 << 40) return RN_ERR_INVALID_ARGUMENT;
  if (K < 1 || K > ((int64_t)1 << 40)) return RN_ERR_INVALID_ARGUMENT;
  int rc = check_table(N + 1, W, starts, Q, average, bins);  // N increments join N + 1 frames
  if (rc != RN_OK) return rc;
  const int64_t n = W - 1;
  rc = check_call({src.data, taper, weights, intensities}, n, bins, device);
  if (rc != RN_OK || bins == 0) return rc;
  if ((rc = src.wait()) != RN_OK) return rc;
  const size_t limit = workspace_limit ? workspace_limit : kDefaultWorkspace;
  const int pairs = G * (G + 1) / 2;
  const int64_t rows = K * pairs;
  std::lock_guard<std::mutex> lock(g_ensemble_cache.mutex);
  SegmentPlans *sp = nullptr;
  const double *d_incr = nullptr;
  rc = get_segment_plans(g_ensemble_cache, device, n, kComponents * G, Q, rows, average, limit, base_bytes(n, K, Q), &sp);
  if (rc != RN_OK) return rc;
  SegmentPlans &s = *sp;
  if ((rc = src.on_device(s.source, (size_t)N * G * 9 * sizeof(double), &d_incr)) != RN_OK) return rc;
  if ((rc = upload_taper_and_weights(s, taper, weights, K)) != RN_OK) return rc;
  if ((rc = upload(s.starts, starts, (size_t)Q)) != RN_OK) return rc;
  auto *x = s.x.as<hipfftDoubleComplex>(), *p = s.p.as<hipfftDoubleComplex>();
  const auto *w = s.w.as<const double>();
  const unsigned gl = (unsigned)((s.L + kPowerThreads - 1) / kPowerThreads);
  const unsigned tiles = (unsigned)((s.R + kPairTile - 1) / kPairTile);
  auto build = [&](int64_t q0, int count) {
    build_group_segments_kernel<<<dim3(blocks_of_256(s.L), (unsigned)s.B, (unsigned)G), 256>>>(
        d_incr, s.tau.as<const double>(), s.n, s.L, G, s.starts.as<const int64_t>(), q0, count, x);
  };
  auto mean_power = [&](int count, int64_t r0, int count_r, bool first) {
    group_segment_mean_power_kernel<<<dim3(gl, tiles), kPowerThreads>>>(x, s.L, count, G, w, K, r0, count_r, s.R,
                                                                        1.0 / (double)Q, first, p);
  };
  auto row_power = [&](int64_t r0, int count_r) {
    group_segment_power_kernel<<<dim3(gl, tiles), kPowerThreads>>>(x, s.L, G, w, K, r0, count_r, s.R, p);
  };
  return run_segments(s, Q, rows, average, build, mean_power, row_power, intensities);
}

}  // namespace

extern "C" int rn_md_raman_segments_at(const double *alpha, int64_t S, int64_t segment_steps, const int64_t *starts,
                                       int64_t Q, const double *taper, const double *weights, int64_t K, int average,
                                       int device, size_t workspace_limit, double *intensities, int64_t num_bins) {
  return md_raman_segments_at(Source::host(alpha), S, segment_steps, starts, Q, taper, weights, K, average, device,
                              workspace_limit, intensities, num_bins);
}

extern "C" int rn_md_raman_segments_at_device(const double *d_alpha, int64_t S, int64_t segment_steps,
                                              const int64_t *starts, int64_t Q, const double *taper,
                                              const double *weights, int64_t K, int average, int device,
                                              size_t workspace_limit, double *intensities, int64_t num_bins,
                                              void *stream) {
  return md_raman_segments_at(Source::device(d_alpha, stream), S, segment_steps, starts, Q, taper, weights, K, average,
                              device, workspace_limit, intensities, num_bins);
}

extern "C" int rn_md_raman_partial_segments(const double *increments, int64_t N, int G, int64_t segment_steps,
                                            const int64_t *starts, int64_t Q, const double *taper, const double *weights,
                                            int64_t K, int average, int device, size_t workspace_limit,
                                            double *intensities, int64_t num_bins) {
  return md_raman_partial_segments(Source::host(increments), N, G, segment_steps, starts, Q, taper, weights, K, average,
                                   device, workspace_limit, intensities, num_bins);
}

extern "C" int rn_md_raman_partial_segments_device(const double *d_increments, int64_t N, int G, int64_t segment_steps,
                                                   const int64_t *starts, int64_t Q, const double *taper,
                                                   const double *weights, int64_t K, int average, int device,
                                                   size_t workspace_limit, double *intensities, int64_t num_bins,
                                                   void *stream) {
  return md_raman_partial_segments(Source::device(d_increments, stream), N, G, segment_steps, starts, Q, taper, weights,
                                   K, average, device, workspace_limit, intensities, num_bins);
}
