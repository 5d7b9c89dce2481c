// On-device many-channel MD Raman spectra from a table of segment starts: the self-spectrum of every channel of a set of
// polarizability increments (the phonon modes of PotGNN.calc_mode_increments) and the spectrum of their sum.  What
// ModeMDRamanSpectrum.measure / measure_segments reduce (include/rn_potgnn.h, rn_md_raman_modes).
//
// Definition.  Increments incr[t][c][9] (N steps, C channels), weights W[K][21], a start table, W frames per segment
// (n = W - 1 increments) and a taper tau[0..n-1].  With channel C the sum over the channels, ascending per entry,
//   series       x_{q,c,j}[t] = component j of the symmetric part of tau[t] incr[starts[q] + t][c],  t = 0..n-1, c <= C
//   row (q,k,c)  rn_md_raman_partial_segments' I_k[g][g] of channel c alone:
//                P_qkc(f) = sum_{j,l} M_k[j][l] Re(X_{q,c,j}(f) conj X_{q,c,l}(f)) on the zero-padded length L, then the
//                core's back half (inverse -> positive lags -> length-n transform -> bins)
// average = 1 is the mean over the Q segments taken on P, in table order.  Rows c < C are the self-spectra, row C the
// whole spectrum; the interference between channels, row C - sum_c row c, is the caller's.
//
// Pipeline, per block of B segments and Cb channels (x[B][Cb][6][L]):
//   builder: the six tapered symmetric components of each channel of the block; the summed channel is one more channel,
//   whose thread adds the C channels of its step first -> 6 Cb B batched forward FFTs of length L
//   -> diagonal power kernels: a thread owns one frequency of a tile of kChannelTile rows, loads the channel's six values
//   and contracts them with the row's form from LDS (load_forms / contract_groups of the atom-group reducer)
//   -> the core's back half.  A row of a segment is r = k Cb + channel of the block, so the rows of a (q, k) are
//   contiguous in the output.
// Blocking.  The channels go through in an outer loop of blocks of Cb (a short last block is padded with zero channels),
// each through run_segments with series = 6 Cb and rows = K Cb.  Channels are independent, so every row's arithmetic is
// the same whatever Cb and B are, and a channel of zeros yields rows that are exactly zero.
// float64 throughout.  A plan cache of its own, keyed by (device, n, 6 Cb, B, R).  All work runs on the null stream (after
// a synchronise of the caller's stream in the _device entry).
#include <vector>

#include "spectrum_segment_core.hpp"

namespace {
using namespace rn_spectrum;

constexpr int kChannelTile = 8;           // rows per thread of the power kernels (blockIdx.y)
constexpr int64_t kMostChannels = (int64_t)1 << 30;

// average = 0.  Slot j of the sub-block (rows r0 .. r0+count-1 of the segment block, row r = (b K + k) Cb + cl): P_r(f);
// slots >= count are zeroed.
__global__ void __launch_bounds__(kPowerThreads)
    channel_power_kernel(const hipfftDoubleComplex *__restrict__ x, int64_t L, int Cb, const double *__restrict__ w,
                         int64_t K, int64_t r0, int count, int slots, hipfftDoubleComplex *__restrict__ p) {
  __shared__ double ms[kChannelTile * kFormSize];
  const int j0 = blockIdx.y * kChannelTile;
  const int nr = std::min(kChannelTile, count - j0);  // (may be <= 0: a tile of zeroed slots)
  load_forms(w, r0 + j0, nr, Cb, K, ms);
  __syncthreads();
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= L) return;
  for (int i = 0; i < kChannelTile && j0 + i < slots; ++i) {
    double v = 0.0;
    if (i < nr) {
      const int64_t r = r0 + j0 + i;
      const int64_t b = r / ((int64_t)Cb * K), cl = r % Cb;
      hipfftDoubleComplex vc[kComponents];
      load_group(x + ((b * Cb + cl) * kComponents) * L + f, L, vc);
      v = contract_groups(ms + i * kFormSize, vc, vc);
    }
    p[(int64_t)(j0 + i) * L + f] = make_double2(v, 0.0);
  }
}

// average = 1.  Slot i (row r0 + i = k Cb + cl of a segment, i < rc): pbar[i][f] (+)= sum over the block's `count`
// segments, in order, of P_br(f) * inv_q; `first` starts the sum at zero; slots >= rc are zeroed.  One thread owns its
// (row, f) for the whole call.
__global__ void __launch_bounds__(kPowerThreads)
    channel_mean_power_kernel(const hipfftDoubleComplex *__restrict__ x, int64_t L, int count, int Cb,
                              const double *__restrict__ w, int64_t K, int64_t r0, int rc, int slots, double inv_q,
                              int first, hipfftDoubleComplex *__restrict__ pbar) {
  __shared__ double ms[kChannelTile * kFormSize];
  const int i0 = blockIdx.y * kChannelTile;
  const int nr = std::min(kChannelTile, rc - i0);
  load_forms(w, r0 + i0, nr, Cb, K, ms);
  __syncthreads();
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= L) return;
  const int64_t segment = (int64_t)Cb * kComponents * L;
  for (int i = 0; i < kChannelTile && i0 + i < slots; ++i) {
    hipfftDoubleComplex *out = pbar + (int64_t)(i0 + i) * L + f;
    double acc = (first || i >= nr) ? 0.0 : out->x;
    if (i < nr) {
      const hipfftDoubleComplex *xc = x + ((r0 + i0 + i) % Cb) * kComponents * L + f;
      for (int b = 0; b < count; ++b) {
        hipfftDoubleComplex vc[kComponents];
        load_group(xc + b * segment, L, vc);
        acc = fma(contract_groups(ms + i * kFormSize, vc, vc), inv_q, acc);
      }
    }
    *out = make_double2(acc, 0.0);
  }
}

PlanCache<SegmentPlans> g_modes_cache;  // apart from the caches of the other reducers
PhaseTimer g_timer;                      // builder, forward FFTs, power kernel, back half; under g_modes_cache.mutex

// the most channels per block whose series of one segment and K rows each fit `avail` bytes and the caps of the core; 0:
// not one
int64_t channels_per_block(size_t avail, int64_t L, int64_t bins, int64_t K, int64_t channels) {
  const size_t cz = sizeof(hipfftDoubleComplex);
  const size_t per_channel = (size_t)kComponents * L * cz + (size_t)L * cz + (size_t)bins * sizeof(double);
  const int64_t most = std::min<int64_t>({channels, kMaxChannels, std::max<int64_t>(1, kMaxRows / K),
                                          std::max<int64_t>(1, (int64_t)(kMaxBlockBytes / ((size_t)kComponents * L * cz)))});
  return std::min<int64_t>(most, (int64_t)(avail / per_channel));
}

// d_incr: device float64[N][C][9] -> out: host [K][C+1][bins] (average) or [Q][K][C+1][bins]
int modes_on_device(SegmentPlans &s, const double *d_incr, int64_t C, int64_t K, int64_t Q, int average, double *out) {
  const int64_t L = s.L, bins = num_bins(s.n), channels = C + 1;
  const int Cb = s.series / kComponents;
  auto *x = s.x.as<hipfftDoubleComplex>(), *p = s.p.as<hipfftDoubleComplex>();
  const auto *w = s.w.as<const double>();
  const unsigned gl = (unsigned)((L + kPowerThreads - 1) / kPowerThreads);
  const unsigned tiles = (unsigned)((s.R + kChannelTile - 1) / kChannelTile);
  const int64_t segments = average ? 1 : Q;
  std::vector<double> rows;  // a block's rows, when they are not the rows of `out`
  for (int64_t c0 = 0; c0 < channels; c0 += Cb) {
    const int cc = (int)std::min<int64_t>(Cb, channels - c0);
    auto build = [&](int64_t q0, int count) {
      g_timer.mark(0);
      build_channel_segments_kernel<<<dim3(blocks_of_256(L), (unsigned)s.B, (unsigned)Cb), 256>>>(
          d_incr, s.tau.as<const double>(), s.n, L, C, s.starts.as<const int64_t>(), q0, count, c0, cc, Cb, x);
      g_timer.mark(1);
    };
    auto mean_power = [&](int count, int64_t r0, int rc, bool first) {
      g_timer.mark(2);
      channel_mean_power_kernel<<<dim3(gl, tiles), kPowerThreads>>>(x, L, count, Cb, w, K, r0, rc, s.R, 1.0 / (double)Q,
                                                                   first, p);
      g_timer.mark(3);
    };
    auto row_power = [&](int64_t r0, int rc) {
      g_timer.mark(2);
      channel_power_kernel<<<dim3(gl, tiles), kPowerThreads>>>(x, L, Cb, w, K, r0, rc, s.R, p);
      g_timer.mark(3);
    };
    int rc;
    if (Cb == channels) {
      rc = run_segments(s, Q, K * Cb, average, build, mean_power, row_power, out);
    } else {
      rows.resize((size_t)segments * K * Cb * bins);
      rc = run_segments(s, Q, K * Cb, average, build, mean_power, row_power, rows.data());
      for (int64_t qk = 0; rc == RN_OK && qk < segments * K; ++qk)
        std::copy_n(rows.data() + (size_t)qk * Cb * bins, (size_t)cc * bins, out + (qk * channels + c0) * bins);
    }
    g_timer.close();
    if (rc != RN_OK) return rc;
  }
  return RN_OK;
}

// both entries: increments (float64[N][C][9]) from `src`; starts (host [Q]), taper (host [W-1]), weights (host [K][21])
// -> intensities (host)
int md_raman_modes(Source src, int64_t N, int C, int64_t W, const int64_t *starts, int64_t Q, const double *taper,
                   const double *weights, int64_t K, int average, int device, size_t workspace_limit,
                   double *intensities, int64_t bins) {
  for (const void *q : {(const void *)src.data, (const void *)starts, (const void *)taper, (const void *)weights,
                        (const void *)intensities})
    if (!q) return RN_ERR_INVALID_ARGUMENT;
  if (C < 1 || C > kMostChannels || N < 1 || N > (int64_t)1 << 40) return RN_ERR_INVALID_ARGUMENT;
  if (K < 1 || K > ((int64_t)1 << 40)) return RN_ERR_INVALID_ARGUMENT;
  int rc = check_table(N + 1, W, starts, Q, average, bins);  // N increments join N + 1 frames
  if (rc != RN_OK) return rc;
  const int64_t n = W - 1;
  rc = check_call({src.data, taper, weights, intensities}, n, bins, device);
  if (rc != RN_OK || bins == 0) return rc;
  if ((rc = src.wait()) != RN_OK) return rc;
  const int64_t L = padded_length(n), channels = (int64_t)C + 1;
  const size_t limit = workspace_limit ? workspace_limit : kDefaultWorkspace;
  const size_t base = (size_t)n * sizeof(double) + (size_t)K * kPairs * sizeof(double) + (size_t)Q * sizeof(int64_t);
  if (limit <= base) return RN_ERR_OUT_OF_MEMORY;
  std::lock_guard<std::mutex> lock(g_modes_cache.mutex);
  int64_t most = channels_per_block(limit - base, L, bins, K, channels);
  if (most < 1) return RN_ERR_OUT_OF_MEMORY;
  SegmentPlans *sp = nullptr;
  for (;;) {  // (the plans' work areas may not fit beside the largest block: halve it)
    const int Cb = (int)balanced(channels, most);
    rc = get_segment_plans(g_modes_cache, device, n, kComponents * Cb, Q, K * Cb, average, limit, base, &sp);
    if (rc != RN_ERR_OUT_OF_MEMORY || most == 1) break;
    most = (most + 1) / 2;
  }
  if (rc != RN_OK) return rc;
  SegmentPlans &s = *sp;
  const double *d_incr = nullptr;
  if ((rc = src.on_device(s.source, (size_t)N * C * 9 * sizeof(double), &d_incr)) != RN_OK) return rc;
  if ((rc = upload_taper_and_weights(s, taper, weights, K)) != RN_OK) return rc;
  if ((rc = upload(s.starts, starts, (size_t)Q)) != RN_OK) return rc;
  g_timer.reset();
  rc = modes_on_device(s, d_incr, C, K, Q, average, intensities);
  g_timer.collect();
  return rc;
}

}  // namespace

extern "C" int rn_md_raman_modes(const double *increments, int64_t N, int C, int64_t segment_steps, const int64_t *starts,
                                 int64_t Q, const double *taper, const double *weights, int64_t K, int average,
                                 int device, size_t workspace_limit, double *intensities, int64_t num_bins) {
  return md_raman_modes(Source::host(increments), N, C, segment_steps, starts, Q, taper, weights, K, average, device,
                        workspace_limit, intensities, num_bins);
}

extern "C" int rn_md_raman_modes_device(const double *d_increments, int64_t N, int C, int64_t segment_steps,
                                        const int64_t *starts, int64_t Q, const double *taper, const double *weights,
                                        int64_t K, int average, int device, size_t workspace_limit, double *intensities,
                                        int64_t num_bins, void *stream) {
  return md_raman_modes(Source::device(d_increments, stream), N, C, segment_steps, starts, Q, taper, weights, K, average,
                        device, workspace_limit, intensities, num_bins);
}

extern "C" int rn_md_raman_modes_set_profiling(int enabled) {
  return g_timer.set_profiling(g_modes_cache.mutex, enabled);
}

extern "C" int rn_md_raman_modes_phase_times(double *millis) { return g_timer.phase_times(g_modes_cache.mutex, millis); }
