// On-device reduction of a polarizability time series to the unpolarised MD Raman spectrum
// (SURVEY.md 8f item 3): MDRamanSpectrum.measure before the laser / Bose-Einstein corrections
// (ramannoodle/spectrum/_raman.py:282-297 with calc_signal_spectrum, spectrum/utils.py:76-124).
//
// The reference forms d(alpha)/dt, seven signals from it, the positive-lag autocorrelation of
// each (scipy.signal.correlate) and the real part of the length-(S-1) FFT of each, and adds
// them as 45 a^2 + 7 g^2.  Everything after the autocorrelation is linear, and by
// Wiener-Khinchin the autocorrelations are inverse transforms of power spectra, so here:
//   7 zero-padded forward FFTs (one batched launch) -> ONE weighted power spectrum
//   5|X_iso|^2 + 3.5(|X_1|^2+|X_2|^2+|X_3|^2) + 21(|X_xy|^2+|X_yz|^2+|X_xz|^2)
//   -> one inverse FFT (the combined autocorrelation) -> one length-(S-1) FFT.
// float64 throughout.  The transforms are hipFFT's, loaded on first use so that the library
// itself does not depend on it.  Plans and work buffers are cached per (device, series length):
// creating three hipFFT plans costs ~50 ms, the transforms of a 10^4-step series ~0.1 ms.
// rn_md_raman_intensities_device takes the time series where the evaluator left it (HBM), so that
// only the intensities leave the GPU.
#include "spectrum_common.hpp"

namespace {
using namespace rn_spectrum;

// x_j[n] from alpha[n+1] - alpha[n]; signals: trace, xx-yy, yy-zz, zz-xx, xy, yz, xz
__global__ void build_signals_kernel(const double *__restrict__ alpha, int64_t N, int64_t L,
                                     hipfftDoubleComplex *__restrict__ x) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= L) return;
  double s[7] = {0, 0, 0, 0, 0, 0, 0};
  if (n < N) {
    const double *a0 = alpha + n * 9, *a1 = a0 + 9;
    const double xx = a1[0] - a0[0], yy = a1[4] - a0[4], zz = a1[8] - a0[8];
    const double xy = a1[1] - a0[1], yz = a1[5] - a0[5], xz = a1[2] - a0[2];
    s[0] = xx + yy + zz;
    s[1] = xx - yy;
    s[2] = yy - zz;
    s[3] = zz - xx;
    s[4] = xy;
    s[5] = yz;
    s[6] = xz;
  }
#pragma unroll
  for (int j = 0; j < 7; ++j) x[(int64_t)j * L + n] = make_double2(s[j], 0.0);
}
// 45 (1/9) |iso|^2 + 7 (1/2 (...) + 3 (...))
__global__ void power_kernel(const hipfftDoubleComplex *__restrict__ x, int64_t L,
                             hipfftDoubleComplex *__restrict__ p) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= L) return;
  auto mag2 = [&](int j) {
    const hipfftDoubleComplex v = x[(int64_t)j * L + f];
    return v.x * v.x + v.y * v.y;
  };
  const double v = 5.0 * mag2(0) + 3.5 * (mag2(1) + mag2(2) + mag2(3)) + 21.0 * (mag2(4) + mag2(5) + mag2(6));
  p[f] = make_double2(v, 0.0);
}
__global__ void take_lags_kernel(const hipfftDoubleComplex *__restrict__ r, int64_t N, double scale,
                                 hipfftDoubleComplex *__restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < N) out[k] = make_double2(r[k].x * scale, 0.0);
}
__global__ void real_bins_kernel(const hipfftDoubleComplex *__restrict__ y, int64_t bins, double *__restrict__ out) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m < bins) out[m] = y[m + 1].x;  // the zero-frequency bin is dropped
}

// plans + work buffers of one (device, series length)
struct Plans {
  int device = -1;
  int64_t S = 0, L = 0;
  DeviceBuffer x, p, r, out, alpha;
  FftPlan plan_batch, plan_l, plan_n;
};
PlanCache<Plans> g_cache;

// returns the cache entry for (device, S), creating it if needed; rc != RN_OK on failure
int get_plans(int device, int64_t S, Plans **out) {
  if ((*out = g_cache.find([&](const Plans &e) { return e.device == device && e.S == S; }))) return RN_OK;
  const int64_t N = S - 1, bins = num_bins(N), L = padded_length(N);
  Plans &b = g_cache.emplace_front();
  b.device = device;
  b.S = S;
  b.L = L;
  const size_t cz = sizeof(hipfftDoubleComplex);
  int rc = RN_OK;
  if (b.x.ensure((size_t)7 * L * cz) != RN_OK || b.p.ensure((size_t)L * cz) != RN_OK ||
      b.r.ensure((size_t)N * cz) != RN_OK || b.out.ensure((size_t)(bins > 0 ? bins : 1) * sizeof(double)) != RN_OK)
    rc = RN_ERR_OUT_OF_MEMORY;
  else if (!b.plan_batch.make((int)L, 7) || !b.plan_l.make((int)L, 1) || !b.plan_n.make((int)N, 1))
    rc = RN_ERR_HIP;
  if (rc != RN_OK) {
    g_cache.drop_front();
    return rc;
  }
  g_cache.trim();
  *out = &b;
  return RN_OK;
}

// d_alpha: device float64[S][3][3]; result in b.out (device float64[bins]); null stream, synchronous
int reduce_on_device(Plans &b, const double *d_alpha) {
  const int64_t N = b.S - 1, L = b.L, bins = num_bins(N);
  auto *x = b.x.as<hipfftDoubleComplex>(), *p = b.p.as<hipfftDoubleComplex>(), *r = b.r.as<hipfftDoubleComplex>();
  const unsigned gl = blocks_of_256(L), gn = blocks_of_256(N);
  build_signals_kernel<<<gl, 256>>>(d_alpha, N, L, x);
  if (!b.plan_batch.exec(x, HIPFFT_FORWARD)) return RN_ERR_HIP;
  power_kernel<<<gl, 256>>>(x, L, p);
  if (!b.plan_l.exec(p, HIPFFT_BACKWARD)) return RN_ERR_HIP;
  take_lags_kernel<<<gn, 256>>>(p, N, 1.0 / (double)L, r);
  if (!b.plan_n.exec(r, HIPFFT_FORWARD)) return RN_ERR_HIP;
  real_bins_kernel<<<blocks_of_256(bins), 256>>>(r, bins, b.out.as<double>());
  if (hipGetLastError() != hipSuccess) return RN_ERR_HIP;
  return RN_OK;
}

// both entries: alpha (float64[S][3][3]) from `src` -> intensities (host float64[num_bins])
int md_raman_intensities(Source src, int64_t S, int device, double *intensities, int64_t bins) {
  int rc = check_call({src.data, intensities}, S - 1, bins, device);
  if (rc != RN_OK || bins == 0) return rc;
  if ((rc = src.wait()) != RN_OK) return rc;
  std::lock_guard<std::mutex> lock(g_cache.mutex);
  Plans *b = nullptr;
  const double *d_alpha = nullptr;
  if ((rc = get_plans(device, S, &b)) != RN_OK) return rc;
  if ((rc = src.on_device(b->alpha, (size_t)S * 9 * sizeof(double), &d_alpha)) != RN_OK) return rc;
  if ((rc = reduce_on_device(*b, d_alpha)) != RN_OK) return rc;
  if (hipMemcpy(intensities, b->out.ptr, (size_t)bins * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
    return RN_ERR_HIP;
  return RN_OK;
}

}  // namespace

extern "C" int rn_md_raman_intensities(const double *alpha, int64_t S, int device, double *intensities,
                                       int64_t num_bins) {
  return md_raman_intensities(Source::host(alpha), S, device, intensities, num_bins);
}

extern "C" int rn_md_raman_intensities_device(const double *d_alpha, int64_t S, int device, double *intensities,
                                              int64_t num_bins, void *stream) {
  return md_raman_intensities(Source::device(d_alpha, stream), S, device, intensities, num_bins);
}
