// On-device reduction of a polarizability time series to polarized / oriented MD Raman spectra:
// MDRamanSpectrum.measure_polarized before the laser / Bose-Einstein corrections.
//
// Configuration k (incident e_i, scattered e_s, orientation R) has the signal
// s_k(t) = e_s . R da(t) R^T . e_i, a linear form w_k . d(t) of the six components
// d = (xx, yy, zz, xy, yz, xz) of the symmetric part of da(t) = alpha(t+1) - alpha(t).  Its spectrum
// (calc_signal_spectrum: positive-lag autocorrelation, real part of the length-(S-1) FFT) is linear
// in the autocorrelation, so
//   I_k(f) = sum_{j<=l} W_k[p(j,l)] C_jl(f),
// with C_jl the same transform of the symmetrised cross-correlation (r_jl + r_lj)/2 and W_k the 21
// packed coefficients of a symmetric 6x6 form (off-diagonal entries doubled), built on the host.
// Hence 21 basis spectra, whatever the number of configurations K:
//   6 zero-padded forward FFTs (one batched launch, length L >= 2(S-1)-1)
//   for each group of G <= 21 pairs: Re(X_j conj X_l) (Wiener-Khinchin: its inverse is the symmetrised
//     cross-correlation) -> batched inverse of length L -> positive lags, scaled by 1/L, in place ->
//     batched forward of length N = S-1 (stride L, in place) -> real bins 1..bins into C[21][bins]
//   I[K][bins] = W[K][21] . C[21][bins]  (contraction kernel), copied to the host in blocks of K.
// float64 throughout; hipFFT is loaded once for the library (spectrum_common.hpp).  Plans and work
// buffers are cached per (device, S, G) in a cache of their own, so that rn_md_raman_intensities'
// cache and results are untouched.  All work runs on the null stream (after a synchronise of the
// caller's stream in the _device entry), like spectrum.hip.
#include "spectrum_common.hpp"

namespace {
using namespace rn_spectrum;

constexpr int kContractThreads = 256;
constexpr int kContractConfigs = 16;  // configurations per contraction block (blockIdx.y)
constexpr int64_t kMaxBlockConfigs = (int64_t)65535 * kContractConfigs;  // gridDim.y <= 65535
constexpr size_t kKeepOutputBytes = (size_t)256 << 20;  // larger output blocks are freed after the call

// x_c[n] for n < N from the symmetric part of alpha[n+1] - alpha[n]; zero for N <= n < L
__global__ void build_components_kernel(const double *__restrict__ alpha, int64_t N, int64_t L,
                                        hipfftDoubleComplex *__restrict__ x) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= L) return;
  double s[kComponents] = {0, 0, 0, 0, 0, 0};
  if (n < N) {
    const double *a0 = alpha + n * 9, *a1 = a0 + 9;
    double d[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) d[i] = a1[i] - a0[i];
    symmetric_components(d, s);
  }
#pragma unroll
  for (int c = 0; c < kComponents; ++c) x[(int64_t)c * L + n] = make_double2(s[c], 0.0);
}

// slot g of the group (pairs first .. first+count-1): Re(X_j conj X_l); slots >= count are zeroed
__global__ void cross_power_kernel(const hipfftDoubleComplex *__restrict__ x, int64_t L, int first, int count,
                                   int G, hipfftDoubleComplex *__restrict__ p) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int g = blockIdx.y;
  if (f >= L || g >= G) return;
  double v = 0.0;
  if (g < count) {
    int j, l;
    upper_pair(first + g, kComponents, j, l);
    const hipfftDoubleComplex a = x[(int64_t)j * L + f], b = x[(int64_t)l * L + f];
    v = a.x * b.x + a.y * b.y;
  }
  p[(int64_t)g * L + f] = make_double2(v, 0.0);
}

// out[k][m] = sum_p w[k0 + k][p] c[p][m] for k < kc: each thread keeps one frequency of the 21 basis
// spectra in registers and writes it for kContractConfigs configurations (coalesced rows)
__global__ void __launch_bounds__(kContractThreads) contract_kernel(const double *__restrict__ w, int64_t k0,
                                                                    int64_t kc, const double *__restrict__ c,
                                                                    int64_t bins, double *__restrict__ out) {
  __shared__ double ws[kContractConfigs * kPairs];
  const int64_t kb = (int64_t)blockIdx.y * kContractConfigs;
  const int nk = (int)std::min<int64_t>(kContractConfigs, kc - kb);
  for (int i = threadIdx.x; i < nk * kPairs; i += blockDim.x) ws[i] = w[(k0 + kb) * kPairs + i];
  __syncthreads();
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= bins) return;
  double cv[kPairs];
#pragma unroll
  for (int p = 0; p < kPairs; ++p) cv[p] = c[(int64_t)p * bins + m];
  for (int k = 0; k < nk; ++k) {
    const double *wk = ws + k * kPairs;
    double acc = 0.0;
#pragma unroll
    for (int p = 0; p < kPairs; ++p) acc = fma(wk[p], cv[p], acc);
    out[(kb + k) * bins + m] = acc;
  }
}

// plans + work buffers of one (device, S, G)
struct PolPlans {
  int device = -1;
  int64_t S = 0, L = 0;
  int G = 0;
  DeviceBuffer x, p, c, alpha, w, out;
  size_t fixed_bytes = 0;  // x + p + c + the plans' work areas
  FftPlan plan_x, plan_inv, plan_n;
};
PlanCache<PolPlans> g_pol_cache;  // separate from spectrum.hip's cache

// the bytes a call needs besides the plans' work areas, for G pairs per group and kc configurations per block
size_t buffer_bytes(int64_t L, int64_t bins, int64_t G, int64_t K, int64_t kc) {
  const size_t cz = sizeof(hipfftDoubleComplex);
  return (size_t)kComponents * L * cz + (size_t)G * L * cz + (size_t)kPairs * bins * sizeof(double) +
         (size_t)K * kPairs * sizeof(double) + (size_t)kc * bins * sizeof(double);
}

// creates the entry for (device, S, G); rc != RN_OK on failure (nothing is left behind)
int make_plans(int device, int64_t S, int G, PolPlans **out) {
  const int64_t N = S - 1, bins = num_bins(N), L = padded_length(N);
  PolPlans &b = g_pol_cache.emplace_front();
  b.device = device;
  b.S = S;
  b.L = L;
  b.G = G;
  const size_t cz = sizeof(hipfftDoubleComplex);
  int rc = RN_OK;
  if (b.x.ensure((size_t)kComponents * L * cz) != RN_OK || b.p.ensure((size_t)G * L * cz) != RN_OK ||
      b.c.ensure((size_t)kPairs * bins * sizeof(double)) != RN_OK)
    rc = RN_ERR_OUT_OF_MEMORY;
  // plan_n: length N, batch G, each batch at the start of its length-L slot
  else if (!b.plan_x.make((int)L, kComponents) || !b.plan_inv.make((int)L, G) || !b.plan_n.make((int)N, G, (int)L))
    rc = RN_ERR_HIP;
  if (rc != RN_OK) {
    g_pol_cache.drop_front();
    return rc;
  }
  b.fixed_bytes = buffer_bytes(L, bins, G, 0, 0) + b.plan_x.work_bytes() + b.plan_inv.work_bytes() +
                  b.plan_n.work_bytes();
  *out = &b;
  return RN_OK;
}

// finds or creates the entry for (device, S) whose G fits `limit` together with K configurations'
// weights and a block of at least one configuration's intensities; *kc = configurations per block
int get_plans(int device, int64_t S, int64_t K, size_t limit, PolPlans **out, int64_t *kc) {
  const int64_t N = S - 1, bins = num_bins(N), L = padded_length(N);
  // the largest G whose buffers fit; G is then balanced over the groups (21 pairs in ceil(21/G) groups)
  int gmax = 0;
  for (int g = kPairs; g >= 1; --g)
    if (buffer_bytes(L, bins, g, K, 1) <= limit) {
      gmax = g;
      break;
    }
  if (gmax == 0) return RN_ERR_OUT_OF_MEMORY;
  PolPlans *b = nullptr;
  for (int attempt = 0; attempt < 3 && !b; ++attempt) {
    const int groups = (kPairs + gmax - 1) / gmax, G = (kPairs + groups - 1) / groups;
    b = g_pol_cache.find([&](const PolPlans &e) { return e.device == device && e.S == S && e.G == G; });
    if (!b) {
      int rc = make_plans(device, S, G, &b);
      if (rc != RN_OK) return rc;
    }
    const size_t need = b->fixed_bytes + (size_t)K * kPairs * sizeof(double) + (size_t)bins * sizeof(double);
    if (need > limit) {
      // the plans' work areas do not fit beside the buffers: fewer pairs per group (work scales with G)
      const size_t work = b->fixed_bytes - buffer_bytes(L, bins, G, 0, 0);
      const size_t per_pair = (size_t)L * sizeof(hipfftDoubleComplex) + work / (size_t)G;
      const size_t base = buffer_bytes(L, bins, 0, K, 1);
      const int fit = limit > base ? (int)std::min<size_t>((limit - base) / per_pair, (size_t)kPairs) : 0;
      g_pol_cache.drop_front();
      b = nullptr;
      gmax = std::min(fit, G - 1);
      if (gmax < 1) return RN_ERR_OUT_OF_MEMORY;
    }
  }
  if (!b) return RN_ERR_OUT_OF_MEMORY;
  g_pol_cache.trim();
  const size_t spare = limit - b->fixed_bytes - (size_t)K * kPairs * sizeof(double);
  *kc = std::max<int64_t>(1, std::min<int64_t>({K, (int64_t)(spare / ((size_t)bins * sizeof(double))),
                                                 kMaxBlockConfigs}));
  *out = b;
  return RN_OK;
}

// d_alpha: device float64[S][3][3]; fills b.c with the 21 basis spectra; null stream
int basis_on_device(PolPlans &b, const double *d_alpha) {
  const int64_t N = b.S - 1, L = b.L, bins = num_bins(N);
  auto *x = b.x.as<hipfftDoubleComplex>(), *p = b.p.as<hipfftDoubleComplex>();
  const unsigned gl = blocks_of_256(L), gn = blocks_of_256(N), gb = blocks_of_256(bins);
  build_components_kernel<<<gl, 256>>>(d_alpha, N, L, x);
  if (!b.plan_x.exec(x, HIPFFT_FORWARD)) return RN_ERR_HIP;
  for (int first = 0; first < kPairs; first += b.G) {
    const int count = std::min(b.G, kPairs - first);
    cross_power_kernel<<<dim3(gl, (unsigned)b.G), 256>>>(x, L, first, count, b.G, p);
    if (!b.plan_inv.exec(p, HIPFFT_BACKWARD)) return RN_ERR_HIP;
    slot_lags_kernel<<<dim3(gn, (unsigned)b.G), 256>>>(p, N, L, 1.0 / (double)L);
    if (!b.plan_n.exec(p, HIPFFT_FORWARD)) return RN_ERR_HIP;
    // C[first + g][m] = Re(Y_g[m + 1]) for the group's real slots
    slot_bins_kernel<<<dim3(gb, (unsigned)count), 256>>>(p, L, bins, count, b.c.as<double>() + first * bins);
  }
  if (hipGetLastError() != hipSuccess) return RN_ERR_HIP;
  return RN_OK;
}

// weights (host [K][21]) -> intensities (host [K][bins]), kc configurations at a time
int contract_to_host(PolPlans &b, const double *weights, int64_t K, int64_t kc, double *intensities) {
  const int64_t bins = num_bins(b.S - 1);
  int rc;
  if ((rc = b.w.ensure((size_t)K * kPairs * sizeof(double))) != RN_OK) return rc;
  if ((rc = b.out.ensure((size_t)kc * bins * sizeof(double))) != RN_OK) return rc;
  if (hipMemcpy(b.w.ptr, weights, (size_t)K * kPairs * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
    return RN_ERR_HIP;
  const auto *w = b.w.as<const double>(), *c = b.c.as<const double>();
  auto *o = b.out.as<double>();
  for (int64_t k0 = 0; k0 < K; k0 += kc) {
    const int64_t n = std::min(kc, K - k0);
    const dim3 grid((unsigned)((bins + kContractThreads - 1) / kContractThreads),
                    (unsigned)((n + kContractConfigs - 1) / kContractConfigs));
    contract_kernel<<<grid, kContractThreads>>>(w, k0, n, c, bins, o);
    if (hipGetLastError() != hipSuccess) return RN_ERR_HIP;
    if (hipMemcpy(intensities + k0 * bins, o, (size_t)n * bins * sizeof(double), hipMemcpyDeviceToHost) !=
        hipSuccess)
      return RN_ERR_HIP;
  }
  if (b.out.bytes > kKeepOutputBytes) b.out.release();  // the cache keeps the basis, not a large block of intensities
  return RN_OK;
}

// both entries: alpha (float64[S][3][3]) from `src`, weights (host [K][21]) -> intensities (host [K][bins])
int md_raman_polarized(Source src, int64_t S, const double *weights, int64_t K, int device, size_t workspace_limit,
                       double *intensities, int64_t bins) {
  if (K < 1 || K > ((int64_t)1 << 40)) return RN_ERR_INVALID_ARGUMENT;
  int rc = check_call({src.data, weights, intensities}, S - 1, bins, device);
  if (rc != RN_OK || bins == 0) return rc;
  if ((rc = src.wait()) != RN_OK) return rc;
  const size_t limit = workspace_limit ? workspace_limit : kDefaultWorkspace;
  std::lock_guard<std::mutex> lock(g_pol_cache.mutex);
  PolPlans *b = nullptr;
  int64_t kc = 0;
  const double *d_alpha = nullptr;
  if ((rc = get_plans(device, S, K, limit, &b, &kc)) != RN_OK) return rc;
  if ((rc = src.on_device(b->alpha, (size_t)S * 9 * sizeof(double), &d_alpha)) != RN_OK) return rc;
  if ((rc = basis_on_device(*b, d_alpha)) != RN_OK) return rc;
  return contract_to_host(*b, weights, K, kc, intensities);
}

}  // namespace

extern "C" int rn_md_raman_polarized(const double *alpha, int64_t S, const double *weights, int64_t K, int device,
                                     size_t workspace_limit, double *intensities, int64_t num_bins) {
  return md_raman_polarized(Source::host(alpha), S, weights, K, device, workspace_limit, intensities, num_bins);
}

extern "C" int rn_md_raman_polarized_device(const double *d_alpha, int64_t S, const double *weights, int64_t K,
                                            int device, size_t workspace_limit, double *intensities,
                                            int64_t num_bins, void *stream) {
  return md_raman_polarized(Source::device(d_alpha, stream), S, weights, K, device, workspace_limit, intensities,
                            num_bins);
}
