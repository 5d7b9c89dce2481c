// On-device reduction of atom-group increments to partial MD Raman spectra: PartialMDRamanSpectrum.measure /
// measure_polarized before the laser / Bose-Einstein corrections.
//
// Group g's increments da_g(n), n < N (= S - 1 steps), give the six components d_{g,c} = (xx, yy, zz, xy, yz, xz) of
// their symmetric part.  For configuration k (a symmetric 6x6 form M_k unpacked from its 21 packed weights, as in
// spectrum_polarized.hip) and a pair of groups g <= h, the partial spectrum is calc_signal_spectrum's transform of
// the symmetrised cross-correlation of the two groups' signals, contracted with M_k:
//   I_k[g][h](f) = sum_{c,c'} M_k[c][c'] C(d_{g,c}, d_{h,c'})(f),
// with C(a, b) the real part of the length-N FFT of the positive lags of (r_ab + r_ba) / 2.  So sum_{g,h} I_k[g][h] is
// the spectrum of the summed increments and I_k[g][g] that of group g alone.  On the device:
//   6G zero-padded forward FFTs (one batched launch, length L >= 2N - 1)
//   for each block of B rows (k, g <= h):  P(f) = sum_{c,c'} M_k[c][c'] Re(X_{g,c}(f) conj X_{h,c'}(f))  (contraction
//     kernel; Wiener-Khinchin: its inverse is the contracted symmetrised cross-correlation) -> batched inverse of
//     length L -> positive lags, scaled by 1/L, in place -> batched forward of length N (stride L, in place) -> real
//     bins 1..bins, copied to the host rows.
// float64 throughout; hipFFT is loaded once for the library (spectrum_common.hpp).  Plans and work buffers are cached per (device, N, G, B) in
// a cache of their own, apart from the caches of rn_md_raman_intensities and rn_md_raman_polarized.  All work runs on the
// null stream (after a synchronise of the caller's stream in the _device entry).
#include "kernels.hpp"
#include "spectrum_common.hpp"

namespace {
using namespace rn_spectrum;
using rn::kMaxGroups;

constexpr int kMaxSlots = 64;  // rows per FFT block

// x[g*6 + c][n] for n < N from the symmetric part of incr[n][g]; zero for N <= n < L
__global__ void build_group_components_kernel(const double *__restrict__ incr, int64_t N, int64_t L, int G,
                                              hipfftDoubleComplex *__restrict__ x) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int g = blockIdx.y;
  if (n >= L || g >= G) return;
  double s[kComponents] = {0, 0, 0, 0, 0, 0};
  if (n < N) symmetric_components(incr + (n * G + g) * 9, s);
#pragma unroll
  for (int c = 0; c < kComponents; ++c) x[((int64_t)g * kComponents + c) * L + n] = make_double2(s[c], 0.0);
}

// slot j of the block (rows r0 .. r0+count-1, row r = k * pairs + q): the contracted cross-power of the row's two
// groups; slots >= count are zeroed
__global__ void partial_contract_kernel(const hipfftDoubleComplex *__restrict__ x, int64_t L, const double *__restrict__ w,
                                        int64_t r0, int count, int G, hipfftDoubleComplex *__restrict__ p) {
  __shared__ double m[kComponents * kComponents];
  const int j = blockIdx.y;
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int pairs = G * (G + 1) / 2;
  const int64_t r = r0 + j;
  if (j < count && threadIdx.x < kPairs) {  // M_k from the packed weights: diagonal as is, off-diagonal halved
    const int64_t k = r / pairs;
    int a, b;
    upper_pair(threadIdx.x, kComponents, a, b);
    const double v = w[k * kPairs + threadIdx.x];
    m[a * kComponents + b] = a == b ? v : 0.5 * v;
    m[b * kComponents + a] = a == b ? v : 0.5 * v;
  }
  __syncthreads();
  if (f >= L) return;
  double v = 0.0;
  if (j < count) {
    int g, h;
    upper_pair((int)(r % pairs), G, g, h);
    hipfftDoubleComplex a[kComponents], b[kComponents];
#pragma unroll
    for (int c = 0; c < kComponents; ++c) {
      a[c] = x[((int64_t)g * kComponents + c) * L + f];
      b[c] = x[((int64_t)h * kComponents + c) * L + f];
    }
#pragma unroll
    for (int c = 0; c < kComponents; ++c) {
      double row = 0.0;
#pragma unroll
      for (int e = 0; e < kComponents; ++e) row = fma(m[c * kComponents + e], a[c].x * b[e].x + a[c].y * b[e].y, row);
      v += row;
    }
  }
  p[(int64_t)j * L + f] = make_double2(v, 0.0);
}

// plans + work buffers of one (device, N, G, B)
struct PartialPlans {
  int device = -1;
  int64_t N = 0, L = 0;
  int G = 0, B = 0;
  DeviceBuffer x, p, out, incr, w;
  size_t fixed_bytes = 0;  // x + p + out + the plans' work areas
  FftPlan plan_x, plan_inv, plan_n;
};
PlanCache<PartialPlans> g_partial_cache;  // apart from the other two spectrum caches

// the bytes of a call's buffers besides the plans' work areas and the staged inputs
size_t buffer_bytes(int64_t L, int64_t bins, int G, int B) {
  const size_t cz = sizeof(hipfftDoubleComplex);
  return (size_t)kComponents * G * L * cz + (size_t)B * L * cz + (size_t)B * bins * sizeof(double);
}

int make_plans(int device, int64_t N, int G, int B, PartialPlans **out) {
  const int64_t L = padded_length(N), bins = num_bins(N);
  PartialPlans &b = g_partial_cache.emplace_front();
  b.device = device;
  b.N = N;
  b.L = L;
  b.G = G;
  b.B = B;
  const size_t cz = sizeof(hipfftDoubleComplex);
  int rc = RN_OK;
  if (b.x.ensure((size_t)kComponents * G * L * cz) != RN_OK || b.p.ensure((size_t)B * L * cz) != RN_OK ||
      b.out.ensure((size_t)B * bins * sizeof(double)) != RN_OK)
    rc = RN_ERR_OUT_OF_MEMORY;
  else if (!b.plan_x.make((int)L, kComponents * G) || !b.plan_inv.make((int)L, B) || !b.plan_n.make((int)N, B, (int)L))
    rc = RN_ERR_HIP;
  if (rc != RN_OK) {
    g_partial_cache.drop_front();
    return rc;
  }
  b.fixed_bytes = buffer_bytes(L, bins, G, B) + b.plan_x.work_bytes() + b.plan_inv.work_bytes() + b.plan_n.work_bytes();
  *out = &b;
  return RN_OK;
}

// finds or creates the entry for (device, N, G) with as many rows per block as fit `limit` beside K configurations'
// weights (at most kMaxSlots, at most the number of rows)
int get_plans(int device, int64_t N, int G, int64_t K, size_t limit, PartialPlans **out) {
  const int64_t L = padded_length(N), bins = num_bins(N);
  const int64_t rows = K * G * (G + 1) / 2;
  const size_t wbytes = (size_t)K * kPairs * sizeof(double);
  const size_t per_slot = (size_t)L * sizeof(hipfftDoubleComplex) + (size_t)bins * sizeof(double);
  const size_t base = buffer_bytes(L, bins, G, 0) + wbytes;
  if (limit < base + per_slot) return RN_ERR_OUT_OF_MEMORY;
  int bmax = (int)std::min<int64_t>({(int64_t)kMaxSlots, rows, (int64_t)((limit - base) / per_slot)});
  for (int attempt = 0; attempt < 3; ++attempt) {
    PartialPlans *b = g_partial_cache.find(
        [&](const PartialPlans &e) { return e.device == device && e.N == N && e.G == G && e.B == bmax; });
    if (!b) {
      int rc = make_plans(device, N, G, bmax, &b);
      if (rc != RN_OK) return rc;
    }
    if (b->fixed_bytes + wbytes <= limit) {
      g_partial_cache.trim();
      *out = b;
      return RN_OK;
    }
    // the plans' work areas do not fit beside the buffers: fewer rows per block (the inverse / length-N work scales with B)
    const size_t work = b->fixed_bytes - buffer_bytes(L, bins, G, bmax);
    g_partial_cache.drop_front();
    const size_t slot = per_slot + work / (size_t)bmax;
    const int fit = limit > base ? (int)std::min<size_t>((limit - base) / slot, (size_t)kMaxSlots) : 0;
    bmax = std::min(fit, bmax - 1);
    if (bmax < 1) return RN_ERR_OUT_OF_MEMORY;
  }
  return RN_ERR_OUT_OF_MEMORY;
}

// d_incr: device float64[N][G][9] -> out: host float64[K][G(G+1)/2][bins]; null stream
int partial_on_device(PartialPlans &b, const double *d_incr, const double *weights, int64_t K, double *out) {
  const int64_t N = b.N, L = b.L, bins = num_bins(N);
  const int G = b.G, B = b.B;
  const int64_t rows = K * G * (G + 1) / 2;
  int rc;
  if ((rc = b.w.ensure((size_t)K * kPairs * sizeof(double))) != RN_OK) return rc;
  if (hipMemcpy(b.w.ptr, weights, (size_t)K * kPairs * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
    return RN_ERR_HIP;
  auto *x = b.x.as<hipfftDoubleComplex>(), *p = b.p.as<hipfftDoubleComplex>();
  const unsigned gl = blocks_of_256(L), gn = blocks_of_256(N), gb = blocks_of_256(bins);
  build_group_components_kernel<<<dim3(gl, (unsigned)G), 256>>>(d_incr, N, L, G, x);
  if (!b.plan_x.exec(x, HIPFFT_FORWARD)) return RN_ERR_HIP;
  for (int64_t r0 = 0; r0 < rows; r0 += B) {
    const int count = (int)std::min<int64_t>(B, rows - r0);
    partial_contract_kernel<<<dim3(gl, (unsigned)B), 256>>>(x, L, b.w.as<const double>(), r0, count, G, p);
    if (!b.plan_inv.exec(p, HIPFFT_BACKWARD)) return RN_ERR_HIP;
    slot_lags_kernel<<<dim3(gn, (unsigned)B), 256>>>(p, N, L, 1.0 / (double)L);
    if (!b.plan_n.exec(p, HIPFFT_FORWARD)) return RN_ERR_HIP;
    slot_bins_kernel<<<dim3(gb, (unsigned)count), 256>>>(p, L, bins, count, b.out.as<double>());
    if (hipGetLastError() != hipSuccess) return RN_ERR_HIP;
    if (hipMemcpy(out + r0 * bins, b.out.ptr, (size_t)count * bins * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      return RN_ERR_HIP;
  }
  return RN_OK;
}

// both entries: increments (float64[N][G][9]) from `src`, weights (host [K][21]) -> intensities (host, packed pairs)
int md_raman_partial(Source src, int64_t N, int G, const double *weights, int64_t K, int device, size_t workspace_limit,
                     double *intensities, int64_t bins) {
  if (K < 1 || K > ((int64_t)1 << 40) || G < 1 || G > kMaxGroups) return RN_ERR_INVALID_ARGUMENT;
  int rc = check_call({src.data, weights, intensities}, N, bins, device);
  if (rc != RN_OK || bins == 0) return rc;
  if ((rc = src.wait()) != RN_OK) return rc;
  const size_t limit = workspace_limit ? workspace_limit : kDefaultWorkspace;
  std::lock_guard<std::mutex> lock(g_partial_cache.mutex);
  PartialPlans *b = nullptr;
  const double *d_incr = nullptr;
  if ((rc = get_plans(device, N, G, K, limit, &b)) != RN_OK) return rc;
  if ((rc = src.on_device(b->incr, (size_t)N * G * 9 * sizeof(double), &d_incr)) != RN_OK) return rc;
  return partial_on_device(*b, d_incr, weights, K, intensities);
}

}  // namespace

extern "C" int rn_md_raman_partial(const double *increments, int64_t N, int G, const double *weights, int64_t K,
                                   int device, size_t workspace_limit, double *intensities, int64_t num_bins) {
  return md_raman_partial(Source::host(increments), N, G, weights, K, device, workspace_limit, intensities, num_bins);
}

extern "C" int rn_md_raman_partial_device(const double *d_increments, int64_t N, int G, const double *weights,
                                          int64_t K, int device, size_t workspace_limit, double *intensities,
                                          int64_t num_bins, void *stream) {
  return md_raman_partial(Source::device(d_increments, stream), N, G, weights, K, device, workspace_limit, intensities,
                          num_bins);
}
