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
// float64 throughout; hipFFT comes from the same dlopen()ed library as spectrum.hip.  Plans and work
// buffers are cached per (device, S, G) in a cache of their own, so that rn_md_raman_intensities'
// cache and results are untouched.  All work runs on the null stream (after a synchronise of the
// caller's stream in the _device entry), like spectrum.hip.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>

#include <algorithm>
#include <cstdint>
#include <list>
#include <mutex>

#include "../../include/rn_potgnn.h"

namespace {

constexpr int kPairs = 21;
constexpr int kComponents = 6;
constexpr int kContractThreads = 256;
constexpr int kContractConfigs = 16;  // configurations per contraction block (blockIdx.y)
constexpr int64_t kMaxBlockConfigs = (int64_t)65535 * kContractConfigs;  // gridDim.y <= 65535
constexpr size_t kKeepOutputBytes = (size_t)256 << 20;  // larger output blocks are freed after the call

struct FftApi {
  void *lib = nullptr;
  hipfftResult (*plan_many)(hipfftHandle *, int, int *, int *, int, int, int *, int, int, hipfftType, int) = nullptr;
  hipfftResult (*exec_z2z)(hipfftHandle, hipfftDoubleComplex *, hipfftDoubleComplex *, int) = nullptr;
  hipfftResult (*destroy)(hipfftHandle) = nullptr;
  hipfftResult (*get_size)(hipfftHandle, size_t *) = nullptr;  // optional
  bool ok = false;
};
FftApi &fft_api() {
  static FftApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    for (const char *name : {"libhipfft.so", "libhipfft.so.0", "/opt/rocm/lib/libhipfft.so"}) {
      api.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (api.lib) break;
    }
    if (!api.lib) return;
    api.plan_many = reinterpret_cast<decltype(api.plan_many)>(dlsym(api.lib, "hipfftPlanMany"));
    api.exec_z2z = reinterpret_cast<decltype(api.exec_z2z)>(dlsym(api.lib, "hipfftExecZ2Z"));
    api.destroy = reinterpret_cast<decltype(api.destroy)>(dlsym(api.lib, "hipfftDestroy"));
    api.get_size = reinterpret_cast<decltype(api.get_size)>(dlsym(api.lib, "hipfftGetSize"));
    api.ok = api.plan_many && api.exec_z2z && api.destroy;
  });
  return api;
}

// pair index p -> (j, l), j <= l, row-major over the upper triangle: (0,0) (0,1) .. (0,5) (1,1) .. (5,5)
__host__ __device__ inline void pair_components(int p, int &j, int &l) {
  j = 0;
  int row = kComponents;
  while (p >= row) {
    p -= row;
    ++j;
    --row;
  }
  l = j + p;
}

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
    s[0] = d[0];
    s[1] = d[4];
    s[2] = d[8];
    s[3] = 0.5 * (d[1] + d[3]);
    s[4] = 0.5 * (d[5] + d[7]);
    s[5] = 0.5 * (d[2] + d[6]);
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
    pair_components(first + g, j, l);
    const hipfftDoubleComplex a = x[(int64_t)j * L + f], b = x[(int64_t)l * L + f];
    v = a.x * b.x + a.y * b.y;
  }
  p[(int64_t)g * L + f] = make_double2(v, 0.0);
}

// the positive lags 0..N-1 of each slot, real part scaled by 1/L, in place
__global__ void lags_kernel(hipfftDoubleComplex *__restrict__ p, int64_t N, int64_t L, double scale) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int g = blockIdx.y;
  if (k >= N) return;
  hipfftDoubleComplex *q = p + (int64_t)g * L + k;
  *q = make_double2(q->x * scale, 0.0);
}

// C[first + g][m] = Re(Y_g[m + 1]) for the group's real slots (the zero-frequency bin is dropped)
__global__ void basis_bins_kernel(const hipfftDoubleComplex *__restrict__ y, int64_t L, int64_t bins, int first,
                                  int count, double *__restrict__ c) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int g = blockIdx.y;
  if (m >= bins || g >= count) return;
  c[(int64_t)(first + g) * bins + m] = y[(int64_t)g * L + m + 1].x;
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
  void *x = nullptr, *p = nullptr, *c = nullptr, *alpha = nullptr, *w = nullptr, *out = nullptr;
  size_t w_bytes = 0, out_bytes = 0;
  size_t fixed_bytes = 0;  // x + p + c + the plans' work areas
  hipfftHandle plan_x = 0, plan_inv = 0, plan_n = 0;
  bool have_x = false, have_inv = false, have_n = false;
  ~PolPlans() {
    FftApi &api = fft_api();
    if (api.ok) {
      if (have_x) api.destroy(plan_x);
      if (have_inv) api.destroy(plan_inv);
      if (have_n) api.destroy(plan_n);
    }
    for (void *q : {x, p, c, alpha, w, out})
      if (q) (void)hipFree(q);
  }
};
std::mutex g_pol_mutex;
std::list<PolPlans> g_pol_cache;  // front = most recently used; separate from spectrum.hip's cache
constexpr size_t kPolCacheEntries = 4;
constexpr size_t kDefaultWorkspace = (size_t)4 << 30;

size_t plan_work(hipfftHandle h) {
  size_t bytes = 0;
  FftApi &api = fft_api();
  if (api.get_size && api.get_size(h, &bytes) != HIPFFT_SUCCESS) bytes = 0;
  return bytes;
}

// the bytes a call needs besides the plans' work areas, for G pairs per group and kc configurations per block
size_t buffer_bytes(int64_t L, int64_t bins, int64_t G, int64_t K, int64_t kc) {
  const size_t cz = sizeof(hipfftDoubleComplex);
  return (size_t)kComponents * L * cz + (size_t)G * L * cz + (size_t)kPairs * bins * sizeof(double) +
         (size_t)K * kPairs * sizeof(double) + (size_t)kc * bins * sizeof(double);
}

// creates the entry for (device, S, G); rc != RN_OK on failure (nothing is left behind)
int make_plans(int device, int64_t S, int G, PolPlans **out) {
  FftApi &api = fft_api();
  const int64_t N = S - 1, bins = (N + 1) / 2 - 1;
  int64_t L = 1;
  while (L < 2 * N - 1) L <<= 1;
  g_pol_cache.emplace_front();
  PolPlans &b = g_pol_cache.front();
  b.device = device;
  b.S = S;
  b.L = L;
  b.G = G;
  const size_t cz = sizeof(hipfftDoubleComplex);
  int rc = RN_OK;
  if (hipMalloc(&b.x, (size_t)kComponents * L * cz) != hipSuccess ||
      hipMalloc(&b.p, (size_t)G * L * cz) != hipSuccess ||
      hipMalloc(&b.c, (size_t)kPairs * bins * sizeof(double)) != hipSuccess)
    rc = RN_ERR_OUT_OF_MEMORY;
  int nl = (int)L, nn = (int)N;
  if (rc == RN_OK) {
    b.have_x = api.plan_many(&b.plan_x, 1, &nl, nullptr, 1, nl, nullptr, 1, nl, HIPFFT_Z2Z, kComponents) ==
               HIPFFT_SUCCESS;
    b.have_inv = api.plan_many(&b.plan_inv, 1, &nl, nullptr, 1, nl, nullptr, 1, nl, HIPFFT_Z2Z, G) == HIPFFT_SUCCESS;
    // length N, batch G, each batch at the start of its length-L slot
    b.have_n = api.plan_many(&b.plan_n, 1, &nn, &nl, 1, nl, &nl, 1, nl, HIPFFT_Z2Z, G) == HIPFFT_SUCCESS;
    if (!(b.have_x && b.have_inv && b.have_n)) rc = RN_ERR_HIP;
  }
  if (rc != RN_OK) {
    g_pol_cache.pop_front();
    return rc;
  }
  b.fixed_bytes = (size_t)kComponents * L * cz + (size_t)G * L * cz + (size_t)kPairs * bins * sizeof(double) +
                  plan_work(b.plan_x) + plan_work(b.plan_inv) + plan_work(b.plan_n);
  *out = &b;
  return RN_OK;
}

// finds or creates the entry for (device, S) whose G fits `limit` together with K configurations'
// weights and a block of at least one configuration's intensities; *kc = configurations per block
int get_plans(int device, int64_t S, int64_t K, size_t limit, PolPlans **out, int64_t *kc) {
  const int64_t N = S - 1, bins = (N + 1) / 2 - 1;
  int64_t L = 1;
  while (L < 2 * N - 1) L <<= 1;
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
    for (auto it = g_pol_cache.begin(); it != g_pol_cache.end(); ++it)
      if (it->device == device && it->S == S && it->G == G) {
        g_pol_cache.splice(g_pol_cache.begin(), g_pol_cache, it);
        b = &g_pol_cache.front();
        break;
      }
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
      g_pol_cache.pop_front();
      b = nullptr;
      gmax = std::min(fit, G - 1);
      if (gmax < 1) return RN_ERR_OUT_OF_MEMORY;
    }
  }
  if (!b) return RN_ERR_OUT_OF_MEMORY;
  while (g_pol_cache.size() > kPolCacheEntries) g_pol_cache.pop_back();
  const size_t spare = limit - b->fixed_bytes - (size_t)K * kPairs * sizeof(double);
  *kc = std::max<int64_t>(1, std::min<int64_t>({K, (int64_t)(spare / ((size_t)bins * sizeof(double))),
                                                 kMaxBlockConfigs}));
  *out = b;
  return RN_OK;
}

int ensure(void **buf, size_t *have, size_t want) {
  if (*buf && *have == want) return RN_OK;
  if (*buf) (void)hipFree(*buf);
  *buf = nullptr;
  *have = 0;
  if (hipMalloc(buf, want) != hipSuccess) {
    *buf = nullptr;
    return RN_ERR_OUT_OF_MEMORY;
  }
  *have = want;
  return RN_OK;
}

// d_alpha: device float64[S][3][3]; fills b.c with the 21 basis spectra; null stream
int basis_on_device(PolPlans &b, const double *d_alpha) {
  FftApi &api = fft_api();
  const int64_t N = b.S - 1, L = b.L, bins = (N + 1) / 2 - 1;
  auto *x = static_cast<hipfftDoubleComplex *>(b.x), *p = static_cast<hipfftDoubleComplex *>(b.p);
  const unsigned gl = (unsigned)((L + 255) / 256), gn = (unsigned)((N + 255) / 256),
                 gb = (unsigned)((bins + 255) / 256);
  build_components_kernel<<<gl, 256>>>(d_alpha, N, L, x);
  if (api.exec_z2z(b.plan_x, x, x, HIPFFT_FORWARD) != HIPFFT_SUCCESS) return RN_ERR_HIP;
  for (int first = 0; first < kPairs; first += b.G) {
    const int count = std::min(b.G, kPairs - first);
    cross_power_kernel<<<dim3(gl, (unsigned)b.G), 256>>>(x, L, first, count, b.G, p);
    if (api.exec_z2z(b.plan_inv, p, p, HIPFFT_BACKWARD) != HIPFFT_SUCCESS) return RN_ERR_HIP;
    lags_kernel<<<dim3(gn, (unsigned)b.G), 256>>>(p, N, L, 1.0 / (double)L);
    if (api.exec_z2z(b.plan_n, p, p, HIPFFT_FORWARD) != HIPFFT_SUCCESS) return RN_ERR_HIP;
    basis_bins_kernel<<<dim3(gb, (unsigned)count), 256>>>(p, L, bins, first, count, static_cast<double *>(b.c));
  }
  if (hipGetLastError() != hipSuccess) return RN_ERR_HIP;
  return RN_OK;
}

// weights (host [K][21]) -> intensities (host [K][bins]), kc configurations at a time
int contract_to_host(PolPlans &b, const double *weights, int64_t K, int64_t kc, double *intensities) {
  const int64_t bins = b.S / 2 - 1;  // (N + 1) / 2 - 1 with N = S - 1
  int rc;
  if ((rc = ensure(&b.w, &b.w_bytes, (size_t)K * kPairs * sizeof(double))) != RN_OK) return rc;
  if ((rc = ensure(&b.out, &b.out_bytes, (size_t)kc * bins * sizeof(double))) != RN_OK) return rc;
  if (hipMemcpy(b.w, weights, (size_t)K * kPairs * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
    return RN_ERR_HIP;
  const auto *w = static_cast<const double *>(b.w);
  const auto *c = static_cast<const double *>(b.c);
  auto *o = static_cast<double *>(b.out);
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
  if (b.out_bytes > kKeepOutputBytes) {  // the cache keeps the basis, not a large block of intensities
    (void)hipFree(b.out);
    b.out = nullptr;
    b.out_bytes = 0;
  }
  return RN_OK;
}

int check_args(const void *alpha, const double *weights, int64_t K, const void *intensities, int64_t S,
               int64_t num_bins, int device) {
  const int64_t N = S - 1;
  if (!alpha || !weights || !intensities || K < 1 || K > ((int64_t)1 << 40) || S < 3 ||
      num_bins != (N + 1) / 2 - 1 || N > (int64_t)1 << 28)
    return RN_ERR_INVALID_ARGUMENT;
  if (!fft_api().ok) return RN_ERR_UNSUPPORTED;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return RN_ERR_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return RN_ERR_HIP;
  return RN_OK;
}

}  // namespace

extern "C" int rn_md_raman_polarized(const double *alpha, int64_t S, const double *weights, int64_t K, int device,
                                     size_t workspace_limit, double *intensities, int64_t num_bins) {
  int rc = check_args(alpha, weights, K, intensities, S, num_bins, device);
  if (rc != RN_OK || num_bins == 0) return rc;
  const size_t limit = workspace_limit ? workspace_limit : kDefaultWorkspace;
  std::lock_guard<std::mutex> lock(g_pol_mutex);
  PolPlans *b = nullptr;
  int64_t kc = 0;
  if ((rc = get_plans(device, S, K, limit, &b, &kc)) != RN_OK) return rc;
  // the host copy of alpha is staged outside the workspace accounting, as rn_md_raman_intensities does
  if (!b->alpha && hipMalloc(&b->alpha, (size_t)S * 9 * sizeof(double)) != hipSuccess) return RN_ERR_OUT_OF_MEMORY;
  if (hipMemcpy(b->alpha, alpha, (size_t)S * 9 * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
    return RN_ERR_HIP;
  if ((rc = basis_on_device(*b, static_cast<const double *>(b->alpha))) != RN_OK) return rc;
  return contract_to_host(*b, weights, K, kc, intensities);
}

extern "C" int rn_md_raman_polarized_device(const double *d_alpha, int64_t S, const double *weights, int64_t K,
                                            int device, size_t workspace_limit, double *intensities,
                                            int64_t num_bins, void *stream) {
  int rc = check_args(d_alpha, weights, K, intensities, S, num_bins, device);
  if (rc != RN_OK || num_bins == 0) return rc;
  // the producer of d_alpha ran on `stream`: the reduction runs on the null stream after it
  if (stream && hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return RN_ERR_HIP;
  const size_t limit = workspace_limit ? workspace_limit : kDefaultWorkspace;
  std::lock_guard<std::mutex> lock(g_pol_mutex);
  PolPlans *b = nullptr;
  int64_t kc = 0;
  if ((rc = get_plans(device, S, K, limit, &b, &kc)) != RN_OK) return rc;
  if ((rc = basis_on_device(*b, d_alpha)) != RN_OK) return rc;
  return contract_to_host(*b, weights, K, kc, intensities);
}
