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
// float64 throughout; hipFFT is dlopen()ed as in spectrum.hip.  Plans and work buffers are cached per (device, N, G, B) in
// a cache of their own, apart from the caches of rn_md_raman_intensities and rn_md_raman_polarized.  All work runs on the
// null stream (after a synchronise of the caller's stream in the _device entry).
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
constexpr int kMaxGroups = 16;
constexpr int kMaxSlots = 64;  // rows per FFT block
constexpr size_t kDefaultWorkspace = (size_t)4 << 30;

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

// index p of the packed upper triangle of an n x n matrix -> (j, l), j <= l, row-major: (0,0) (0,1) .. (0,n-1) (1,1) ..
__host__ __device__ inline void upper_pair(int p, int n, int &j, int &l) {
  j = 0;
  int row = n;
  while (p >= row) {
    p -= row;
    ++j;
    --row;
  }
  l = j + p;
}

// x[g*6 + c][n] for n < N from the symmetric part of incr[n][g]; zero for N <= n < L
__global__ void build_group_components_kernel(const double *__restrict__ incr, int64_t N, int64_t L, int G,
                                              hipfftDoubleComplex *__restrict__ x) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int g = blockIdx.y;
  if (n >= L || g >= G) return;
  double s[kComponents] = {0, 0, 0, 0, 0, 0};
  if (n < N) {
    const double *d = incr + (n * G + g) * 9;
    s[0] = d[0];
    s[1] = d[4];
    s[2] = d[8];
    s[3] = 0.5 * (d[1] + d[3]);
    s[4] = 0.5 * (d[5] + d[7]);
    s[5] = 0.5 * (d[2] + d[6]);
  }
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

// the positive lags 0..N-1 of each slot, real part scaled by 1/L, in place
__global__ void partial_lags_kernel(hipfftDoubleComplex *__restrict__ p, int64_t N, int64_t L, double scale) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y;
  if (k >= N) return;
  hipfftDoubleComplex *q = p + (int64_t)j * L + k;
  *q = make_double2(q->x * scale, 0.0);
}

// out[j][m] = Re(Y_j[m + 1]) for the block's real slots (the zero-frequency bin is dropped)
__global__ void partial_bins_kernel(const hipfftDoubleComplex *__restrict__ y, int64_t L, int64_t bins, int count,
                                    double *__restrict__ out) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y;
  if (m >= bins || j >= count) return;
  out[(int64_t)j * bins + m] = y[(int64_t)j * L + m + 1].x;
}

// plans + work buffers of one (device, N, G, B)
struct PartialPlans {
  int device = -1;
  int64_t N = 0, L = 0;
  int G = 0, B = 0;
  void *x = nullptr, *p = nullptr, *out = nullptr, *incr = nullptr, *w = nullptr;
  size_t incr_bytes = 0, w_bytes = 0;
  size_t fixed_bytes = 0;  // x + p + out + the plans' work areas
  hipfftHandle plan_x = 0, plan_inv = 0, plan_n = 0;
  bool have_x = false, have_inv = false, have_n = false;
  ~PartialPlans() {
    FftApi &api = fft_api();
    if (api.ok) {
      if (have_x) api.destroy(plan_x);
      if (have_inv) api.destroy(plan_inv);
      if (have_n) api.destroy(plan_n);
    }
    for (void *q : {x, p, out, incr, w})
      if (q) (void)hipFree(q);
  }
};
std::mutex g_partial_mutex;
std::list<PartialPlans> g_partial_cache;  // front = most recently used; apart from the other two spectrum caches
constexpr size_t kPartialCacheEntries = 4;

size_t plan_work(hipfftHandle h) {
  size_t bytes = 0;
  FftApi &api = fft_api();
  if (api.get_size && api.get_size(h, &bytes) != HIPFFT_SUCCESS) bytes = 0;
  return bytes;
}

int64_t padded_length(int64_t N) {
  int64_t L = 1;
  while (L < 2 * N - 1) L <<= 1;
  return L;
}

// the bytes of a call's buffers besides the plans' work areas and the staged inputs
size_t buffer_bytes(int64_t L, int64_t bins, int G, int B) {
  const size_t cz = sizeof(hipfftDoubleComplex);
  return (size_t)kComponents * G * L * cz + (size_t)B * L * cz + (size_t)B * bins * sizeof(double);
}

int make_plans(int device, int64_t N, int G, int B, PartialPlans **out) {
  FftApi &api = fft_api();
  const int64_t L = padded_length(N), bins = (N + 1) / 2 - 1;
  g_partial_cache.emplace_front();
  PartialPlans &b = g_partial_cache.front();
  b.device = device;
  b.N = N;
  b.L = L;
  b.G = G;
  b.B = B;
  const size_t cz = sizeof(hipfftDoubleComplex);
  int rc = RN_OK;
  if (hipMalloc(&b.x, (size_t)kComponents * G * L * cz) != hipSuccess || hipMalloc(&b.p, (size_t)B * L * cz) != hipSuccess ||
      hipMalloc(&b.out, (size_t)B * bins * sizeof(double)) != hipSuccess)
    rc = RN_ERR_OUT_OF_MEMORY;
  int nl = (int)L, nn = (int)N;
  if (rc == RN_OK) {
    b.have_x = api.plan_many(&b.plan_x, 1, &nl, nullptr, 1, nl, nullptr, 1, nl, HIPFFT_Z2Z, kComponents * G) ==
               HIPFFT_SUCCESS;
    b.have_inv = api.plan_many(&b.plan_inv, 1, &nl, nullptr, 1, nl, nullptr, 1, nl, HIPFFT_Z2Z, B) == HIPFFT_SUCCESS;
    b.have_n = api.plan_many(&b.plan_n, 1, &nn, &nl, 1, nl, &nl, 1, nl, HIPFFT_Z2Z, B) == HIPFFT_SUCCESS;
    if (!(b.have_x && b.have_inv && b.have_n)) rc = RN_ERR_HIP;
  }
  if (rc != RN_OK) {
    g_partial_cache.pop_front();
    return rc;
  }
  b.fixed_bytes = buffer_bytes(L, bins, G, B) + plan_work(b.plan_x) + plan_work(b.plan_inv) + plan_work(b.plan_n);
  *out = &b;
  return RN_OK;
}

// finds or creates the entry for (device, N, G) with as many rows per block as fit `limit` beside K configurations'
// weights (at most kMaxSlots, at most the number of rows)
int get_plans(int device, int64_t N, int G, int64_t K, size_t limit, PartialPlans **out) {
  const int64_t L = padded_length(N), bins = (N + 1) / 2 - 1;
  const int64_t rows = K * G * (G + 1) / 2;
  const size_t wbytes = (size_t)K * kPairs * sizeof(double);
  const size_t per_slot = (size_t)L * sizeof(hipfftDoubleComplex) + (size_t)bins * sizeof(double);
  const size_t base = buffer_bytes(L, bins, G, 0) + wbytes;
  if (limit < base + per_slot) return RN_ERR_OUT_OF_MEMORY;
  int bmax = (int)std::min<int64_t>({(int64_t)kMaxSlots, rows, (int64_t)((limit - base) / per_slot)});
  for (int attempt = 0; attempt < 3; ++attempt) {
    PartialPlans *b = nullptr;
    for (auto it = g_partial_cache.begin(); it != g_partial_cache.end(); ++it)
      if (it->device == device && it->N == N && it->G == G && it->B == bmax) {
        g_partial_cache.splice(g_partial_cache.begin(), g_partial_cache, it);
        b = &g_partial_cache.front();
        break;
      }
    if (!b) {
      int rc = make_plans(device, N, G, bmax, &b);
      if (rc != RN_OK) return rc;
    }
    if (b->fixed_bytes + wbytes <= limit) {
      while (g_partial_cache.size() > kPartialCacheEntries) g_partial_cache.pop_back();
      *out = &g_partial_cache.front();
      return RN_OK;
    }
    // the plans' work areas do not fit beside the buffers: fewer rows per block (the inverse / length-N work scales with B)
    const size_t work = b->fixed_bytes - buffer_bytes(L, bins, G, bmax);
    g_partial_cache.pop_front();
    const size_t slot = per_slot + work / (size_t)bmax;
    const int fit = limit > base ? (int)std::min<size_t>((limit - base) / slot, (size_t)kMaxSlots) : 0;
    bmax = std::min(fit, bmax - 1);
    if (bmax < 1) return RN_ERR_OUT_OF_MEMORY;
  }
  return RN_ERR_OUT_OF_MEMORY;
}

int ensure(void **buf, size_t *have, size_t want) {
  if (*buf && *have >= want) return RN_OK;
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

// d_incr: device float64[N][G][9] -> out: host float64[K][G(G+1)/2][bins]; null stream
int partial_on_device(PartialPlans &b, const double *d_incr, const double *weights, int64_t K, double *out) {
  FftApi &api = fft_api();
  const int64_t N = b.N, L = b.L, bins = (N + 1) / 2 - 1;
  const int G = b.G, B = b.B;
  const int64_t rows = K * G * (G + 1) / 2;
  int rc;
  if ((rc = ensure(&b.w, &b.w_bytes, (size_t)K * kPairs * sizeof(double))) != RN_OK) return rc;
  if (hipMemcpy(b.w, weights, (size_t)K * kPairs * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
    return RN_ERR_HIP;
  auto *x = static_cast<hipfftDoubleComplex *>(b.x), *p = static_cast<hipfftDoubleComplex *>(b.p);
  const unsigned gl = (unsigned)((L + 255) / 256), gn = (unsigned)((N + 255) / 256),
                 gb = (unsigned)((bins + 255) / 256);
  build_group_components_kernel<<<dim3(gl, (unsigned)G), 256>>>(d_incr, N, L, G, x);
  if (api.exec_z2z(b.plan_x, x, x, HIPFFT_FORWARD) != HIPFFT_SUCCESS) return RN_ERR_HIP;
  for (int64_t r0 = 0; r0 < rows; r0 += B) {
    const int count = (int)std::min<int64_t>(B, rows - r0);
    partial_contract_kernel<<<dim3(gl, (unsigned)B), 256>>>(x, L, static_cast<const double *>(b.w), r0, count, G, p);
    if (api.exec_z2z(b.plan_inv, p, p, HIPFFT_BACKWARD) != HIPFFT_SUCCESS) return RN_ERR_HIP;
    partial_lags_kernel<<<dim3(gn, (unsigned)B), 256>>>(p, N, L, 1.0 / (double)L);
    if (api.exec_z2z(b.plan_n, p, p, HIPFFT_FORWARD) != HIPFFT_SUCCESS) return RN_ERR_HIP;
    partial_bins_kernel<<<dim3(gb, (unsigned)count), 256>>>(p, L, bins, count, static_cast<double *>(b.out));
    if (hipGetLastError() != hipSuccess) return RN_ERR_HIP;
    if (hipMemcpy(out + r0 * bins, b.out, (size_t)count * bins * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      return RN_ERR_HIP;
  }
  return RN_OK;
}

int check_args(const void *incr, int64_t N, int G, const double *weights, int64_t K, const void *out, int64_t num_bins,
               int device) {
  if (!incr || !weights || !out || K < 1 || K > ((int64_t)1 << 40) || G < 1 || G > kMaxGroups || N < 2 ||
      N > (int64_t)1 << 28 || num_bins != (N + 1) / 2 - 1)
    return RN_ERR_INVALID_ARGUMENT;
  if (!fft_api().ok) return RN_ERR_UNSUPPORTED;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return RN_ERR_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return RN_ERR_HIP;
  return RN_OK;
}

}  // namespace

extern "C" int rn_md_raman_partial(const double *increments, int64_t N, int G, const double *weights, int64_t K,
                                   int device, size_t workspace_limit, double *intensities, int64_t num_bins) {
  int rc = check_args(increments, N, G, weights, K, intensities, num_bins, device);
  if (rc != RN_OK || num_bins == 0) return rc;
  const size_t limit = workspace_limit ? workspace_limit : kDefaultWorkspace;
  std::lock_guard<std::mutex> lock(g_partial_mutex);
  PartialPlans *b = nullptr;
  if ((rc = get_plans(device, N, G, K, limit, &b)) != RN_OK) return rc;
  // the host increments are staged outside the workspace accounting, as the other spectrum entries stage alpha
  const size_t bytes = (size_t)N * G * 9 * sizeof(double);
  if ((rc = ensure(&b->incr, &b->incr_bytes, bytes)) != RN_OK) return rc;
  if (hipMemcpy(b->incr, increments, bytes, hipMemcpyHostToDevice) != hipSuccess) return RN_ERR_HIP;
  return partial_on_device(*b, static_cast<const double *>(b->incr), weights, K, intensities);
}

extern "C" int rn_md_raman_partial_device(const double *d_increments, int64_t N, int G, const double *weights,
                                          int64_t K, int device, size_t workspace_limit, double *intensities,
                                          int64_t num_bins, void *stream) {
  int rc = check_args(d_increments, N, G, weights, K, intensities, num_bins, device);
  if (rc != RN_OK || num_bins == 0) return rc;
  // the producer of d_increments ran on `stream`: the reduction runs on the null stream after it
  if (stream && hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return RN_ERR_HIP;
  const size_t limit = workspace_limit ? workspace_limit : kDefaultWorkspace;
  std::lock_guard<std::mutex> lock(g_partial_mutex);
  PartialPlans *b = nullptr;
  if ((rc = get_plans(device, N, G, K, limit, &b)) != RN_OK) return rc;
  return partial_on_device(*b, d_increments, weights, K, intensities);
}
