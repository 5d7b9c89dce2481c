// What the on-device MD spectrum reducers share (spectrum.hip, spectrum_polarized.hip, spectrum_partial.hip,
// spectrum_segments.hip, spectrum_ensemble.hip, spectrum_vdos.hip, spectrum_mode_vdos.hip, spectrum_modes.hip): the hipFFT loader, the
// series-length arithmetic, the RAII holder for plans, the most-recently-used plan cache, the argument / device check
// and the two per-slot kernels of the polarized, partial and segment pipelines; the holder for device buffers and the
// host-or-HBM source of a call come from entry_runtime.hpp.  The three whole-run reducers each keep their own signal
// builder, power / contraction kernel, plans struct, workspace arithmetic and pipeline; the segment reducers (the last
// five files) share those through spectrum_segment_core.hpp, and the two that read positions share their front end
// through spectrum_steps.hpp.
//
// Two decisions that hold for every reducer:
//  * Buffer sizing.  The rule is at the head of entry_runtime.hpp (Fit::kExact for what `workspace_limit` counts,
//    Fit::kGrowOnly for the rest).  Here the limit counts the weights, the taper, the polarized output block and the
//    fixed x / p / c / out buffers of an entry; the staged copies of a host input (`alpha`, `incr`) are outside the
//    accounting by rn_potgnn.h's own words.
//  * Shrink and retry.  The polarized reducer shrinks G (pairs per group, then balanced over ceil(21/G) groups), the
//    partial reducer shrinks B (rows per block, capped by the row count) and the segment reducers shrink B and R
//    (segments and rows per block) together.  The three differ in the key, the balancing, the per-slot cost and what
//    the leftover bytes are used for, and share only "make, measure the work areas, drop": the polarized and the partial
//    reducer each keep their own loop over the shared cache and arithmetic below.  The segment reducers have one loop,
//    get_segment_plans of spectrum_segment_core.hpp, which takes the block chooser as a callable.
#pragma once
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>

#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <list>
#include <mutex>

#include "../../include/rn_potgnn.h"
#include "entry_runtime.hpp"

namespace rn_spectrum {

constexpr int kComponents = 6;  // (xx, yy, zz, xy, yz, xz) of a symmetric 3x3 block
constexpr int kPairs = 21;      // pairs j <= l of the components: the packed weights of a symmetric 6x6 form
constexpr size_t kDefaultWorkspace = (size_t)4 << 30;  // workspace_limit = 0
constexpr size_t kCacheEntries = 4;

// hipFFT, loaded on first use so that the library itself does not depend on it; one table for the whole library
struct FftApi {
  void *lib = nullptr;
  hipfftResult (*plan_many)(hipfftHandle *, int, int *, int *, int, int, int *, int, int, hipfftType, int) = nullptr;
  hipfftResult (*exec_z2z)(hipfftHandle, hipfftDoubleComplex *, hipfftDoubleComplex *, int) = nullptr;
  hipfftResult (*destroy)(hipfftHandle) = nullptr;
  hipfftResult (*get_size)(hipfftHandle, size_t *) = nullptr;  // optional
  bool ok = false;
};
inline FftApi &fft_api() {
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

// N = S - 1 differences of an S-step series: the zero-padded transform length L >= 2N - 1 (a power of two) ...
inline int64_t padded_length(int64_t N) {
  int64_t L = 1;
  while (L < 2 * N - 1) L <<= 1;
  return L;
}
// ... and the number of returned bins: the non-negative frequencies of fftfreq(N) without the zero bin
inline int64_t num_bins(int64_t N) { return (N + 1) / 2 - 1; }

inline unsigned blocks_of_256(int64_t n) { return (unsigned)((n + 255) / 256); }

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

// the six components of the symmetric part of a row-major 3x3 block
__device__ inline void symmetric_components(const double *d, double *s) {
  s[0] = d[0];
  s[1] = d[4];
  s[2] = d[8];
  s[3] = 0.5 * (d[1] + d[3]);
  s[4] = 0.5 * (d[5] + d[7]);
  s[5] = 0.5 * (d[2] + d[6]);
}

// A batch of slots, each a length-L complex row: the positive lags 0..N-1 of each slot (blockIdx.y), real part scaled
// by 1/L, in place ...
static __global__ void slot_lags_kernel(hipfftDoubleComplex *__restrict__ p, int64_t N, int64_t L, double scale) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int g = blockIdx.y;
  if (k >= N) return;
  hipfftDoubleComplex *q = p + (int64_t)g * L + k;
  *q = make_double2(q->x * scale, 0.0);
}
// ... and out[g][m] = Re(Y_g[m + 1]) for the first `count` slots (the zero-frequency bin is dropped)
static __global__ void slot_bins_kernel(const hipfftDoubleComplex *__restrict__ y, int64_t L, int64_t bins, int count,
                                        double *__restrict__ out) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int g = blockIdx.y;
  if (m >= bins || g >= count) return;
  out[(int64_t)g * bins + m] = y[(int64_t)g * L + m + 1].x;
}

// a 1-D Z2Z hipFFT plan, destroyed with its holder
struct FftPlan {
  hipfftHandle handle = 0;
  bool made = false;
  FftPlan() = default;
  FftPlan(const FftPlan &) = delete;
  FftPlan &operator=(const FftPlan &) = delete;
  ~FftPlan() {
    if (made) fft_api().destroy(handle);
  }
  // `batch` transforms of length n: contiguous rows (slot = 0), or each at the start of its length-`slot` row
  bool make(int n, int batch, int slot = 0) {
    int *embed = slot ? &slot : nullptr;
    const int dist = slot ? slot : n;
    made = fft_api().plan_many(&handle, 1, &n, embed, 1, dist, embed, 1, dist, HIPFFT_Z2Z, batch) == HIPFFT_SUCCESS;
    return made;
  }
  size_t work_bytes() const {  // hipFFT's work area, 0 where it cannot be asked
    size_t bytes = 0;
    FftApi &api = fft_api();
    if (api.get_size && api.get_size(handle, &bytes) != HIPFFT_SUCCESS) bytes = 0;
    return bytes;
  }
  bool exec(void *data, int direction) const {  // in place, on the null stream
    auto *z = static_cast<hipfftDoubleComplex *>(data);
    return fft_api().exec_z2z(handle, z, z, direction) == HIPFFT_SUCCESS;
  }
};

// Most-recently-used cache of one reducer's plans (front = most recent), instantiated once per reducer so that the
// caches stay apart and each keeps kCacheEntries entries.  The caller holds `mutex` for the whole call.
template <class Entry>
struct PlanCache {
  std::mutex mutex;
  std::list<Entry> entries;
  template <class Match>
  Entry *find(Match match) {
    for (auto it = entries.begin(); it != entries.end(); ++it)
      if (match(*it)) {
        entries.splice(entries.begin(), entries, it);
        return &entries.front();
      }
    return nullptr;
  }
  Entry &emplace_front() {
    entries.emplace_front();
    return entries.front();
  }
  void drop_front() { entries.pop_front(); }  // the entry just made (or just found) is not kept
  void trim() {
    while (entries.size() > kCacheEntries) entries.pop_back();
  }
};

// The checks every entry makes, in this order, after its own conditions (K, G): null pointers, the range of N (the
// number of differences), num_bins, hipFFT present, the device index; then selects the device.
inline int check_call(std::initializer_list<const void *> pointers, int64_t N, int64_t bins, int device) {
  for (const void *q : pointers)
    if (!q) return RN_ERR_INVALID_ARGUMENT;
  if (N < 2 || N > (int64_t)1 << 28 || bins != num_bins(N)) return RN_ERR_INVALID_ARGUMENT;
  if (!fft_api().ok) return RN_ERR_UNSUPPORTED;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return RN_ERR_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return RN_ERR_HIP;
  return RN_OK;
}

}  // namespace rn_spectrum
