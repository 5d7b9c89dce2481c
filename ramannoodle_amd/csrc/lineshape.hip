// Lorentzian line-shape fits of spectrum rows, one wave per fit (include/rn_lineshape.h; the definition is
// fit_lorentzians_host of ramannoodle_amd/lineshape.py, and every step below follows it operation for operation).
//
// Kernel.  A workgroup is four waves and a wave owns fit 4 blockIdx.x + wave; waves share nothing (no LDS, no barrier),
// so a wave past the table or on a degenerate window returns at once.  Lane l owns bins l, l + 64, .. of the window.
// The first kRegBins of them (window bins < kCapacity) are normalised once and stay in registers; the bins of a longer
// window past kCapacity are read again and divided by the maximum again in every evaluation: the same values, so the
// two paths differ in nothing but where z comes from.  An evaluation at (h, x0, g, c) accumulates the 15 sums of the
// recipe (N: 10, J^T r: 4, S) per lane in ascending bins and adds them over the lanes with an xor butterfly.  a + b and
// b + a are the same bits, so after the butterfly every lane holds identical sums, and everything that follows (the
// 4x4 elimination, the trial step, accept / reject / stop) is computed redundantly by every lane with identical
// results: the control flow is wave-uniform without a broadcast, and every shuffle runs with all 64 lanes.  The start
// values are reduced the same way (min, sum, and max with the lowest index winning a tie).  No atomics; the order of
// every sum depends on n alone, so a fit's bits do not depend on F, its place in the table or its neighbours.
// The work is latency-bound float64 VALU arithmetic (one division per bin and evaluation) and six shuffle stages per
// sum; a call launches one wave per fit and leaves the overlap to the number of waves.
//
// Entries: fit_entry.hpp, with nothing of their own but the least number of bins and the launch.
#include <cmath>
#include <cstdint>
#include <mutex>

#include "../../include/rn_lineshape.h"
#include "fit_entry.hpp"

namespace {

constexpr int kLanes = 64;
constexpr int kWaves = 4;                       // fits per workgroup
constexpr int kRegBins = 8;                     // bins a lane keeps in registers
constexpr int kCapacity = kRegBins * kLanes;    // rn_lineshape_window_capacity
constexpr int kSums = 15;
constexpr int kOutputs = RN_LINESHAPE_OUTPUTS;
constexpr double kStepTolerance = 1e-10;
constexpr double kPi = 3.141592653589793;

struct Params {
  double h, x0, g, c;
};

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int m = kLanes / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// one bin's terms of the 15 sums (lineshape.py, _sums): s[0..9] the upper triangle of J^T J in the order
// (h, x0, g, c), s[10..13] J^T r, s[14] r^2
__device__ inline void add_terms(double z, double x, const Params &p, double g2, double inv_g, double (&s)[kSums]) {
  const double d = x - p.x0;
  const double inv = 1.0 / (d * d + g2);
  const double l = g2 * inv;
  const double r = z - (p.h * l + p.c);
  const double u = (p.h + p.h) * l * inv;
  const double jx = u * d;
  const double jg = jx * d * inv_g;
  s[0] += l * l;
  s[1] += l * jx;
  s[2] += l * jg;
  s[3] += l;
  s[4] += jx * jx;
  s[5] += jx * jg;
  s[6] += jx;
  s[7] += jg * jg;
  s[8] += jg;
  s[9] += 1.0;
  s[10] += l * r;
  s[11] += jx * r;
  s[12] += jg * r;
  s[13] += r;
  s[14] += r * r;
}

// delta of (N + damping diag N) delta = J^T r: elimination without pivoting, rows in the order (h, x0, g, c)
__device__ inline void solve(const double (&s)[kSums], double damping, double (&delta)[4]) {
  double a[4][5];
  int k = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = i; j < 4; ++j) {
      a[i][j] = s[k];
      a[j][i] = s[k];
      ++k;
    }
    a[i][4] = s[10 + i];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i][i] = a[i][i] + damping * a[i][i];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i + 1; j < 4; ++j) {
      const double f = a[j][i] / a[i][i];
#pragma unroll
      for (int m = i + 1; m < 5; ++m) a[j][m] = a[j][m] - f * a[i][m];
    }
#pragma unroll
  for (int i = 3; i >= 0; --i) {
    double t = a[i][4];
#pragma unroll
    for (int j = i + 1; j < 4; ++j) t = t - a[i][j] * delta[j];
    delta[i] = t / a[i][i];
  }
}

__global__ void __launch_bounds__(kWaves *kLanes)
    lineshape_fit_kernel(const double *__restrict__ rows, int64_t bins, const int64_t *__restrict__ row_index,
                         const int64_t *__restrict__ first_bin, const int64_t *__restrict__ num_bins, int64_t F,
                         int max_iterations, double *__restrict__ out, int32_t *__restrict__ status,
                         int32_t *__restrict__ iterations) {
  const int lane = threadIdx.x & (kLanes - 1);
  const int64_t fit = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (fit >= F) return;
  const int64_t n = num_bins[fit];
  const double *__restrict__ y = rows + row_index[fit] * bins + first_bin[fit];
  double *result = out + fit * kOutputs;

  // the window: finite?  max (lowest index on a tie) and min
  double zreg[kRegBins];
  bool bad = false;
  double top = -INFINITY, low = INFINITY;
  int64_t peak = n;
#pragma unroll
  for (int j = 0; j < kRegBins; ++j) {
    const int64_t i = lane + kLanes * j;
    zreg[j] = 0.0;
    if (i < n) {
      const double v = y[i];
      zreg[j] = v;
      bad |= !std::isfinite(v);
      if (v > top) {
        top = v;
        peak = i;
      }
      low = v < low ? v : low;
    }
  }
  for (int64_t i = lane + kCapacity; i < n; i += kLanes) {
    const double v = y[i];
    bad |= !std::isfinite(v);
    if (v > top) {
      top = v;
      peak = i;
    }
    low = v < low ? v : low;
  }
  bool degenerate = __any(bad) != 0;
  if (!degenerate) {
#pragma unroll
    for (int m = kLanes / 2; m >= 1; m >>= 1) {
      const double other_top = __shfl_xor(top, m), other_low = __shfl_xor(low, m);
      const int other_peak = __shfl_xor((int)peak, m);  // (n < 2^31: checked by the entry)
      if (other_top > top || (other_top == top && other_peak < peak)) {
        top = other_top;
        peak = other_peak;
      }
      low = other_low < low ? other_low : low;
    }
    degenerate = top <= 0.0 || top == low;
  }
  if (degenerate) {
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < kOutputs; ++k) result[k] = NAN;
      status[fit] = 2;
      iterations[fit] = 0;
    }
    return;
  }

  // normalise; the moments and the start values
#pragma unroll
  for (int j = 0; j < kRegBins; ++j) zreg[j] = zreg[j] / top;
  const double c0 = low / top;
  double total = 0.0, moment = 0.0, above = 0.0;
#pragma unroll
  for (int j = 0; j < kRegBins; ++j) {
    const int64_t i = lane + kLanes * j;
    if (i < n) {
      total += zreg[j];
      moment += (double)i * zreg[j];
      above += zreg[j] - c0;
    }
  }
  for (int64_t i = lane + kCapacity; i < n; i += kLanes) {
    const double z = y[i] / top;
    total += z;
    moment += (double)i * z;
    above += z - c0;
  }
  total = wave_sum(total);
  moment = wave_sum(moment);
  above = wave_sum(above);

  Params p;
  p.c = c0;
  p.h = 1.0 - c0;  // z[peak] = top / top
  p.x0 = (double)peak;
  p.g = above / (kPi * p.h);
  p.g = p.g < 0.5 ? 0.5 : p.g;
  p.g = p.g > 0.5 * (double)n ? 0.5 * (double)n : p.g;

  auto evaluate = [&](const Params &at, double(&s)[kSums]) {
#pragma unroll
    for (int k = 0; k < kSums; ++k) s[k] = 0.0;
    const double g2 = at.g * at.g, inv_g = 1.0 / at.g;
#pragma unroll
    for (int j = 0; j < kRegBins; ++j) {
      const int64_t i = lane + kLanes * j;
      if (i < n) add_terms(zreg[j], (double)i, at, g2, inv_g, s);
    }
    for (int64_t i = lane + kCapacity; i < n; i += kLanes) add_terms(y[i] / top, (double)i, at, g2, inv_g, s);
#pragma unroll
    for (int k = 0; k < kSums; ++k) s[k] = wave_sum(s[k]);
  };

  double sums[kSums], trial_sums[kSums];
  evaluate(p, sums);
  double damping = 1e-3;
  int state = 1, count = 0;
  const double nd = (double)n;
  while (count < max_iterations) {
    ++count;
    double delta[4];
    solve(sums, damping, delta);
    const bool finite =
        std::isfinite(delta[0]) && std::isfinite(delta[1]) && std::isfinite(delta[2]) && std::isfinite(delta[3]);
    const bool small = finite && fabs(delta[0]) / p.h <= kStepTolerance && fabs(delta[1]) / p.g <= kStepTolerance &&
                       fabs(delta[2]) / p.g <= kStepTolerance && fabs(delta[3]) / p.h <= kStepTolerance;
    Params trial;
    trial.h = p.h + delta[0];
    trial.x0 = p.x0 + delta[1];
    trial.g = p.g + delta[2];
    trial.c = p.c + delta[3];
    bool accepted = false;
    if (finite && trial.h > 0.0 && trial.g >= 0.125 && trial.g <= 4.0 * nd && trial.x0 >= -nd && trial.x0 <= 2.0 * nd) {
      evaluate(trial, trial_sums);
      accepted = trial_sums[14] <= sums[14];
    }
    if (accepted) {
      p = trial;
#pragma unroll
      for (int k = 0; k < kSums; ++k) sums[k] = trial_sums[k];
      damping = damping / 10.0;
      damping = damping < 1e-12 ? 1e-12 : damping;
      if (small) {
        state = 0;
        break;
      }
    } else {
      if (small) {
        state = 0;
        break;
      }
      damping = damping * 10.0;
      if (damping > 1e12) {
        state = 3;
        break;
      }
    }
  }
  if (lane == 0) {
    result[0] = p.h;
    result[1] = p.x0;
    result[2] = p.g;
    result[3] = p.c;
    result[4] = sums[14];
    result[5] = top;
    result[6] = total;
    result[7] = total != 0.0 ? moment / total : NAN;
    status[fit] = state;
    iterations[fit] = count;
  }
}

// ----------------------------------------------------------------------------- entries
using rn_fit::FitArgs;
thread_local rn_spectrum::ErrorText g_error;
rn_fit::FitWorkspace g_fits(kOutputs);

int lineshape_fit(int device, const FitArgs &a) {
  if (int rc = rn_fit::check_sizes(a, g_error)) return rc;
  if (a.F == 0) return RN_OK;
  if (a.any_null()) return g_error.fail(RN_ERR_INVALID_ARGUMENT, "a null pointer");
  for (int64_t f = 0; f < a.F; ++f) {
    if (int rc = rn_fit::check_row(a, f, g_error)) return rc;
    if (a.num_bins[f] < RN_LINESHAPE_MIN_BINS)
      return g_error.fail(RN_ERR_INVALID_ARGUMENT, "fit %lld: %lld bins, a fit needs at least %d", (long long)f,
                          (long long)a.num_bins[f], RN_LINESHAPE_MIN_BINS);
    if (int rc = rn_fit::check_window(a, f, g_error)) return rc;
  }
  if (int rc = rn_spectrum::select_device(device, g_error)) return rc;

  std::lock_guard<std::mutex> lock(g_fits.mutex);
  g_fits.bind(device);
  if (g_fits.ensure(a) != RN_OK) return g_fits.no_memory(a, g_error);
  rn_spectrum::FirstError ok;
  const double *d_rows = g_fits.stage(a, ok);
  if (ok.first == hipSuccess) {
    lineshape_fit_kernel<<<rn_fit::fit_blocks(a.F, kWaves), kWaves * kLanes, 0, a.stream>>>(
        d_rows, a.bins, g_fits.column(a, 0), g_fits.column(a, 1), g_fits.column(a, 2), a.F, a.max_iterations,
        g_fits.d_out(), g_fits.d_status(), g_fits.d_iterations(a));
    ok(hipGetLastError());
  }
  return g_fits.finish(a, ok, g_error);
}

}  // namespace

extern "C" int rn_lineshape_fit(int device, const double *rows, int64_t num_rows, int64_t bins,
                                const int64_t *row_index, const int64_t *first_bin, const int64_t *num_bins, int64_t F,
                                int max_iterations, double *out, int32_t *status, int32_t *iterations) {
  return lineshape_fit(device, {rows, true, num_rows, bins, row_index, first_bin, num_bins, F, max_iterations, out, status,
                                iterations, nullptr});
}

extern "C" int rn_lineshape_fit_device(int device, const double *d_rows, int64_t num_rows, int64_t bins,
                                       const int64_t *row_index, const int64_t *first_bin, const int64_t *num_bins,
                                       int64_t F, int max_iterations, double *out, int32_t *status, int32_t *iterations,
                                       void *stream) {
  return lineshape_fit(device, {d_rows, false, num_rows, bins, row_index, first_bin, num_bins, F, max_iterations, out,
                                status, iterations, static_cast<hipStream_t>(stream)});
}

extern "C" int rn_lineshape_window_capacity(void) { return kCapacity; }

extern "C" const char *rn_lineshape_last_error(void) { return g_error.text.c_str(); }
