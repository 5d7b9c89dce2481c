// Multi-peak line-shape fits of spectrum rows, one wave per fit (include/rn_peakfit.h; the definition is fit_peaks_host
// of ramannoodle_amd/peakfit.py, and every step below follows it operation for operation).
//
// Kernel, one instantiation per (P, baseline, shape).  A workgroup is four waves and a wave owns fit
// 4 blockIdx.x + wave; waves share nothing (each has its own LDS tile, there is no barrier), so a wave past the table or
// on a degenerate window returns at once.  Lane l owns bins l, l + 64, .. of the window; the first kRegBins of them are
// normalised once and stay in registers, the bins of a longer window past kCapacity are read and divided again in every
// evaluation: the same values.
//
// An evaluation at the parameters q forms the Gram matrix of A = [J | r | 0] (p Jacobian columns, the residual, zeros
// up to 16) on the matrix pipe.  Per chunk of 64 bins a lane writes its bin's row of A to the wave's tile (64 rows of 16
// columns; the odd row stride of 17 doubles spreads the row-wise writes and the column-wise reads over the banks), and
// reads A[4 s + quad][l15] for s = 0 .. 15 (lane = 16 quad + l15): that one value is both operands of
// v_mfma_f64_16x16x4_f64, whose A operand is (row l15, k quad) of A^T and whose B operand is (k quad, column l15) of A.
// Sixteen instructions per chunk accumulate A^T A in four registers per lane: register j of lane (l15, quad) is row
// 4 j + quad, column l15 (tools/mfma_f64_layout_probe.hip).  N = J^T J is its leading p x p block, J^T r its column p and
// S its entry (p, p).  Chunks run in ascending bins and k-steps past the last bin are skipped, so the order of every sum
// depends on n alone.
//
// The solve keeps one column of the augmented matrix per lane: lane c < 16 holds column c of A^T A (column p is the
// right-hand side) and lane 16 + c the unit column e_c, row i in register a[i]; the columns come out of the accumulators
// with one shuffle per row.  Elimination step i divides the pivot row by the pivot in every lane at once (lane j then
// holds the factor of row j) and subtracts the pivot row from the rows below with the factors read by v_readlane from
// constant lanes; back-substitution runs per lane on the lane's own column, with the triangle's entries read the same
// way.  delta is lane p's solution and (N^-1)_ii is entry i of lane 16 + i's.  Every value that steers the fit (delta,
// S, the pivots) is read into scalar registers, so the control flow is wave-uniform.  No atomics, no scratch.
//
// Entries: fit_entry.hpp, with the model's scalars, the three real columns (origin, centres, widths: one more grow-only
// buffer, staged on the same stream) and their checks next to the integer table.
#include <cmath>
#include <cstdint>
#include <mutex>

#include "../../include/rn_peakfit.h"
#include "fit_entry.hpp"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kLanes = 64;
constexpr int kWaves = 4;                       // fits per workgroup
constexpr int kRegBins = 8;                     // bins a lane keeps in registers
constexpr int kCapacity = kRegBins * kLanes;    // rn_peakfit_window_capacity
constexpr int kColumns = 16;                    // the tile of the instruction
constexpr int kStride = kColumns + 1;           // doubles per row of the LDS tile
constexpr int kOutputs = RN_PEAKFIT_OUTPUTS;
constexpr int kSlots = 14;                      // parameter (and error) slots of the outputs
constexpr double kStepTolerance = 1e-10;

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int m = kLanes / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// v of lane `from` (a constant), in scalar registers
__device__ inline double read_lane(double v, int from) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), from);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), from);
  return __hiloint2double(hi, lo);
}

// the writes of this wave to its tile are visible to its reads (LDS runs in order within a wave: this only keeps the
// compiler from moving one past the other)
__device__ inline void tile_fence() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// (N + damping diag N | J^T r | I) by columns, eliminated without pivoting in parameter order and solved: x[i] of lane c
// is entry i of the solution for column c, pivot[i] the wave-uniform pivots
template <int NP>
__device__ inline void solve(const f64x4 &gram, double damping, int lane, double (&x)[NP], double (&pivot)[NP]) {
  const int l15 = lane & 15;
  double a[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    a[i] = __shfl(gram[i >> 2], (i & 3) * 16 + l15);
    if (l15 == i) a[i] = a[i] + damping * a[i];
    if (lane >= 16) a[i] = l15 == i ? 1.0 : 0.0;
  }
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    pivot[i] = read_lane(a[i], i);
    const double factors = a[i] / pivot[i];
#pragma unroll
    for (int j = i + 1; j < NP; ++j) a[j] = a[j] - read_lane(factors, j) * a[i];
  }
#pragma unroll
  for (int i = NP - 1; i >= 0; --i) {
    double t = a[i];
#pragma unroll
    for (int j = i + 1; j < NP; ++j) t = t - read_lane(a[i], j) * x[j];
    x[i] = t / pivot[i];
  }
}

template <int P, bool LINEAR, bool DHO>
__global__ void __launch_bounds__(kWaves *kLanes)
    peakfit_kernel(const double *__restrict__ rows, int64_t bins, const int64_t *__restrict__ row_index,
                   const int64_t *__restrict__ first_bin, const int64_t *__restrict__ num_bins,
                   const double *__restrict__ origins, const double *__restrict__ centres,
                   const double *__restrict__ widths, int64_t F, int max_iterations, double *__restrict__ out,
                   int32_t *__restrict__ status, int32_t *__restrict__ iterations) {
  constexpr int NP = 3 * P + 1 + (LINEAR ? 1 : 0);  // parameters; column NP of A is the residual
  constexpr int C = 3 * P;                          // the baseline's slot
  static_assert(NP + 1 <= kColumns, "J and r fill one tile");
  __shared__ double tiles[kWaves][kLanes * kStride];
  const int lane = threadIdx.x & (kLanes - 1);
  const int l15 = lane & 15, quad = lane >> 4;
  double *tile = tiles[threadIdx.x >> 6];
  const int64_t fit = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (fit >= F) return;
  const int64_t n = num_bins[fit];
  const double *__restrict__ y = rows + row_index[fit] * bins + first_bin[fit];
  double *result = out + fit * kOutputs;

  // the window: finite?  max and min
  double zreg[kRegBins];
  bool bad = false;
  double top = -INFINITY, low = INFINITY;
#pragma unroll
  for (int j = 0; j < kRegBins; ++j) {
    const int64_t i = lane + kLanes * j;
    zreg[j] = 0.0;
    if (i < n) {
      const double v = y[i];
      zreg[j] = v;
      bad |= !std::isfinite(v);
      top = v > top ? v : top;
      low = v < low ? v : low;
    }
  }
  for (int64_t i = lane + kCapacity; i < n; i += kLanes) {
    const double v = y[i];
    bad |= !std::isfinite(v);
    top = v > top ? v : top;
    low = v < low ? v : low;
  }
  bool degenerate = __any(bad) != 0;
  if (!degenerate) {
#pragma unroll
    for (int m = kLanes / 2; m >= 1; m >>= 1) {
      const double other_top = __shfl_xor(top, m), other_low = __shfl_xor(low, m);
      top = other_top > top ? other_top : top;
      low = other_low < low ? other_low : low;
    }
    degenerate = top <= 0.0 || top == low;
  }
  if (degenerate) {
    if (lane < kOutputs) result[lane] = NAN;
    if (lane == 0) {
      status[fit] = 2;
      iterations[fit] = 0;
    }
    return;
  }

  // normalise; the moments and the start values
#pragma unroll
  for (int j = 0; j < kRegBins; ++j) zreg[j] = zreg[j] / top;
  double total = 0.0, moment = 0.0;
#pragma unroll
  for (int j = 0; j < kRegBins; ++j) {
    const int64_t i = lane + kLanes * j;
    if (i < n) {
      total += zreg[j];
      moment += (double)i * zreg[j];
    }
  }
  for (int64_t i = lane + kCapacity; i < n; i += kLanes) {
    const double z = y[i] / top;
    total += z;
    moment += (double)i * z;
  }
  total = wave_sum(total);
  moment = wave_sum(moment);

  const double nd = (double)n;
  const double origin = DHO ? origins[fit] : 0.0;
  const double middle = 0.5 * (double)(n - 1);
  double p[NP];
  p[C] = low / top;
  if (LINEAR) p[C + 1] = 0.0;
#pragma unroll
  for (int k = 0; k < P; ++k) {
    const double centre = centres[fit * P + k];
    const double h = y[(int64_t)rint(centre)] / top - p[C];  // (0 <= centre <= n - 1: checked by the entry)
    p[3 * k] = h > 1e-3 ? h : 1e-3;
    p[3 * k + 1] = centre;
    double g = widths[fit * P + k];
    g = g < 0.5 ? 0.5 : g;
    p[3 * k + 2] = g > 0.5 * nd ? 0.5 * nd : g;
  }

  // the columns of the tile that no row of A fills stay zero
#pragma unroll
  for (int k = NP + 1; k < kColumns; ++k) tile[lane * kStride + k] = 0.0;

  auto evaluate = [&](const double(&at)[NP], f64x4 &gram) {
    gram = f64x4{0.0, 0.0, 0.0, 0.0};
    double g2[P], scale_g[P], ahead[P];  // per peak: g^2 | 2 g, 1 / g | 1 / (2 g), 2 h | 4 h
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const double h = at[3 * k], g = at[3 * k + 2];
      g2[k] = DHO ? g + g : g * g;
      scale_g[k] = DHO ? 0.5 / g : 1.0 / g;
      ahead[k] = DHO ? 4.0 * h : h + h;
    }
    auto chunk = [&](double z, int64_t first) {
      const int64_t i = first + lane;
      const double x = (double)i;
      double row[NP + 1];
      double model = 0.0;
#pragma unroll
      for (int k = 0; k < P; ++k) {
        const double h = at[3 * k], x0 = at[3 * k + 1];
        double shape, jx, jg;
        if (DHO) {
          const double xi = x + origin, xi0 = x0 + origin;
          const double a = (xi0 - xi) * (xi0 + xi);
          const double twice = g2[k] * xi;
          const double b = twice * twice;
          const double inverse = 1.0 / (a * a + b);
          shape = b * inverse;
          const double u = ahead[k] * shape * inverse * a;
          jx = -(u * xi0);
          jg = u * a * scale_g[k];
        } else {
          const double d = x - x0;
          const double inverse = 1.0 / (d * d + g2[k]);
          shape = g2[k] * inverse;
          const double u = ahead[k] * shape * inverse;
          jx = u * d;
          jg = jx * d * scale_g[k];
        }
        model = k == 0 ? h * shape : model + h * shape;
        row[3 * k] = shape;
        row[3 * k + 1] = jx;
        row[3 * k + 2] = jg;
      }
      model = model + at[C];
      row[C] = 1.0;
      if (LINEAR) {
        const double t = x - middle;
        model = model + at[C + 1] * t;
        row[C + 1] = t;
      }
      row[NP] = z - model;
      const bool inside = i < n;
#pragma unroll
      for (int k = 0; k <= NP; ++k) tile[lane * kStride + k] = inside ? row[k] : 0.0;
      tile_fence();
      const int64_t left = n - first;
      const int steps = left >= kLanes ? kLanes / 4 : (int)((left + 3) >> 2);
#pragma unroll
      for (int s = 0; s < kLanes / 4; ++s) {
        if (s < steps) {
          const double v = tile[(4 * s + quad) * kStride + l15];
          gram = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v, gram, 0, 0, 0);
        }
      }
      tile_fence();
    };
#pragma unroll
    for (int j = 0; j < kRegBins; ++j)
      if ((int64_t)kLanes * j < n) chunk(zreg[j], (int64_t)kLanes * j);
    for (int64_t first = kCapacity; first < n; first += kLanes) {
      const int64_t i = first + lane;
      chunk(i < n ? y[i] / top : 0.0, first);
    }
  };
  // S = (A^T A)[NP][NP]: register NP / 4 of lane (l15 = NP, quad = NP % 4)
  auto rss = [&](const f64x4 &gram) { return read_lane(gram[NP >> 2], (NP & 3) * 16 + NP); };

  f64x4 gram, trial_gram;
  evaluate(p, gram);
  double S = rss(gram);
  double damping = 1e-3;
  int state = 1, count = 0;
  double x[NP], pivot[NP];
  while (count < max_iterations) {
    ++count;
    solve<NP>(gram, damping, lane, x, pivot);
    double delta[NP];
    bool finite = true;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      delta[i] = read_lane(x[i], NP);
      finite = finite && std::isfinite(delta[i]);
    }
    double tallest = p[0];
#pragma unroll
    for (int k = 1; k < P; ++k) tallest = p[3 * k] > tallest ? p[3 * k] : tallest;
    bool small = finite && fabs(delta[C]) / tallest <= kStepTolerance;
    if (LINEAR) small = small && fabs(delta[C + 1]) * nd / tallest <= kStepTolerance;
    double trial[NP];
    bool valid = finite;
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const double h = p[3 * k], g = p[3 * k + 2];
      small = small && fabs(delta[3 * k]) / h <= kStepTolerance && fabs(delta[3 * k + 1]) / g <= kStepTolerance &&
              fabs(delta[3 * k + 2]) / g <= kStepTolerance;
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) trial[i] = p[i] + delta[i];
#pragma unroll
    for (int k = 0; k < P; ++k)
      valid = valid && trial[3 * k] > 0.0 && trial[3 * k + 2] >= 0.125 && trial[3 * k + 2] <= 4.0 * nd &&
              trial[3 * k + 1] >= -nd && trial[3 * k + 1] <= 2.0 * nd;
    bool accepted = false;
    double trial_S = 0.0;
    if (valid) {
      evaluate(trial, trial_gram);
      trial_S = rss(trial_gram);
      accepted = trial_S <= S;
    }
    if (accepted) {
#pragma unroll
      for (int i = 0; i < NP; ++i) p[i] = trial[i];
      gram = trial_gram;
      S = trial_S;
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

  // the standard errors: the undamped N at the final parameters, its inverse's diagonal from the unit columns
  solve<NP>(gram, 0.0, lane, x, pivot);
  bool curved = true;
  double error[NP];
  const double variance = S / (double)(n - NP);
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    curved = curved && std::isfinite(pivot[i]) && pivot[i] > 0.0;
    error[i] = sqrt(variance * read_lane(x[i], 16 + i));
  }
  double slot = NAN;  // lane k writes slot k of the outputs
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    slot = lane == i ? p[i] : slot;
    slot = lane == kSlots + i && curved ? error[i] : slot;
  }
  slot = lane == 28 ? S : slot;
  slot = lane == 29 ? top : slot;
  slot = lane == 30 ? total : slot;
  slot = lane == 31 && total != 0.0 ? moment / total : slot;
  if (lane < kOutputs) result[lane] = slot;
  if (lane == 0) {
    status[fit] = state;
    iterations[fit] = count;
  }
}

// ----------------------------------------------------------------------------- entries
using Kernel = void (*)(const double *, int64_t, const int64_t *, const int64_t *, const int64_t *, const double *,
                        const double *, const double *, int64_t, int, double *, int32_t *, int32_t *);

template <int P>
Kernel kernel_of(bool linear, bool dho) {
  if (linear) return dho ? peakfit_kernel<P, true, true> : peakfit_kernel<P, true, false>;
  return dho ? peakfit_kernel<P, false, true> : peakfit_kernel<P, false, false>;
}

Kernel kernel_of(int P, bool linear, bool dho) {
  switch (P) {
    case 1: return kernel_of<1>(linear, dho);
    case 2: return kernel_of<2>(linear, dho);
    case 3: return kernel_of<3>(linear, dho);
    default: return kernel_of<4>(linear, dho);
  }
}

using rn_fit::FitArgs;
using rn_spectrum::Fit;
thread_local rn_spectrum::ErrorText g_error;
rn_spectrum::DeviceBuffer g_real;  // origin [F], centres [F][P], widths [F][P]
rn_fit::FitWorkspace g_fits(kOutputs, {&g_real});

int peakfit_fit(int device, const FitArgs &a, int shape, int linear, int P, const double *origin, const double *centres,
                const double *widths) {
  if (int rc = rn_fit::check_sizes(a, g_error)) return rc;
  if (P < 1 || P > RN_PEAKFIT_MAX_PEAKS)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT, "P = %d peaks is outside 1 .. %d", P, RN_PEAKFIT_MAX_PEAKS);
  if (shape != RN_PEAKFIT_LORENTZIAN && shape != RN_PEAKFIT_DHO)
    return g_error.fail(RN_ERR_INVALID_ARGUMENT, "shape = %d is neither RN_PEAKFIT_LORENTZIAN nor RN_PEAKFIT_DHO", shape);
  if (linear != 0 && linear != 1) return g_error.fail(RN_ERR_INVALID_ARGUMENT, "linear = %d is neither 0 nor 1", linear);
  if (a.F == 0) return RN_OK;
  if (a.any_null() || !origin || !centres || !widths) return g_error.fail(RN_ERR_INVALID_ARGUMENT, "a null pointer");
  const int parameters = 3 * P + 1 + linear;
  for (int64_t f = 0; f < a.F; ++f) {
    if (int rc = rn_fit::check_row(a, f, g_error)) return rc;
    if (a.num_bins[f] < parameters + 2)
      return g_error.fail(RN_ERR_INVALID_ARGUMENT, "fit %lld: %lld bins, a fit of %d parameters needs at least p + 2 = %d",
                          (long long)f, (long long)a.num_bins[f], parameters, parameters + 2);
    if (int rc = rn_fit::check_window(a, f, g_error)) return rc;
    if (!std::isfinite(origin[f]))
      return g_error.fail(RN_ERR_INVALID_ARGUMENT, "fit %lld: the origin is not finite", (long long)f);
    if (shape == RN_PEAKFIT_DHO && !(origin[f] > 0.0))
      return g_error.fail(RN_ERR_INVALID_ARGUMENT, "fit %lld: origin %g is not positive, as RN_PEAKFIT_DHO needs",
                          (long long)f, origin[f]);
    for (int k = 0; k < P; ++k) {
      const double centre = centres[f * P + k], width = widths[f * P + k];
      if (!(centre >= 0.0 && centre <= (double)(a.num_bins[f] - 1)))  // (not so for NaN)
        return g_error.fail(RN_ERR_INVALID_ARGUMENT, "fit %lld: centre %d = %g is outside [0, %lld]", (long long)f, k,
                            centre, (long long)(a.num_bins[f] - 1));
      if (!std::isfinite(width) || !(width > 0.0))
        return g_error.fail(RN_ERR_INVALID_ARGUMENT, "fit %lld: width %d = %g is not positive and finite", (long long)f, k,
                            width);
    }
  }
  if (int rc = rn_spectrum::select_device(device, g_error)) return rc;

  std::lock_guard<std::mutex> lock(g_fits.mutex);
  g_fits.bind(device);
  const size_t count = (size_t)a.F;
  if (g_fits.ensure(a) != RN_OK || g_real.ensure((1 + 2 * (size_t)P) * count * sizeof(double), Fit::kGrowOnly) != RN_OK)
    return g_fits.no_memory(a, g_error);
  double *d_origin = g_real.as<double>(), *d_centres = d_origin + count, *d_widths = d_centres + (size_t)P * count;
  rn_spectrum::FirstError ok;
  const double *d_rows = g_fits.stage(a, ok);
  ok(hipMemcpyAsync(d_origin, origin, count * sizeof(double), hipMemcpyHostToDevice, a.stream));
  ok(hipMemcpyAsync(d_centres, centres, (size_t)P * count * sizeof(double), hipMemcpyHostToDevice, a.stream));
  ok(hipMemcpyAsync(d_widths, widths, (size_t)P * count * sizeof(double), hipMemcpyHostToDevice, a.stream));
  if (ok.first == hipSuccess) {
    kernel_of(P, linear != 0, shape == RN_PEAKFIT_DHO)<<<rn_fit::fit_blocks(a.F, kWaves), kWaves * kLanes, 0, a.stream>>>(
        d_rows, a.bins, g_fits.column(a, 0), g_fits.column(a, 1), g_fits.column(a, 2), d_origin, d_centres, d_widths, a.F,
        a.max_iterations, g_fits.d_out(), g_fits.d_status(), g_fits.d_iterations(a));
    ok(hipGetLastError());
  }
  return g_fits.finish(a, ok, g_error);
}

}  // namespace

extern "C" int rn_peakfit_fit(int device, const double *rows, int64_t num_rows, int64_t bins, const int64_t *row_index,
                              const int64_t *first_bin, const int64_t *num_bins, int64_t F, int shape, int linear, int P,
                              const double *origin, const double *centres, const double *widths, int max_iterations,
                              double *out, int32_t *status, int32_t *iterations) {
  return peakfit_fit(device, {rows, true, num_rows, bins, row_index, first_bin, num_bins, F, max_iterations, out, status,
                              iterations, nullptr}, shape, linear, P, origin, centres, widths);
}

extern "C" int rn_peakfit_fit_device(int device, const double *d_rows, int64_t num_rows, int64_t bins,
                                     const int64_t *row_index, const int64_t *first_bin, const int64_t *num_bins,
                                     int64_t F, int shape, int linear, int P, const double *origin, const double *centres,
                                     const double *widths, int max_iterations, double *out, int32_t *status,
                                     int32_t *iterations, void *stream) {
  return peakfit_fit(device, {d_rows, false, num_rows, bins, row_index, first_bin, num_bins, F, max_iterations, out, status,
                              iterations, static_cast<hipStream_t>(stream)}, shape, linear, P, origin, centres, widths);
}

extern "C" int rn_peakfit_window_capacity(void) { return kCapacity; }

extern "C" const char *rn_peakfit_last_error(void) { return g_error.text.c_str(); }
