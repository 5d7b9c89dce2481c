/* C ABI of the multi-peak line-shape fits on gfx950 (librn_potgnn.so; kernel: csrc/peakfit.hip).
 *
 * A fit is (row, first bin b0, bin count n, origin o, P start centres, P start widths) of rows [num_rows][bins], P in
 * 1 .. RN_PEAKFIT_MAX_PEAKS.  It works in bin units, x = 0 .. n-1 from b0, on the normalised values
 * z = y / max(y in the window), all float64, with the parameters (h_1, x0_1, g_1, .., h_P, x0_P, g_P, c[, s]) and the
 * model m(x) = sum_k h_k l_k(x) + c + s (x - (n - 1) / 2).  shape RN_PEAKFIT_LORENTZIAN: l = g^2 / ((x - x0)^2 + g^2).
 * shape RN_PEAKFIT_DHO, the velocity power spectrum of a damped oscillator: l = b / (a^2 + b) with xi = x + o,
 * xi0 = x0 + o, a = xi0^2 - xi^2, b = (2 g xi)^2; o is the window's first bin on the absolute axis, in bins.  linear = 0
 * leaves s out: p = 3 P + 1 + linear parameters.  The recipe (start values, Levenberg-Marquardt with one elimination
 * order, the validity box, the stop rules, the standard errors from the curvature) is stated in
 * ramannoodle_amd/peakfit.py, whose fit_peaks_host is the definition the kernel is tested against; the kernel differs
 * from it by the order of the sums over the bins and by fused multiply-adds only.
 *
 * Per fit, out[RN_PEAKFIT_OUTPUTS]: the parameters in slots 0 .. p-1, their standard errors in slots 14 .. 14+p-1 (all
 * NaN when the curvature matrix has a pivot <= 0), the residual sum of squares S, the window's maximum, sum z and
 * sum x z / sum z in slots 28 .. 31; unused slots are NaN.  status: 0 converged, 1 stopped at max_iterations, 2 a
 * degenerate window (a non-finite value, max <= 0 or max == min: every output NaN, iterations 0), 3 no acceptable step
 * (the damping passed 1e12).  iterations: the number of solves.
 *
 * Conventions (those of rn_lineshape.h): every function returns RN_OK (0) or a negative rn_status of rn_potgnn.h; the
 * text of the calling thread's last error is what the last_error entry returns.  Arguments are validated before the
 * device is touched: RN_ERR_INVALID_ARGUMENT for what rn_lineshape_fit refuses and for P outside 1 .. 4, an unknown
 * shape, linear outside {0, 1}, num_bins < p + 2, a centre outside [0, n-1], a width or an origin that is not finite,
 * a width <= 0 and, for RN_PEAKFIT_DHO, an origin <= 0.  F = 0 is RN_OK.  No atomics are used and the order of every
 * sum depends on n alone: a fit's result does not depend on F, on its place in the table or on the other fits, and
 * repeated calls give the same bits.  Calls are serialised by one lock (they share a device workspace, which grows to
 * the largest call).
 */
#ifndef RN_PEAKFIT_H
#define RN_PEAKFIT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: this is what it exports */

#define RN_PEAKFIT_OUTPUTS 32
#define RN_PEAKFIT_MAX_PEAKS 4
#define RN_PEAKFIT_LORENTZIAN 0
#define RN_PEAKFIT_DHO 1

/* rows host float64 [num_rows][bins]; row_index / first_bin / num_bins host int64 [F]; origin host float64 [F];
 * centres / widths host float64 [F][P], in bins from b0; out host float64 [F][RN_PEAKFIT_OUTPUTS]; status / iterations
 * host int32 [F].  Returns when the results are in the host arrays. */
int rn_peakfit_fit(int device, const double *rows, int64_t num_rows, int64_t bins, const int64_t *row_index,
                   const int64_t *first_bin, const int64_t *num_bins, int64_t F, int shape, int linear, int P,
                   const double *origin, const double *centres, const double *widths, int max_iterations, double *out,
                   int32_t *status, int32_t *iterations);
/* The same with rows in HBM on `device`, written by work on `stream` (a hipStream_t; null: the default stream): the
 * fits are enqueued on `stream`, behind that work.  The table and the results stay host arrays; returns when the
 * results are in them. */
int rn_peakfit_fit_device(int device, const double *d_rows, int64_t num_rows, int64_t bins, const int64_t *row_index,
                          const int64_t *first_bin, const int64_t *num_bins, int64_t F, int shape, int linear, int P,
                          const double *origin, const double *centres, const double *widths, int max_iterations,
                          double *out, int32_t *status, int32_t *iterations, void *stream);
/* The longest window, in bins, that a wave keeps in registers between iterations; the bins of a longer one past this
 * number are read again from memory in every iteration (the same arithmetic, the same order of the sums). */
int rn_peakfit_window_capacity(void);
const char *rn_peakfit_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
