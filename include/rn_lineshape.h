/* C ABI of the Lorentzian line-shape fits on gfx950 (librn_potgnn.so; kernel: csrc/lineshape.hip).
 *
 * A fit is (row, first bin b0, bin count n) of rows [num_rows][bins].  It works in bin units, x = 0 .. n-1 from b0, on
 * the normalised values z = y / max(y in the window), with the model m(x) = h g^2 / ((x - x0)^2 + g^2) + c, all
 * float64.  The recipe (start values, Levenberg-Marquardt with one elimination order, the validity box, the stop
 * rules) is stated in ramannoodle_amd/lineshape.py, whose fit_lorentzians_host is the definition the kernel is tested
 * against; the kernel differs from it by the order of the sums over the bins and by fused multiply-adds only.
 *
 * Per fit, out[RN_LINESHAPE_OUTPUTS] = (h, x0, g, c, S, max, sum z, sum x z / sum z): the parameters in bin units and
 * normalised values, the residual sum of squares S, the window's maximum and its two moments.  status: 0 converged,
 * 1 stopped at max_iterations, 2 a degenerate window (a non-finite value, max <= 0 or max == min: every output NaN,
 * iterations 0), 3 no acceptable step (the damping passed 1e12).  iterations: the number of solves.
 *
 * Conventions (those of rn_potgnn.h): every function returns RN_OK (0) or a negative rn_status of rn_potgnn.h; the
 * text of the calling thread's last error is what the last_error entry returns.  Arguments are validated before
 * the device is touched: RN_ERR_INVALID_ARGUMENT for a null pointer, num_rows < 1, bins < 1, F < 0,
 * max_iterations < 1, a row index outside [0, num_rows), a bin range outside [0, bins) or num_bins <
 * RN_LINESHAPE_MIN_BINS.  F = 0 is RN_OK.  No atomics are used and the order of every sum depends on n alone: a
 * fit's result does not depend on F, on its place in the table or on the other fits, and repeated calls give the same
 * bits.  Calls are serialised by one lock (they share a device workspace, which grows to the largest call).
 */
#ifndef RN_LINESHAPE_H
#define RN_LINESHAPE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: this is what it exports */

#define RN_LINESHAPE_OUTPUTS 8
#define RN_LINESHAPE_MIN_BINS 5

/* rows host float64 [num_rows][bins]; row_index / first_bin / num_bins host int64 [F]; out host float64
 * [F][RN_LINESHAPE_OUTPUTS]; status / iterations host int32 [F].  Returns when the results are in the host arrays. */
int rn_lineshape_fit(int device, const double *rows, int64_t num_rows, int64_t bins, const int64_t *row_index,
                     const int64_t *first_bin, const int64_t *num_bins, int64_t F, int max_iterations, double *out,
                     int32_t *status, int32_t *iterations);
/* The same with rows in HBM on `device`, written by work on `stream` (a hipStream_t; null: the default stream): the
 * fits are enqueued on `stream`, behind that work.  The table and the results stay host arrays; returns when the
 * results are in them. */
int rn_lineshape_fit_device(int device, const double *d_rows, int64_t num_rows, int64_t bins, const int64_t *row_index,
                            const int64_t *first_bin, const int64_t *num_bins, int64_t F, int max_iterations,
                            double *out, int32_t *status, int32_t *iterations, void *stream);
/* The longest window, in bins, that a wave keeps in registers between iterations; the bins of a longer one past this
 * number are read again from memory in every iteration (the same arithmetic, the same order of the sums). */
int rn_lineshape_window_capacity(void);
const char *rn_lineshape_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
