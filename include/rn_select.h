/* C ABI of the nearest-reference distance and the farthest-point selection on gfx950 (librn_potgnn.so; kernels:
 * csrc/kernels_select.hip, entries: csrc/select.hip).
 *
 * Definition (ramannoodle_amd/selection.py, nearest_host and select_farthest_host, is the statement the kernels are
 * tested against).  All float64.  X[S][D]: the rows to judge; R[M][D]: the reference rows; center[D], scale[D]: optional
 * (null: zeros, ones), applied while the operands are loaded and never written to memory.
 *   d2(a, b)     = sum_c ((a_c - b_c) scale_c)^2                       (center cancels)
 *   nearest:       index[s] = argmin_j d2(X_s, R_j), the lowest j among equal values; dist2[s] = d2(X_s, R_index[s]).
 *                  With exclude_self row s ignores j = s (for X == R: the leave-one-out neighbour).  A row without any
 *                  candidate (M = 1 with exclude_self) gets index -1 and dist2 = +inf.
 *   farthest:      mind[s] = dist2[s] of `nearest` (no exclude_self) when M > 0, +inf when M = 0.  Pick k = 0..count-1:
 *                  p_k = argmax_s mind[s] over the rows not picked yet, the lowest s among equal values; dist2[k] =
 *                  mind[p_k]; then mind[s] = min(mind[s], d2(X_s, X_p_k)).  When M = 0 the first pick is `first`, or,
 *                  with first < 0, the row farthest (in d2) from the column mean of X, the lowest s among equal values;
 *                  its dist2[0] is +inf.  `first` >= 0 with M > 0 is refused: the reference decides the first pick.
 *
 * How.  The search is a product on the float64 matrix pipe: with x' = (x - center) scale, the key |r'|^2 - 2 x'.r'
 * orders the rows of R as d2 does (|x'|^2 is the same for every j); tiles of rn_select_tile_rows() = 64 rows of X
 * against 64 rows of R, 16 columns at a time (any D >= 1: the remainder is zeros), with a running (key, index) per row
 * of X in the epilogue.  Equal keys resolve to the lowest index, and exact duplicates of a row of R have equal keys bit
 * for bit (every key is computed by the same operations in the same order, wherever its row lies).  Long references
 * are split across workgroups in ascending ranges of whole tiles; a second kernel merges the ranges in ascending
 * order, again with the lowest index on equal keys, and then recomputes the winner's d2 from differences: the
 * cancellation of the product form never reaches the caller.  No atomics.  The selection is one launch per pick with
 * no host synchronisation in between: every workgroup first reduces the (value, index) partials that the workgroups
 * of the launch before it left, then updates its rows and writes its own partial to the other of two buffers.  No
 * workgroup waits for another inside a kernel.
 *
 * Conventions (those of rn_lineshape.h): every function returns RN_OK (0) or a negative rn_status of rn_potgnn.h; the
 * text of the calling thread's last error is what rn_select_last_error returns.  Arguments are validated before the
 * device is touched: RN_ERR_INVALID_ARGUMENT for a null pointer, D < 1, S < 0, M < 0 (nearest: M < 1), count < 0 or
 * count > S, first >= S, first >= 0 with M > 0, S, M or D above 2^31 - 1, or a non-finite value of a host array (named
 * by its index).  S = 0 (and count = 0) is a no-op.  Calls are serialised by one lock (they share a device workspace,
 * which grows to the largest call).
 */
#ifndef RN_SELECT_H
#define RN_SELECT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: this is what it exports */

/* X host float64 [S][D]; R host float64 [M][D]; center, scale host float64 [D] or null; dist2 host float64 [S]; index
 * host int64 [S].  Returns when the results are in the host arrays. */
int rn_select_nearest(int device, const double *X, int64_t S, const double *R, int64_t M, int64_t D,
                      const double *center, const double *scale, int exclude_self, double *dist2, int64_t *index);
/* The same with X and R in HBM on `device`, written by work on `stream` (a hipStream_t; null: the default stream):
 * they are read in place, after that work, and not checked for non-finite values.  Everything else stays a host array. */
int rn_select_nearest_device(int device, const double *d_X, int64_t S, const double *d_R, int64_t M, int64_t D,
                             const double *center, const double *scale, int exclude_self, double *dist2,
                             int64_t *index, void *stream);
/* R may be null when M = 0.  first: a row of X, or negative for the default (see above).  picks host int64 [count];
 * dist2 host float64 [count]. */
int rn_select_farthest(int device, const double *X, int64_t S, int64_t D, const double *R, int64_t M,
                       const double *center, const double *scale, int64_t first, int64_t count, int64_t *picks,
                       double *dist2);
int rn_select_farthest_device(int device, const double *d_X, int64_t S, int64_t D, const double *d_R, int64_t M,
                              const double *center, const double *scale, int64_t first, int64_t count, int64_t *picks,
                              double *dist2, void *stream);
/* The rows of a tile of the search (of X and of R alike), and the number of ascending ranges a reference of M rows is
 * split into for S rows of X. */
int rn_select_tile_rows(void);
int64_t rn_select_reference_splits(int64_t S, int64_t M);
/* Profiling, off by default: while it is on, every call also takes the HIP-event times of its four phases, and
 * rn_select_phase_times returns those of the most recent call in millis[4], in milliseconds: the copies to the device,
 * the nearest search (norms, tiles, merge), the picks, the copies to the host. */
int rn_select_set_profiling(int enabled);
int rn_select_phase_times(double *millis);
const char *rn_select_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
