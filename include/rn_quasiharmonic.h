/* C ABI of the covariance moments of quasi-harmonic mode analysis on gfx950 (librn_potgnn.so; kernels:
 * csrc/kernels_covariance.hip, entries: csrc/spectrum_covariance.hip).
 *
 * Definition (ramannoodle_amd/quasiharmonic.py, moments_host, is the statement the kernels are tested against).  All
 * float64.  x[t][j]: wrapped fractional positions of frames t = 0..T-1, K = 3N columns, j = 3 i + r.  a[j]: an anchor
 * structure.  bounds[0..B]: strictly ascending, bounds[0] = 0, bounds[B] = T; block b holds frames bounds[b] ..
 * bounds[b+1]-1.  joined[b] in {0, 1}: 1 when the step out of the block's last frame exists and belongs to block b, 0
 * when it does not exist (a run boundary, the end of the data); joined[B-1] = 0.
 *   displacement  w_t = x_t - a;          w_t -= rint(w_t)      (the minimum image, round to nearest even)
 *   step          s_t = x_{t+1} - x_t;    s_t -= rint(s_t)      for every frame of a block but its last when joined = 0
 *   first[b][j]         = sum_t w_t[j]
 *   second[b][0][j][l]  = sum_t w_t[j] w_t[l]
 *   second[b][1][j][l]  = sum_t s_t[j] s_t[l]
 *   counts[b]           = (frames, steps)
 * Plain fractional coordinates: no masses, no lattice.  Both matrices of a block are full [K][K] and symmetric bit for
 * bit.  A block of one frame with joined = 0 is legal and has a zero step moment.
 *
 * Sums.  The frames of a block are cut into chunks of rn_qh_chunk_frames() frames (the last one shorter); a chunk's
 * partial sums run over its frames in ascending order on the matrix pipe, and a second kernel adds the chunks of a
 * block in ascending order.  No atomics: the order of every sum depends on (T, bounds) alone, repeated calls give the
 * same bits, and so do the two entries.
 *
 * Conventions (those of rn_lineshape.h): every function returns RN_OK (0) or a negative rn_status of rn_potgnn.h; the
 * text of the calling thread's last error is what rn_qh_last_error returns.  Arguments are validated before the device
 * is touched: RN_ERR_INVALID_ARGUMENT for a null pointer, N < 1, T < 1, B < 1, bounds that are not strictly ascending
 * from 0 to T, a joined value outside {0, 1} or joined[B-1] != 0.  Calls are serialised by one lock (they share a device
 * workspace, which grows to the largest call: 64 KiB per chunk and pair of 64-column tiles, and the results).
 */
#ifndef RN_QUASIHARMONIC_H
#define RN_QUASIHARMONIC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: this is what it exports */

/* pos host float64 [T][3N]; anchor host float64 [3N]; bounds host int64 [B+1]; joined host int32 [B]; first host
 * float64 [B][3N]; second host float64 [B][2][3N][3N]; counts host int64 [B][2].  Returns when the results are in the
 * host arrays. */
int rn_qh_moments(int device, const double *pos, int64_t T, int32_t N, const double *anchor, const int64_t *bounds,
                  const int32_t *joined, int64_t B, double *first, double *second, int64_t *counts);
/* The same with pos in HBM on `device`, written by work on `stream` (a hipStream_t; null: the default stream): the
 * positions are read in place, after that work.  Everything else stays a host array; returns when the results are in
 * them. */
int rn_qh_moments_device(int device, const double *d_pos, int64_t T, int32_t N, const double *anchor,
                         const int64_t *bounds, const int32_t *joined, int64_t B, double *first, double *second,
                         int64_t *counts, void *stream);
/* The number of frames of a chunk (see "Sums" above). */
int rn_qh_chunk_frames(void);
/* Profiling, off by default: while it is on, every call also takes the HIP-event times of its four phases, and
 * rn_qh_phase_times returns those of the most recent call in millis[4], in milliseconds: the copies to the device (the
 * positions of the host entry, the anchor, the chunk table), the rank updates, the sums over the chunks, the copies of
 * first and second to the host. */
int rn_qh_set_profiling(int enabled);
int rn_qh_phase_times(double *millis);
const char *rn_qh_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
