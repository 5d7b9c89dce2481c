/* C ABI of harmonic trajectories on gfx950: the positions of atoms that move along harmonic modes with given amplitudes
 * and phases, synthesised on the GPU (librn_potgnn.so; kernel: csrc/kernels_harmonic.hip, entries:
 * csrc/spectrum_harmonic.hip).
 *
 * Definition (ramannoodle_amd/harmonic.py, synthesize_host, is the statement the kernel is tested against).  All
 * float64.  ref[j]: fractional reference positions, K = 3N columns, j = 3 i + r.  D[m][j]: the fractional displacement
 * of a unit mass-weighted amplitude of mode m, M modes.  omega_dt[m]: the angular frequency of mode m times the
 * timestep, in rad.  Per run r < R: amp[r][m] (amu^1/2 Angstrom) and phase[r][m] (rad).  t0 >= 0: the absolute index of
 * the first frame of the call; T frames.
 *   theta[r][t][m] = omega_dt[m] * (double)(t0 + t) + phase[r][m]      (one rounded product, then one rounded sum: no fma)
 *   y[r][t][j]     = ref[j] + sum_m amp[r][m] * cos(theta[r][t][m]) * D[m][j]
 *   out[r][t][j]   = y - floor(y)
 * The kernel forms theta with exactly these two roundings, takes the accurate library cosine of it and sums over m on
 * the float64 matrix pipe, in ascending groups of four modes from zero: an order that depends on M alone.  The left
 * operand amp cos(theta) is made in registers and never exists in memory.  No atomics: repeated calls give the same
 * bits, so do the two entries, and a frame's values depend on its absolute index t0 + t alone, so a run may be
 * synthesised in pieces.
 *
 * Conventions (those of rn_quasiharmonic.h): every function returns RN_OK (0) or a negative rn_status of rn_potgnn.h;
 * the text of the calling thread's last error is what rn_ht_last_error returns.  Arguments are validated before the
 * device is touched: RN_ERR_INVALID_ARGUMENT for a null pointer, N, M, R or T < 1, t0 < 0 or t0 + T > 2^53 (the frame
 * index must be exact in a double), a non-finite value in ref, D, omega_dt, amp or phase (the text names the array and
 * the index), or a call of more than 2^31 - 1 workgroups (64 frames x 128 columns each).  Calls are serialised by one
 * lock: they share the device copies of the inputs, which grow to the largest call.
 */
#ifndef RN_HARMONIC_H
#define RN_HARMONIC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: this is what it exports */

/* ref host float64 [3N]; D host float64 [M][3N]; omega_dt host float64 [M]; amp, phase host float64 [R][M]; out host
 * float64 [R][T][3N].  Returns when out is filled. */
int rn_ht_synthesize(int device, const double *ref, const double *D, const double *omega_dt, const double *amp,
                     const double *phase, int32_t N, int32_t M, int32_t R, int64_t T, int64_t t0, double *out);
/* The same with the result left in HBM: d_out float64 [R][T][3N] on `device`.  The inputs are host arrays and are staged
 * before the call returns (they may be reused at once); the kernel is ordered on `stream` (a hipStream_t; null: the
 * default stream) and nothing is copied back: work that reads d_out is ordered after it on that stream. */
int rn_ht_synthesize_device(int device, const double *ref, const double *D, const double *omega_dt, const double *amp,
                            const double *phase, int32_t N, int32_t M, int32_t R, int64_t T, int64_t t0, double *d_out,
                            void *stream);
/* Profiling, off by default: while it is on, every call also takes the HIP-event times of its three phases (the device
 * entry then waits for its kernel), and rn_ht_phase_times returns those of the most recent call in millis[3], in
 * milliseconds: the copies of the inputs to the device, the kernel, the copy of out to the host (0 for the device
 * entry). */
int rn_ht_set_profiling(int enabled);
int rn_ht_phase_times(double *millis);
const char *rn_ht_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
