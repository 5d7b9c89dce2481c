/* C ABI of the interpolation polarizability model on gfx950 (librn_potgnn.so; kernels: csrc/kernels_interp.hip).
 *
 * The model (ramannoodle's InterpolationModel / ARTModel, finished: building one is the reference's job):
 *   alpha(x) = alpha_ref + sum_j (1 - mask_j) s_j(a_j),   a_j = sum_{i,r} w[i][r] F[j][3i+r],
 *   w the wrapped fractional displacement from the reference positions (d = x - x_ref, m = d - floor(d),
 *   w = m > 0.5 ? m - 1 : m), F[j][3i+r] = sum_s L[r][s] b_j[i][s], and s_j a piecewise polynomial with 3x3 values
 *   given as Taylor tables: DOF j has P_j = piece_offsets[j+1] - piece_offsets[j] pieces, its P_j + 1 breakpoints
 *   x_0 < .. < x_P start at breakpoints[piece_offsets[j] + j], and the coefficients of its piece p,
 *   c[q][9] = s^(q)(x_p) / q! for q = 0 .. orders[j], follow each other in `coefficients`, DOF after DOF, piece after
 *   piece (a DOF of order k takes P_j (k + 1) 9 doubles).  The piece of an amplitude a is
 *   p = #{i in 1..P-1 : x_i <= a}: the end pieces extend beyond the knots.  Everything is float64.
 *
 * Conventions (those of rn_potgnn.h): every function returns RN_OK (0) or a negative rn_status of rn_potgnn.h;
 * rn_interp_last_error() has the text.  Arguments are validated before any device work.  Calls on one handle are
 * serialised by the handle's lock; distinct handles are independent.  The *_device entries take device pointers on the
 * handle's device, enqueue on `stream` (a hipStream_t; null: the default stream) and return without waiting for the
 * kernels, except where they say otherwise; successive calls on one handle share its workspaces, so calls on different
 * streams must be ordered by the caller.  Repeated calls give the same bits, and so does any chunking.
 * workspace_limit (bytes; 0: 1 GiB) bounds the workspace of a chunk of frames: the scaled spline derivatives
 * [frames][6][J], the Jacobian rows [frames + 1][6][N][3] and, for the mode entry, the two mode arrays.  When not even
 * one step fits, the entry returns RN_ERR_OUT_OF_MEMORY.
 */
#ifndef RN_INTERP_H
#define RN_INTERP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: this is what it exports */

typedef struct rn_interp rn_interp;

#define RN_INTERP_MAX_ORDER 5

/* lattice [9] (rows = lattice vectors), ref_positions [N][3] fractional, alpha_ref [9], basis_cart [J][N][3], the tables as
 * above.  RN_ERR_INVALID_ARGUMENT: a null pointer, N < 1, J < 1, an order outside 1..RN_INTERP_MAX_ORDER, piece offsets
 * that do not start at 0 or leave a DOF without a piece, breakpoints that do not ascend, or a non-finite entry anywhere.
 * The tables are uploaded once, padded to the model's highest order with zero leading coefficients. */
int rn_interp_create(int32_t N, const double *lattice, const double *ref_positions, const double *alpha_ref, int32_t J,
                     const double *basis_cart, const int32_t *piece_offsets, const double *breakpoints,
                     const int32_t *orders, const double *coefficients, int device, rn_interp **handle);
void rn_interp_destroy(rn_interp *h);
const char *rn_interp_last_error(const rn_interp *h);

/* mask host uint8 [J]: non-zero = the DOF is left out.  Waits for the handle's earlier work. */
int rn_interp_set_mask(rn_interp *h, const uint8_t *mask);
/* 1 when every table is symmetric (|c[3r+s] - c[3s+r]| <= 1e-12 of the largest |c|), else 0; negative: a status.  The
 * entries that use the Jacobian (its six components) need it and return RN_ERR_INVALID_ARGUMENT otherwise. */
int rn_interp_is_symmetric(const rn_interp *h);

/* Host in, host out: positions [S][N][3] -> alpha [S][9].  S = 0 is RN_OK. */
int rn_interp_calc_polarizabilities(rn_interp *h, const double *positions, int64_t S, double *alpha);
/* Device in, device out, S >= 1. */
int rn_interp_forward_device(rn_interp *h, const double *d_positions, int64_t S, double *d_alpha, void *stream);
/* d vec6_c / d x of every frame: d_jac [S][6][N][3], c = (xx, yy, zz, xy, xz, yz), S >= 1. */
int rn_interp_jacobian_device(rn_interp *h, const double *d_positions, int64_t S, double *d_jac, void *stream);

/* Trapezoid increments per atom group, d_out [S-1][G][9] (rn_potgnn_group_increments_device with sigma = 1): labels
 * host int32 [N] in [0, G), every group used, 1 <= G <= 16, S >= 2. */
int rn_interp_group_increments_device(rn_interp *h, const double *d_positions, int64_t S, const int32_t *labels, int G,
                                      size_t workspace_limit, double *d_out, void *stream);
/* Trapezoid increments per phonon mode, d_out [S-1][M + rest][9] (rn_potgnn_mode_increments_device with sigma = 1):
 * disp / proj host [M][N][3], finite, M >= 1, rest 0 or 1, S >= 2. */
int rn_interp_mode_increments_device(rn_interp *h, const double *d_positions, int64_t S, const double *disp,
                                     const double *proj, int32_t M, int rest, size_t workspace_limit, double *d_out,
                                     void *stream);
/* Raman tensors split by atom group, host: raman [M][G][9] = 2 sum_{i in g} J_i(ref_positions) . d_{m,i}.  M = 0 is RN_OK. */
int rn_interp_partial_raman_tensors(rn_interp *h, const double *ref_positions, const double *displacements, int64_t M,
                                    const int32_t *labels, int G, double *raman);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
