/*
 * rn_potgnn.h -- C ABI of the MI355X (gfx950) PotGNN polarizability evaluator.
 *
 * This is the drop-in boundary for ONE path of wolearyc/ramannoodle: batched evaluation
 * of the PotGNN polarizability model.  The reference has no FFI of its own (it is pure
 * Python); each entry point below names the reference interface it replaces
 * (paths relative to the reference repository root).
 *
 * Conventions
 *   - plain C, no torch types; all pointers are caller-owned unless stated otherwise.
 *   - every function returns RN_OK (0) or a negative rn_status; rn_potgnn_last_error()
 *     gives a human-readable message for the most recent failure on that handle
 *     (or the most recent rn_potgnn_create failure when the handle is NULL).
 *   - Threading: a handle owns mutable state (device workspaces, streams, the forward tape, the
 *     last error string), so it is NOT re-entrant; every entry point that takes a handle holds the
 *     handle's own lock for the duration of the call, i.e. calls on ONE handle from several threads
 *     are serialised by the library, and calls on DISTINCT handles (also on one device) run
 *     concurrently.  The asynchronous pair rn_potgnn_calc_polarizabilities_async / rn_potgnn_wait
 *     keeps its ordering guarantees per handle.  rn_potgnn_last_error() returns a pointer into the
 *     handle: read it before the next call on that handle from another thread.  The reference's
 *     PolarizabilityModel is single-threaded and synchronous (abstract.py:10-29).
 *     The small getters / setters (config_flags, kernel_times, set_profiling, train_row_count, set_stat_reducer) and the
 *     argument checks that read handle state take the same lock.
 *   - no C++ exception crosses this boundary: every failure is a negative rn_status.
 *   - rn_potgnn_forward* / rn_potgnn_train_forward* evaluate in float32 (the *_f64 entries in float64).  A training
 *     forward's tape lives in the handle's workspace until its backward: an evaluation, Jacobian or another training forward
 *     on the same handle in between voids it, and the backward then fails with RN_ERR_INVALID_ARGUMENT.
 *   - the role-specialised EdgeBlock bounds its internal spin waits; a wait that runs out is reported as a launch failure
 *     by the first entry point that synchronises (evaluation with synchronize != 0, rn_potgnn_wait, the training entries,
 *     the Jacobian, rn_potgnn_adam_step), and the rows the affected workgroup stored are NaN, so an entry point that does
 *     not synchronise never hands back plausible numbers from such a launch.
 *   - "host" entry points take host buffers and include PCIe transfers;
 *     "device" entry points take device (HBM) pointers and a hipStream_t (as void*).
 */
#ifndef RN_POTGNN_H
#define RN_POTGNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: this is what it exports */

typedef enum rn_status {
  RN_OK = 0,
  RN_ERR_INVALID_ARGUMENT = -1, /* mapped to ValueError by the Python wrapper          */
  RN_ERR_UNSUPPORTED = -2,      /* e.g. embedding size > 128                            */
  RN_ERR_NO_DEVICE = -3,        /* no gfx950 device / HIP runtime failure at init       */
  RN_ERR_HIP = -4,              /* a HIP call failed; see rn_potgnn_last_error          */
  RN_ERR_OUT_OF_MEMORY = -5
} rn_status;

typedef struct rn_potgnn rn_potgnn; /* opaque */

/*
 * Model description handed to rn_potgnn_create.  Replaces the state that
 * PotGNN.__init__ builds (ramannoodle/pmodel/torch/_gnn.py:484-539).
 */
typedef struct rn_potgnn_config {
  int32_t num_atoms;            /* N                                                    */
  int32_t num_edges;            /* E  directed edges of the frozen reference graph      */
  int32_t num_atom_types;       /* K  rows of the Embedding (_gnn.py:503,509)           */
  int32_t size_node_embedding;  /* Fn (1..128)                                          */
  int32_t size_edge_embedding;  /* Fe (1..128)                                          */
  int32_t num_message_passes;   /* P                                                    */
  double gauss_coefficient;     /* -0.5/(mu1-mu0)^2 as the reference computed it
                                   (_gnn.py:64); the mu grid itself is the
                                   "_edge_embedding.offset" buffer inside `weights`     */
  int32_t max_chunk_structures; /* 0 = choose automatically; else structures per device
                                   work chunk (workspace is sized from it)              */
  int32_t device;               /* HIP device ordinal                                   */
} rn_potgnn_config;

/*
 * One-time neighbour search of the reference structure on the device; replaces the pair
 * test of _radius_graph_pbc (ramannoodle/pmodel/torch/_utils.py:118-137): float32
 * minimum-image distances, adjacency[a*N + b] = (dist <= cutoff && a != b) as host uint8.
 * Compacting the flags row-major gives the edge list sorted by (a, b).
 */
int rn_potgnn_radius_graph(const double *lattice, const double *positions, int32_t num_atoms,
                           double cutoff, int device, uint8_t *adjacency);

/* Number of floats rn_potgnn_create expects in `weights` for this configuration. */
size_t rn_potgnn_weight_count(const rn_potgnn_config *cfg);

/*
 * Create an evaluator.
 *   edge_a, edge_b  int32[E]  reference-graph edges (a -> b), sorted by (a, b), exactly
 *                             rows 1 and 2 of PotGNN._ref_edge_indexes
 *                             (_gnn.py:492-496, _utils.py:137).  The edge triplets
 *                             (_utils.py:153-168) are a pure function of this list and
 *                             are enumerated on the device; see
 *                             rn_potgnn_debug_triplets.
 *   atom_types      int32[N]  _atom_type_map[atomic_numbers] (_gnn.py:502-506,557)
 *   lattice         f64[3*3]  row-major, rows are lattice vectors (Angstrom)
 *   weights         f32[rn_potgnn_weight_count]  the floating-point entries of
 *                             PotGNN.state_dict() concatenated in state_dict order,
 *                             each tensor row-major in its native torch layout
 *                             (SURVEY.md section 8b lists the keys; the integer
 *                             "num_batches_tracked" entry is skipped)
 *   mean, stddev    f64[3*3]  _mean_polarizability / _stddev_polarizability
 */
int rn_potgnn_create(const rn_potgnn_config *cfg, const int32_t *edge_a,
                     const int32_t *edge_b, const int32_t *atom_types,
                     const double *lattice, const float *weights, size_t num_weights,
                     const double *mean, const double *stddev, rn_potgnn **out);

/* Releases device memory and streams owned by the handle.  NULL is allowed. */
void rn_potgnn_destroy(rn_potgnn *h);

/*
 * Replaces PotGNN.calc_polarizabilities (_gnn.py:667-721).
 *   positions  host f64[S*N*3]  fractional coordinates, C-contiguous, not modified
 *   alpha      host f64[S*3*3]  de-standardised symmetric tensors (alpha*sigma + mu)
 * S may be 0.  Includes H2D/D2H copies (pipelined: see rn_potgnn_calc_polarizabilities_to_device).
 */
int rn_potgnn_calc_polarizabilities(rn_potgnn *h, const double *positions, int64_t S,
                                    double *alpha);

/*
 * The same evaluation (float32 arithmetic, host float64 positions) with the result left on the device: d_alpha device
 * f64[S*9].  The positions are cast to float32 while they are staged into page-locked memory -- the reference casts them
 * before any arithmetic (_gnn.py:709), so the results are bit-identical to a float64 upload at half the PCIe bytes -- and
 * go through one work chunk at a time, cast / copy / kernels of consecutive chunks overlapped (rn_potgnn_calc_polarizabilities
 * does the same and then copies the result down).  Returns once everything is enqueued.  Ordering, with `stream` a
 * hipStream_t (NULL = the null stream):
 *   - work queued on `stream` before the call completes before d_alpha is written (an earlier reader of the same buffer:
 *     the previous all-gather on it, the last user of a recycled allocation);
 *   - `stream` is made to wait for the evaluation, so work the caller enqueues on it afterwards -- the all-gather of a
 *     sharded run, dynamics/_trajectory.py:71-90 across ranks -- sees the finished d_alpha;
 *   - a later call on the handle, through any entry point, needs no synchronisation in between: its float32 kernels queue
 *     behind this call's on the handle's streams, the float32 positions this call still reads sit in a device buffer of
 *     their own, and the weight updates of a training step (taped forward, rn_potgnn_adam_step) wait for this call.
 * `positions` may be reused on return.
 */
int rn_potgnn_calc_polarizabilities_to_device(rn_potgnn *h, const double *positions, int64_t S, double *d_alpha,
                                              void *stream);

/*
 * The same evaluation with every kernel instantiated for float64 -- what the reference computes
 * when torch's default dtype is float64 (calc_polarizabilities casts lattice and positions to
 * torch.get_default_dtype(), _gnn.py:705-710, and the modules were built in that dtype).  The
 * float32 master weights are widened exactly; geometry, projections, LayerNorms, gates and the
 * readout run in double.  Roughly 8x slower than the float32 path (no matrix cores, half the
 * frames per launch); meant for validation and for callers that need more than float32 carries.
 */
int rn_potgnn_calc_polarizabilities_f64(rn_potgnn *h, const double *positions, int64_t S,
                                        double *alpha);

/*
 * Pipelined host entry for streamed trajectories: the call enqueues the
 * host-to-device copy of `positions` on the handle's copy stream, the evaluation behind it and the
 * device-to-host copy of the result, and returns without waiting, so that the copy of block k+1
 * (and whatever the caller does meanwhile, e.g. parsing block k+2) overlaps the evaluation of
 * block k.  Two staging slots: a third call first waits for the first one.  `positions` must stay
 * untouched and `alpha` unread until rn_potgnn_wait returns; both should be page-locked
 * (rn_host_buffer_alloc) -- pageable memory works but makes the copies synchronous.
 */
int rn_potgnn_calc_polarizabilities_async(rn_potgnn *h, const double *positions, int64_t S,
                                          double *alpha);
/* Blocks until every rn_potgnn_calc_polarizabilities_async call issued so far has finished. */
int rn_potgnn_wait(rn_potgnn *h);

/* Page-locked host memory for the pipelined entry (hipHostMalloc / hipHostFree). */
int rn_host_buffer_alloc(size_t bytes, int device, void **out);
void rn_host_buffer_free(void *p);

/*
 * Same computation on device-resident buffers (what bench.py times):
 *   d_positions device f64[S*N*3];  d_alpha device f64[S*9] or NULL;
 *   d_vec6 device f32[S*6] or NULL -- standardised (xx,yy,zz,xy,xz,yz), i.e. the value
 *   of PotGNN.forward in eval mode (_gnn.py:617-665).
 * Work is enqueued on `stream` (a hipStream_t; NULL = the null stream) and, when
 * `synchronize` is non-zero, waited for before returning.
 */
int rn_potgnn_forward_device(rn_potgnn *h, const double *d_positions, int64_t S,
                             double *d_alpha, float *d_vec6, void *stream,
                             int synchronize);

/*
 * The device-resident entry with every kernel instantiated for float64 (see
 * rn_potgnn_calc_polarizabilities_f64): d_positions device f64[S*N*3] -> d_alpha device f64[S*9].
 * Used by the sharded phonon path, whose finite differences need float64 and whose results stay in
 * HBM until the all-gather.
 */
int rn_potgnn_forward_device_f64(rn_potgnn *h, const double *d_positions, int64_t S, double *d_alpha,
                                 void *stream, int synchronize);

/*
 * Variable-cell evaluation (an addition: the reference's calc_polarizabilities knows one fixed cell): the three entries
 * above with a lattice PER FRAME, for NPT runs, heating ramps and pressure scans.
 *   lattices / d_lattices  f64[S*9], row-major, rows = lattice vectors in Angstrom, not modified.
 * Frame s is evaluated in lattices[s] exactly as PotGNN.forward evaluates sample s in lattice[s] (_gnn.py:603-611: the
 * minimum-image fractional displacements are mapped to Cartesian with it; the graph topology stays the reference
 * structure's).  Float32 runs cast the lattices to float32 before any arithmetic, as forward casts its lattice argument;
 * use_float64 != 0 runs the kernels instantiated for double on the lattices as given.
 * A NULL lattices pointer is exactly the fixed-cell entry (rn_potgnn_calc_polarizabilities / _f64, _to_device,
 * rn_potgnn_forward_device / _f64), bit for bit.
 *
 * rn_potgnn_calc_polarizabilities_cells: host positions and lattices -> host alpha f64[S*9].  Float32: each piece's
 * lattices are cast into the page-locked piece that holds its float32 positions and copied with them (36 more bytes a
 * frame).
 * rn_potgnn_calc_polarizabilities_cells_to_device: host positions and lattices -> d_alpha device f64[S*9], float32
 * arithmetic, with every ordering guarantee of rn_potgnn_calc_polarizabilities_to_device; the float32 lattices this call
 * still reads sit in a device buffer of their own, next to the positions.  Both host arrays may be reused on return.
 * rn_potgnn_forward_cells_device: device positions and lattices -> d_alpha device f64[S*9]; `stream` and `synchronize`
 * as for rn_potgnn_forward_device.  d_lattices must stay untouched until the work has finished.
 *
 * The host entries check the lattices before any device work: a non-finite entry or a determinant of zero (within
 * rounding: |det| <= 1e-12 |a| |b| |c|) returns RN_ERR_INVALID_ARGUMENT and the message names the first offending frame.  The device entry cannot look at its
 * lattices without waiting for the device and does not: a non-finite lattice gives a non-finite alpha for that frame.
 */
int rn_potgnn_calc_polarizabilities_cells(rn_potgnn *h, const double *positions, const double *lattices, int64_t S,
                                          int use_float64, double *alpha);
int rn_potgnn_calc_polarizabilities_cells_to_device(rn_potgnn *h, const double *positions, const double *lattices,
                                                    int64_t S, double *d_alpha, void *stream);
int rn_potgnn_forward_cells_device(rn_potgnn *h, const double *d_positions, const double *d_lattices, int64_t S,
                                   int use_float64, double *d_alpha, void *stream, int synchronize);

/*
 * Structure descriptors (an addition): desc[s][c] = (1 / E) sum_e edge_P[s][e][c], the mean over a frame's edges of the
 * size_edge_embedding real columns of the edge embedding after the last message pass -- the rows the readout consumes,
 * read once more before it in whatever layout the run keeps them (float32, split-f16 pairs, the narrow pipeline's
 * destination order, float64), summed in float64 in an order that depends on the graph and the widths alone: a frame's
 * descriptor has the same bits whatever S, chunk or lane it was evaluated with.  desc is f64[S * size_edge_embedding].
 * One evaluation yields both outputs: with `alpha` (f64[S*9]) not NULL the polarizabilities of the same frames come
 * with it, bit for bit those of rn_potgnn_calc_polarizabilities / _cells (rn_potgnn_forward_cells_device).  lattices NULL:
 * the fixed cell; otherwise [S*9] as for the _cells entries, checked in the same way by the host entry.  S = 0 is a
 * no-op.  Without descriptors asked for, no entry launches the pooling kernel.
 * rn_potgnn_device_descriptors: everything in HBM; the work starts behind what `stream` holds at the call and `stream`
 * continues behind it (rn_potgnn_forward_device with synchronize = 0).  The pooling kernel touches the caller's pointers
 * one element at a time (d_desc[s * Fe + c], one thread each); tests/test_model_domain.py hands the entry views inside
 * guarded buffers.
 */
int rn_potgnn_descriptors(rn_potgnn *h, const double *positions, const double *lattices, int64_t S, int use_float64,
                          double *desc, double *alpha);
int rn_potgnn_device_descriptors(rn_potgnn *h, const double *d_positions, const double *d_lattices, int64_t S,
                                 int use_float64, double *d_desc, double *d_alpha, void *stream);

/*
 * Replaces PotGNN.forward for host callers (_gnn.py:617-665, eval mode):
 * host f64 positions -> host f32[S*6] standardised 6-vectors.
 */
int rn_potgnn_forward(rn_potgnn *h, const double *positions, int64_t S, float *vec6);

/*
 * PotGNN.forward(lattice[S,3,3], atomic_numbers, positions[S,N,3]) with a lattice PER SAMPLE
 * (_gnn.py:603-611: the minimum-image displacements of sample s are mapped to Cartesian with
 * lattice[s]; the graph topology stays the reference structure's): host f64 lattices[S*9]
 * (row-major, rows are lattice vectors), host f64 positions -> host f32[S*6], eval mode.
 */
int rn_potgnn_forward_lattices(rn_potgnn *h, const double *lattices, const double *positions,
                               int64_t S, float *vec6);

/*
 * PotGNN.forward(lattice[S,3,3], atomic_numbers[S,N], positions[S,N,3]) with BOTH per-sample
 * inputs (_gnn.py:617-665): `lattices` host f64[S*9] or NULL (the reference structure's lattice
 * for every sample); `atom_types` host int32[S*N] or NULL (the reference structure's species) --
 * the atom TYPE of every (sample, atom), i.e. PotGNN._atom_type_map[atomic_numbers]
 * (_convert_to_atom_type, _gnn.py:541-557), which selects the row of the node-embedding table
 * (_gnn.py:642-643).  Types outside [0, num_atom_types) are refused (RN_ERR_INVALID_ARGUMENT): the
 * reference's Embedding raises for them.  Graph topology stays the reference structure's.
 * host f64 positions -> host f32[S*6] standardised 6-vectors, eval mode.
 */
int rn_potgnn_forward_samples(rn_potgnn *h, const double *lattices, const int32_t *atom_types,
                              const double *positions, int64_t S, float *vec6);

/*
 * PotGNN.forward in evaluation mode as the reference computes it when the model was built under
 * torch.set_default_dtype(torch.float64): its parameters are then float64 and forward computes in their dtype
 * (_gnn.py:617-665, 493-494).  Every kernel instantiated for double (the float32 master weights widened exactly);
 * lattices f64[S*9] or NULL, atom_types int32[S*N] or NULL as for rn_potgnn_forward_samples; vec6 host f64[S*6],
 * standardised (xx,yy,zz,xy,xz,yz).
 */
int rn_potgnn_forward_samples_f64(rn_potgnn *h, const double *lattices, const int32_t *atom_types,
                                  const double *positions, int64_t S, double *vec6);

/*
 * The same on DEVICE buffers (PotGNN.forward with CUDA tensors: the reference returns its result on the device its
 * inputs live on, _gnn.py:617-665, test/tests/torch/test_gnn.py:130-160): d_lattices device f32[S*9] or NULL,
 * d_atom_types device int32[S*N] or NULL (already validated by the caller: entries in [0, num_atom_types)),
 * d_positions device f64[S*N*3] -> d_vec6 device f32[S*6]; work is enqueued on `stream`.
 */
int rn_potgnn_forward_samples_device(rn_potgnn *h, const float *d_lattices, const int32_t *d_atom_types,
                                     const double *d_positions, int64_t S, float *d_vec6, void *stream, int synchronize);

/*
 * Replaces the finite-difference loop of Phonons.get_raman_spectrum
 * (ramannoodle/dynamics/_phonon.py:93-106) with ONE batched evaluation of the 2M
 * displaced cells in double precision on the device:
 *   raman[m] = (alpha(ref + delta*d_m) - alpha(ref - delta*d_m)) / delta
 * (divides by delta, not 2*delta -- as the reference does).
 *   ref_positions host f64[N*3], displacements host f64[M*N*3], raman host f64[M*9].
 */
int rn_potgnn_raman_tensors(rn_potgnn *h, const double *ref_positions,
                            const double *displacements, int64_t M, double delta,
                            double *raman);

/*
 * Jacobian of the standardised 6-vector (PotGNN.forward, eval mode) with respect to the
 * fractional coordinates at one structure, by reverse-mode differentiation on the device:
 *   jac[k][n][c] = d vec6_k / d x_{n,c},   jac is host f64[6*N*3].
 * use_float64 != 0 evaluates forward and reverse passes in double precision.
 */
int rn_potgnn_alpha_jacobian(rn_potgnn *h, const double *positions, int use_float64, double *jac);

/*
 * Analytic counterpart of rn_potgnn_raman_tensors -- the d(alpha)/d(r) x phonon-eigenvector
 * contraction: raman[m] = 2 * (d alpha / d r)|_ref . d_m   (factor 2: the reference divides
 * its +-delta difference by delta, ramannoodle/dynamics/_phonon.py:106).  One forward and
 * one reverse pass instead of 2M forward passes; differs from the finite difference by
 * O(delta^2).
 */
int rn_potgnn_raman_tensors_analytic(rn_potgnn *h, const double *ref_positions,
                                     const double *displacements, int64_t M, double *raman);

/* ------------------------------------------------------------------ training
 * Replaces the forward/backward of one optimisation step of train_single_epoch
 * (ramannoodle/pmodel/torch/_train.py:63-76); the optimiser itself stays with the caller
 * (torch.optim works on the host copies of the parameters).
 */

/* Replace the parameters of an existing evaluator (same layout as rn_potgnn_create). */
int rn_potgnn_set_weights(rn_potgnn *h, const float *weights, size_t num_weights);

/*
 * PotGNN.forward in TRAINING mode (_gnn.py:617-665 with BatchNorm1d using the statistics of
 * all S*E rows of this batch, _gnn.py:534) on S <= max_chunk_structures frames; keeps the
 * tape for rn_potgnn_train_backward.  Returns the standardised 6-vectors and the batch
 * mean / biased variance of the BatchNorm input (host f32[Fe] each) so that the caller can
 * update running_mean / running_var as torch does.
 */
int rn_potgnn_train_forward(rn_potgnn *h, const double *positions, int64_t S, float *vec6,
                            float *batch_mean, float *batch_var);

/*
 * Gradient of a scalar loss with respect to every parameter, given dL/dvec6 (host f32[S*6])
 * for the batch of the preceding rn_potgnn_train_forward.  `grads` (host f32, length
 * rn_potgnn_weight_count) has the layout of `weights`; entries of buffers
 * (Gaussian offsets, running statistics) are zero.
 */
int rn_potgnn_train_backward(rn_potgnn *h, const float *dvec6, float *grads);

/*
 * rn_potgnn_train_forward with a lattice and / or atom types PER SAMPLE (training-mode PotGNN.forward accepts any
 * lattice[S,3,3] and atomic_numbers[S,N], _gnn.py:603-611, 541-557): `lattices` host f64[S*9] or NULL, `atom_types` host
 * int32[S*N] or NULL, as for rn_potgnn_forward_samples.  The following rn_potgnn_train_backward(_device) differentiates
 * that forward (the embedding gradient is summed per sample's atom types).  _f64: the float64 validation leg.
 */
int rn_potgnn_train_forward_samples(rn_potgnn *h, const double *lattices, const int32_t *atom_types, const double *positions,
                                    int64_t S, float *vec6, float *batch_mean, float *batch_var);
int rn_potgnn_train_forward_samples_f64(rn_potgnn *h, const double *lattices, const int32_t *atom_types,
                                        const double *positions, int64_t S, double *vec6, double *batch_mean,
                                        double *batch_var);

/*
 * Device-resident optimisation (_train.py:63-76 without host round trips).  With device training
 * enabled, rn_potgnn_train_forward also updates the BatchNorm running statistics where the weights
 * live (torch semantics: momentum 0.1, unbiased variance); rn_potgnn_train_backward_device leaves the
 * parameter gradients in HBM (packed layout; rn_potgnn_gradient_buffer exposes the float32 buffer so
 * that data-parallel ranks can all-reduce it in place over RCCL), and rn_potgnn_adam_step applies
 * torch.optim.Adam (no amsgrad; weight_decay is added to the gradient; `step` counts from 1) to the
 * parameters in HBM and recomputes what depends on them.  A step uploads dL/dvec6 (24 B per structure)
 * and downloads S*6 outputs and 2*Fe statistics.  rn_potgnn_get_weights returns the current values
 * in the layout of rn_potgnn_create's `weights` (state_dict order, buffers included).
 */
int rn_potgnn_set_device_training(rn_potgnn *h, int enabled);
int rn_potgnn_train_backward_device(rn_potgnn *h, const float *dvec6);
/*
 * The same step with nothing crossing PCIe (round 4: train_single_epoch moves a batch to the device and takes the loss
 * there, _train.py:51-75): positions device f64[S*N*3], d_lattices device f32[S*9] or NULL, d_atom_types device int32[S*N]
 * or NULL (validated by the caller) -> d_vec6 device f32[S*6]; then the cotangents d_dvec6 device f32[S*6].  Both need
 * device-resident training (rn_potgnn_set_device_training), order their work after `stream` and make `stream` wait for
 * it; neither synchronises.  The gradients stay in HBM for rn_potgnn_adam_step.
 */
int rn_potgnn_train_forward_samples_device(rn_potgnn *h, const float *d_lattices, const int32_t *d_atom_types,
                                           const double *d_positions, int64_t S, float *d_vec6, void *stream);
int rn_potgnn_train_backward_samples_device(rn_potgnn *h, const float *d_dvec6, void *stream);

/*
 * Input gradients of the forward: vector-Jacobian products of the standardised 6-vectors with respect to the fractional
 * positions and to the lattice.  All pointers are DEVICE memory.
 *
 * rn_potgnn_forward_vjp_device (evaluation mode, running-statistics BatchNorm): d_lattices f64[S][9] (row i = lattice
 * vector i) or NULL (the reference structure's), d_atom_types int32[S][N] atom types or NULL (validated by the caller),
 * d_positions f64[S][N][3], d_dvec6 f64[S][6] one cotangent per frame -> d_dpos f64[S][N][3] and / or d_dlat f64[S][9]
 * (either may be NULL, not both), every entry written.  The forward is recomputed with its tape on lane 0, a work chunk
 * at a time (bounded memory for any S), in float32 or, with use_float64, in the kernels instantiated for double; the
 * taped forward runs on different kernels from the fast evaluation, so float32 gradients belong to the evaluated
 * function up to float32 rounding.  A pending train_forward is discarded (its tape is reused).  Work is ordered after
 * `stream`, `stream` waits for it and is synchronised once at the end.
 *
 * rn_potgnn_train_backward_inputs / _inputs_device: rn_potgnn_train_backward / _samples_device with the input gradients
 * of the pending float32 train_forward written by the same reverse pass (batch-statistics BatchNorm): dpos f64[S][N][3]
 * and / or dlat f64[S][9] (host memory for the first, device memory for the second; the lattice is the one the forward
 * ran on).  The parameter gradients are bit-identical to those of the entries without inputs.  In the host entry
 * grads == NULL leaves them on the device, as rn_potgnn_train_backward_device does.
 */
int rn_potgnn_forward_vjp_device(rn_potgnn *h, const double *d_lattices, const int32_t *d_atom_types,
                                 const double *d_positions, int64_t S, const double *d_dvec6, int use_float64,
                                 double *d_dpos, double *d_dlat, void *stream);
/*
 * Atom-group decomposition (PartialMDRamanSpectrum / PartialPhononRamanSpectrum).  J_i(x) = d alpha / d x_i is the derivative
 * of the de-standardised polarizability (sigma applied, mu drops out) with respect to atom i's fractional coordinates, in
 * evaluation mode; labels host int32[N] put atom i in group labels[i], 1 <= G <= 16, every group non-empty (else
 * RN_ERR_INVALID_ARGUMENT).  The atoms are bucketed by group as a CSR permutation, rebuilt on the handle when the labels
 * change, and each group is summed in a fixed order without atomics.  The Jacobian rows come from the existing reverse
 * pass, whose EdgeBlock backward accumulates cotangents with atomics: repeated calls and different chunkings agree to
 * round-off, not bit for bit.
 *
 * rn_potgnn_group_increments_device: d_positions device f64[S][N][3] (fractional, wrapped), S >= 2 -> d_out device
 * f64[S-1][G][9], the trapezoid increments
 *   d_out[t][g] = sum_{i in g} 1/2 (J_i(x_t) + J_i(x_{t+1})) . dx_{t,i},   dx_t = x_{t+1} - x_t - round(x_{t+1} - x_t),
 * so that sum_g d_out[t][g] = alpha(x_{t+1}) - alpha(x_t) + O(|dx|^3).  The Jacobian rows of a chunk of frames come from
 * the taped forward on lane 0 and one reverse pass with six one-hot cotangents per frame, in float32 or, with use_float64,
 * in the kernels instantiated for double; chunks of frames overlap by one frame (its rows are carried over).  The tape,
 * the reverse pass and the rows of one chunk stay within workspace_limit bytes (0 = 4 GiB); a limit that not one step
 * fits in returns RN_ERR_OUT_OF_MEMORY.  A pending train_forward is discarded.  Work is ordered after `stream`, `stream`
 * waits for it and is synchronised once at the end.
 *
 * rn_potgnn_group_increments_cells_device: the same for a variable cell.  d_lattices device f64[S][9] (row-major, rows =
 * lattice vectors; NULL: exactly the entry above) -> d_out device f64[S-1][G+1][9].  In a deforming cell alpha(x, L) also
 * changes with L at fixed fractional positions, so the increments gain a CELL CHANNEL, the last one:
 *   d_out[t][g] = sum_{i in g} 1/2 (J_i(x_t, L_t) + J_i(x_{t+1}, L_{t+1})) . dx_{t,i}                    g < G
 *   d_out[t][G] = 1/2 (J_L(x_t, L_t) + J_L(x_{t+1}, L_{t+1})) : (L_{t+1} - L_t),   J_L = d alpha / d L  [3][3] per entry
 * and sum over all G + 1 channels = alpha(x_{t+1}, L_{t+1}) - alpha(x_t, L_t) + O(3rd order).  Every Jacobian row is
 * taken at its frame's own lattice; J_L comes out of the same reverse pass (geom_input_bwd_kernel's dlat rows) and is
 * carried over chunk boundaries with the position rows (6 * 9 more doubles a frame, counted against workspace_limit).
 * The cell channel is a kernel of its own: one wave per step, a fixed summation order, no atomics; with a constant
 * lattice it is exactly 0.  Float32 runs evaluate at the lattices cast to float32 and take L_{t+1} - L_t in float64.
 * The cell counts as a group: 1 <= G <= 15, else RN_ERR_INVALID_ARGUMENT.  The lattices are not inspected (device memory).
 *
 * rn_potgnn_partial_raman_tensors: host pointers ref_positions f64[N*3], displacements f64[M][N][3] -> raman
 * f64[M][G][9], R[m][g] = 2 sum_{i in g} J_i(ref) . d_{m,i} (the factor 2 of rn_potgnn_raman_tensors_analytic, so that
 * sum_g R[m][g] is that entry's tensor): one float64 Jacobian at the reference positions, then the same contraction kernel.
 */
int rn_potgnn_group_increments_device(rn_potgnn *h, const double *d_positions, int64_t S, const int32_t *labels, int G,
                                      int use_float64, size_t workspace_limit, double *d_out, void *stream);
int rn_potgnn_group_increments_cells_device(rn_potgnn *h, const double *d_positions, const double *d_lattices, int64_t S,
                                            const int32_t *labels, int G, int use_float64, size_t workspace_limit,
                                            double *d_out, void *stream);
int rn_potgnn_partial_raman_tensors(rn_potgnn *h, const double *ref_positions, const double *displacements, int64_t M,
                                    const int32_t *labels, int G, double *raman);
/*
 * Phonon-mode decomposition (ModeMDRamanSpectrum): the trapezoid increments of the entries above, split by phonon mode
 * instead of by atom group.  disp (D) and proj (P) are float64[M][N][3]: D[m] is the fractional displacement of a unit
 * amplitude of mode m and P[m] its dual in fractional coordinates (spectrum.mode_projectors), so that for a complete
 * orthonormal set sum_m D[m][i][a] P[m][j][b] = delta_ij delta_ab.  With J_c(t) = d vec6_c / d x at frame t (the rows
 * [frame][6][N][3] of the group entries' reverse pass, component order xx, yy, zz, xy, xz, yz), map = {0,3,4,3,1,5,4,5,2}
 * and sigma the de-standardisation:
 *   dx_t           = x_{t+1} - x_t - round(x_{t+1} - x_t)
 *   a_c[t][m]      = sum_{i,r} 1/2 (J_c(t) + J_c(t+1))[i][r] D[m][i][r]
 *   q[t][m]        = sum_{i,r} P[m][i][r] dx_t[i][r]
 *   out[t][m][3r+s] = sigma[3r+s] a_{map(r,s)}[t][m] q[t][m]                                            m < M
 *   out[t][M]      = total[t] - sum_{m<M} out[t][m] (ascending m), total[t] = the one-group increment   (the REST, optional)
 * and, with a lattice per frame, one more channel, the cell channel of rn_potgnn_group_increments_cells_device,
 * unchanged: the channels are [modes..., rest?, cell?] and their sum is the sum over all atom groups.  For a complete
 * set the rest is round-off.  D and P belong to the lattice of the phonon calculation even when the cell varies: the
 * identity above is a change of basis in fractional space.  The seven sums over (i, r) run on the float64 matrix pipe
 * (csrc/kernels_mode.hip: 16 steps x 64 modes per workgroup, 3N in ascending tiles of 32) in one fixed order that does not
 * depend on the chunking, without atomics: for given Jacobian rows repeated calls are bit-identical.
 *
 * rn_potgnn_mode_contract_device: handle-free, the contraction alone.  d_jac device f64[frames][6][N][3], d_positions
 * device f64[frames][N][3], d_disp / d_proj device f64[M][N][3], sigma host f64[9] -> d_out device
 * f64[frames-1][out_channels][9]: channels 0..M-1 and, with rest = 1, channel M are written, the others left alone.
 * Runs on `stream` of the current device and synchronises it before it returns.  RN_ERR_INVALID_ARGUMENT, before any
 * device work: a null pointer, frames < 2, N < 1, M < 1 (or > 64 * 65535), rest not 0 or 1, out_channels < M + rest.
 *
 * rn_potgnn_mode_increments_device: d_positions device f64[S][N][3], d_lattices device f64[S][9] or NULL, disp / proj HOST
 * f64[M][N][3] (finite, else RN_ERR_INVALID_ARGUMENT; any M >= 1: there is no cap at 3N, a caller may project on vectors
 * of their own) -> d_out device f64[S-1][M + rest + (d_lattices != NULL)][9].  Chunks, the one-frame carry-over, the
 * stream ordering and workspace_limit are those of rn_potgnn_group_increments_device (the two share the loop); D and P
 * are uploaded once per call and count against workspace_limit.
 */
int rn_potgnn_mode_contract_device(const double *d_jac, int64_t frames, const double *d_positions, int32_t N,
                                   const double *d_disp, const double *d_proj, int32_t M, const double *sigma, int rest,
                                   int out_channels, double *d_out, void *stream);
int rn_potgnn_mode_increments_device(rn_potgnn *h, const double *d_positions, const double *d_lattices, int64_t S,
                                     const double *disp, const double *proj, int32_t M, int rest, int use_float64,
                                     size_t workspace_limit, double *d_out, void *stream);
int rn_potgnn_train_backward_inputs(rn_potgnn *h, const float *dvec6, float *grads, double *dpos, double *dlat);
int rn_potgnn_train_backward_inputs_device(rn_potgnn *h, const float *d_dvec6, double *d_dpos, double *d_dlat,
                                           void *stream);
int rn_potgnn_gradient_buffer(rn_potgnn *h, void **device_ptr, size_t *count);
int rn_potgnn_adam_step(rn_potgnn *h, double lr, double beta1, double beta2, double eps,
                        double weight_decay, int64_t step);
int rn_potgnn_get_weights(rn_potgnn *h, float *weights, size_t num_weights);

/*
 * The same step evaluated in float64 on the device (every kernel of the forward and of the
 * reverse pass has a double instantiation): what the float32 gradients are validated against,
 * next to float64 autograd through the oracle.  vec6 / batch_mean / batch_var / dvec6 / grads
 * are host float64 arrays with the layouts of the float32 entry points.
 */
int rn_potgnn_train_forward_f64(rn_potgnn *h, const double *positions, int64_t S, double *vec6,
                                double *batch_mean, double *batch_var);
int rn_potgnn_train_backward_f64(rn_potgnn *h, const double *dvec6, double *grads);

/*
 * Data-parallel training (gradient all-reduce plus all-reduced BatchNorm batch
 * statistics for single-device parity).  With a reducer installed, rn_potgnn_train_forward /
 * _backward hand it the float64 column sums of the readout BatchNorm (forward: sum z, sum z^2
 * and the row count; backward: sum dy, sum dy*zhat) and continue with what it leaves in
 * `values`: the element-wise SUM over all ranks.  Every rank must take the same number of
 * training steps.  The parameter gradients returned by rn_potgnn_train_backward are those of
 * this rank's rows; averaging them over ranks (what DistributedDataParallel does) gives the
 * gradient of the mean loss over the global batch.  fn == NULL removes the reducer.
 * rn_potgnn_train_row_count: rows the last train_forward's statistics covered (all ranks),
 * for the unbiased running variance.
 */
typedef int (*rn_potgnn_reduce_fn)(double *values, int64_t count, void *ctx);
int rn_potgnn_set_stat_reducer(rn_potgnn *h, rn_potgnn_reduce_fn fn, void *ctx);
double rn_potgnn_train_row_count(const rn_potgnn *h);

/* ------------------------------------------------------------------ introspection */

/*
 * On-device reduction of a polarizability time series to the unpolarised MD Raman spectrum
 * before the laser / Bose-Einstein corrections: replaces the diff, the seven
 * autocorrelations and the seven FFTs of MDRamanSpectrum.measure (ramannoodle/spectrum/_raman.py:
 * 282-297 via calc_signal_spectrum, spectrum/utils.py:76-124) by one batched forward FFT, one
 * weighted power spectrum, one inverse FFT and one length-(S-1) FFT in float64 (hipFFT, loaded
 * on first use: RN_ERR_UNSUPPORTED if it cannot be).  alpha: host float64[S][3][3];
 * intensities: host float64[num_bins] with num_bins = ceil((S-1)/2) - 1, the non-negative
 * frequencies of fftfreq(S-1) without the zero bin (45 a^2 + 7 g^2, same scale as the reference).
 */
int rn_md_raman_intensities(const double *alpha, int64_t S, int device, double *intensities,
                            int64_t num_bins);
/*
 * The same reduction for a time series that is already in HBM (the output of
 * rn_potgnn_forward_device, produced on `stream`): d_alpha is a device float64[S][3][3]; only the
 * num_bins intensities travel to the host (intensities: host float64[num_bins]).  hipFFT plans and
 * work buffers are cached per (device, S) by both entry points.
 */
int rn_md_raman_intensities_device(const double *d_alpha, int64_t S, int device, double *intensities,
                                   int64_t num_bins, void *stream);

/*
 * Polarized / oriented MD Raman spectra of K configurations (MDRamanSpectrum.measure_polarized before
 * the laser / Bose-Einstein corrections).  With da(t) = alpha(t+1) - alpha(t) and its symmetric part
 * d(t) = (xx, yy, zz, xy, yz, xz) (component order 0..5; the off-diagonal ones are (a_ij + a_ji) / 2),
 * configuration k's intensities are
 *   I_k(f) = sum_{j<=l} weights[k][p(j,l)] C_jl(f),   f = bins 1..num_bins of fftfreq(S-1),
 * where C_jl is calc_signal_spectrum's transform (real part of the length-(S-1) FFT of the positive
 * lags) of the symmetrised cross-correlation (r_jl(t) + r_lj(t)) / 2, r_jl(t) = sum_n d_j(n+t) d_l(n).
 * The 21 pairs are packed row-major over the upper triangle, p = (0,0) (0,1) .. (0,5) (1,1) .. (1,5)
 * (2,2) .. (5,5); the weights of a symmetric 6x6 form M_k are M_k[j][j] on the diagonal and
 * 2 M_k[j][l] off it.  For the signal s_k = w_k . d (e_s . R da R^T . e_i), M_k = w_k w_k^T, and I_k is
 * calc_signal_spectrum(s_k) without the zero bin.  The device computes the 21 basis spectra once
 * (6 + 2 * 21 FFTs whatever K is) and contracts them with the weights; it never sees geometry.
 * alpha: host float64[S][3][3]; weights: host float64[K][21]; intensities: host float64[K][num_bins],
 * num_bins = ceil((S-1)/2) - 1 as for rn_md_raman_intensities (same argument checks and codes,
 * RN_ERR_UNSUPPORTED without hipFFT).  workspace_limit (bytes, 0 = 4 GiB) bounds the device memory of
 * the call besides the staged copy of alpha: the pairs go through the FFTs in groups of at most 21,
 * as many as fit, and the intensities reach the host in blocks of configurations; a limit that not even
 * one pair and one configuration fit in returns RN_ERR_OUT_OF_MEMORY.  hipFFT plans and work buffers
 * are cached per (device, S, group size), apart from rn_md_raman_intensities' cache.  The work runs on
 * the null stream and the call returns when the intensities are on the host.
 */
int rn_md_raman_polarized(const double *alpha, int64_t S, const double *weights, int64_t K, int device,
                          size_t workspace_limit, double *intensities, int64_t num_bins);
/*
 * The same for a time series already in HBM (d_alpha: device float64[S][3][3], produced on `stream`):
 * the call synchronises `stream` before it reads d_alpha, then runs on the null stream; only the
 * K * num_bins intensities travel to the host.
 */
int rn_md_raman_polarized_device(const double *d_alpha, int64_t S, const double *weights, int64_t K, int device,
                                 size_t workspace_limit, double *intensities, int64_t num_bins, void *stream);

/*
 * Partial (atom-group) MD Raman spectra of K configurations from per-group increments: increments host
 * float64[N][G][9] (N = S - 1 steps, N >= 2; group g's da(t), e.g. from rn_potgnn_group_increments_device), 1 <= G <= 16,
 * weights host float64[K][21] as for rn_md_raman_polarized.  With d_g(t) the six components of the symmetric part of
 * group g's increment and M_k the symmetric 6x6 form of configuration k's weights,
 *   I_k[g][h](f) = sum_{c,c'} M_k[c][c'] C(d_{g,c}, d_{h,c'})(f),   f = bins 1..num_bins of fftfreq(N),
 * C(a, b) as C_jl of rn_md_raman_polarized (calc_signal_spectrum's transform of the symmetrised cross-correlation): so
 * sum_{g,h} I_k[g][h] is rn_md_raman_polarized of the summed increments and I_k[g][g] that of group g alone.
 * intensities: host float64[K][G(G+1)/2][num_bins], the pairs g <= h packed row-major over the upper triangle
 * ((0,0) (0,1) .. (0,G-1) (1,1) ..), num_bins = ceil(N/2) - 1.  The device runs 6G forward FFTs in one batched launch,
 * then per block of rows (k, g <= h) a contraction kernel, an inverse FFT and a length-N FFT.  workspace_limit (bytes,
 * 0 = 4 GiB) bounds the device memory besides the staged increments: a limit that the components and one row do not fit
 * in returns RN_ERR_OUT_OF_MEMORY.  hipFFT plans and buffers are cached per (device, N, G, rows per block), apart from
 * the caches of rn_md_raman_intensities and rn_md_raman_polarized.  Work runs on the null stream; the call returns when
 * the intensities are on the host (RN_ERR_UNSUPPORTED without hipFFT).
 */
int rn_md_raman_partial(const double *increments, int64_t N, int G, const double *weights, int64_t K, int device,
                        size_t workspace_limit, double *intensities, int64_t num_bins);
/* The same for increments already in HBM (d_increments: device float64[N][G][9], produced on `stream`): the call
 * synchronises `stream` before it reads them; only the intensities travel to the host. */
int rn_md_raman_partial_device(const double *d_increments, int64_t N, int G, const double *weights, int64_t K,
                               int device, size_t workspace_limit, double *intensities, int64_t num_bins, void *stream);

/*
 * Segment-averaged (Welch) and time-resolved MD Raman spectra of K configurations (MDRamanSpectrum.measure_segments /
 * measure_segments_polarized before the laser / Bose-Einstein corrections).  The series alpha[0..S-1] is cut into
 * Q = (S - segment_steps) / hop + 1 segments of segment_steps polarizabilities, segment q starting at step q * hop; with
 * n = segment_steps - 1 and the taper tau[0..n-1] (host float64[n], already normalised to mean(tau^2) = 1), segment q's
 * tapered differences are
 *   d_q[t] = tau[t] (alpha[q hop + t + 1] - alpha[q hop + t]),   t = 0..n-1,
 * and row (q, k) is rn_md_raman_polarized's I_k(f) evaluated on d_q instead of the whole series' differences: bins
 * 1..num_bins of fftfreq(n), num_bins = ceil(n/2) - 1, weights host float64[K][21] as there.  With tau = 1, row q is
 * rn_md_raman_polarized of alpha[q hop .. q hop + segment_steps); with any taper, of the series (0, cumsum(d_q)).
 * intensities: host float64[Q][K][num_bins] (average = 0), or float64[K][num_bins], the arithmetic mean of the Q rows of
 * each configuration with no further normalisation (average = 1): magnitudes scale with the segment length as
 * rn_md_raman_polarized's do with S.  Everything after the contracted power spectrum is linear, so the mean is taken
 * before the inverse transform: 6 Q forward FFTs and 2 K more, against Q (6 + 2 * 21) for Q calls of
 * rn_md_raman_polarized (fewer when K < 21 Q; beyond that the gain is the Q K rows that are neither transformed back nor
 * copied).  When neither the K rows of the mean nor the Q segments fit the workspace in one block each, the segments are
 * transformed again for every block of configurations.  Each (k, f) of the mean is summed by one thread in segment
 * order, without atomics: repeated calls are bit-identical.  Checks, in this order: a null pointer, K < 1,
 * segment_steps < 3 or > S, hop < 1, a wrong num_bins, average not 0 or 1 (RN_ERR_INVALID_ARGUMENT each); hipFFT missing
 * (RN_ERR_UNSUPPORTED); a bad device (RN_ERR_NO_DEVICE).  workspace_limit (bytes, 0 = 4 GiB) bounds the device memory of the call besides the staged copy of
 * alpha: the segments go through the forward FFTs in blocks, as many as fit, and the rows through the inverse and length-n
 * FFTs in sub-blocks; a limit that one segment and one row do not fit in returns RN_ERR_OUT_OF_MEMORY.  hipFFT plans and
 * work buffers are cached per (device, n, segments per block, rows per block), apart from the caches of the other three
 * reducers.  The work runs on the null stream and the call returns when the intensities are on the host.
 */
int rn_md_raman_segments(const double *alpha, int64_t S, int64_t segment_steps, int64_t hop, const double *taper,
                         const double *weights, int64_t K, int average, int device, size_t workspace_limit,
                         double *intensities, int64_t num_bins);
/* The same for a time series already in HBM (d_alpha: device float64[S][3][3], produced on `stream`): the call
 * synchronises `stream` before it reads d_alpha, then runs on the null stream; only the intensities travel to the host. */
int rn_md_raman_segments_device(const double *d_alpha, int64_t S, int64_t segment_steps, int64_t hop, const double *taper,
                                const double *weights, int64_t K, int average, int device, size_t workspace_limit,
                                double *intensities, int64_t num_bins, void *stream);

/*
 * rn_md_raman_segments with the segments laid by a table: segment q starts at step starts[q] (host int64[Q], Q >= 1)
 * instead of q * hop, d_q[t] = tau[t] (alpha[starts[q] + t + 1] - alpha[starts[q] + t]).  alpha may be several runs
 * joined end to end: the caller lays the table so that no segment crosses a run boundary (the difference across one is
 * a jump that would put a broadband artefact into every bin), and average = 1 is then the mean over all segments of
 * all runs in one call.  intensities: host float64[Q][K][num_bins] (average = 0, rows in table order) or
 * float64[K][num_bins] (average = 1).  Taper, weights, num_bins, the mean on the power spectra in table order without
 * atomics, workspace_limit (which also counts the 8 Q bytes of the table), RN_ERR_OUT_OF_MEMORY and the null stream are
 * rn_md_raman_segments'; with starts[q] = q * hop the result is bit-identical to it (the same arithmetic in the same
 * order).  Checks, before any device work: a null pointer, K < 1, segment_steps < 3 or > S, Q < 1, a wrong num_bins,
 * average not 0 or 1, a start < 0 or > S - segment_steps (RN_ERR_INVALID_ARGUMENT each); then hipFFT and the device as
 * there.  Plans and work buffers are cached in a cache of their own, shared with rn_md_raman_partial_segments and apart
 * from the caches of the other four reducers.
 */
int rn_md_raman_segments_at(const double *alpha, int64_t S, int64_t segment_steps, const int64_t *starts, int64_t Q,
                            const double *taper, const double *weights, int64_t K, int average, int device,
                            size_t workspace_limit, double *intensities, int64_t num_bins);
/* The same for a time series already in HBM (d_alpha: device float64[S][3][3], produced on `stream`): the call
 * synchronises `stream` before it reads d_alpha; starts, taper and weights stay host arrays. */
int rn_md_raman_segments_at_device(const double *d_alpha, int64_t S, int64_t segment_steps, const int64_t *starts,
                                   int64_t Q, const double *taper, const double *weights, int64_t K, int average,
                                   int device, size_t workspace_limit, double *intensities, int64_t num_bins,
                                   void *stream);

/*
 * Replicate spectra of rn_md_raman_segments_at's segment mean, for error bars: R linear combinations of the Q segments'
 * spectra, formed on the power spectra before the back half, which is linear, exactly as average = 1 forms the mean.
 * alpha, S, segment_steps = W (n = W - 1), starts, Q, taper, weights, K and num_bins as for rn_md_raman_segments_at;
 * replicate_weights: host float64[R][Q], R >= 1, any finite values (zero and negative ones included), applied as given
 * with no normalisation: a bootstrap draw of blocks of segments, a delete-one-block jackknife mean, a block mean.
 *   intensities[r][k] = back half of  sum_q replicate_weights[r][q] P_qk(f),   P_qk the contracted power spectrum of
 *                       segment q and configuration k (row (q, k) of average = 0 is the back half of P_qk alone)
 * host float64[R][K][num_bins]; it equals replicate_weights @ (the rows of average = 0) up to rounding, at 6 Q forward
 * FFTs and 2 R K more instead of Q (6 + 2 K), and only the R K rows are copied.  A row of 1/Q is the mean of average = 1
 * up to rounding; a row of zeros gives rows that are exactly zero.  The sum over q is a float64 matrix product on the
 * matrix pipe whose right operand (the 21 pair powers of each segment at each frequency) is generated in registers
 * (csrc/spectrum_replicates.hip).  Every (r, k, f) is summed by one lane, segments in table order, without atomics:
 * repeated calls with the same arguments are bit-identical.  Blocks of segments are multiples of four, so the products
 * group the same segments whatever the block size, but each block's sum is contracted with the weights before it is
 * added to the stored partial result: calls whose workspace_limit gives a different number of segment blocks agree to
 * rounding error, not bit for bit.  Checks, before any device work: a null pointer, K < 1, R < 1, segment_steps < 3 or
 * > S, Q < 1, a wrong num_bins, a start out of range, a replicate weight that is not finite (RN_ERR_INVALID_ARGUMENT
 * each); then hipFFT (RN_ERR_UNSUPPORTED) and the device (RN_ERR_NO_DEVICE).  workspace_limit (bytes, 0 = 4 GiB) bounds
 * the device memory besides the staged copy of alpha: the taper, the weights, the table, the replicate weights
 * (8 R Q bytes, R and Q rounded up to multiples of 16 and 4), the segments' series and the accumulator rows with their
 * bins.  The segments go through in blocks of a multiple of four, the rows in blocks of whole 16-replicate tiles with
 * all K configurations or, when those do not fit, one tile with some of the configurations; a limit that four
 * segments (or all Q) and one row of each replicate of a tile do not fit in returns RN_ERR_OUT_OF_MEMORY.  Plans and
 * work buffers are cached in a cache of their own.  Work runs on the null stream; the call returns when the intensities
 * are on the host.
 */
int rn_md_raman_segment_replicates(const double *alpha, int64_t S, int64_t segment_steps, const int64_t *starts,
                                   int64_t Q, const double *taper, const double *weights, int64_t K,
                                   const double *replicate_weights, int64_t R, int device, size_t workspace_limit,
                                   double *intensities, int64_t num_bins);
/* The same for a time series already in HBM (d_alpha: device float64[S][3][3], produced on `stream`): the call
 * synchronises `stream` before it reads d_alpha; starts, taper, weights and replicate_weights stay host arrays. */
int rn_md_raman_segment_replicates_device(const double *d_alpha, int64_t S, int64_t segment_steps,
                                          const int64_t *starts, int64_t Q, const double *taper, const double *weights,
                                          int64_t K, const double *replicate_weights, int64_t R, int device,
                                          size_t workspace_limit, double *intensities, int64_t num_bins, void *stream);
/* Device time of the phases of the most recent rn_md_raman_segment_replicates(_device) call (HIP events on the null
 * stream): millis[4] = segment builder, forward FFTs, product kernel, back half with its copies to the host.  Measured
 * only while enabled with rn_md_raman_segment_replicates_set_profiling(1). */
int rn_md_raman_segment_replicates_set_profiling(int enabled);
int rn_md_raman_segment_replicates_phase_times(double *millis);

/*
 * Segment-averaged (Welch) and time-resolved partial (atom-group) MD Raman spectra: rn_md_raman_partial per segment of a
 * start table.  increments: host float64[N][G][9], 1 <= G <= 16; increment t belongs to the step from frame t to frame
 * t + 1 of the N + 1 frames, so frame indices mean what they mean in rn_md_raman_segments_at: a segment of
 * segment_steps = W frames starting at frame starts[q] uses the n = W - 1 increments starts[q] .. starts[q] + W - 2,
 * multiplied by tau[0..n-1], and 0 <= starts[q], starts[q] + W - 1 <= N.  Runs are joined with one row between them
 * (the increment across the boundary, or zeros) that no segment of a boundary-respecting table reads.  Row (q, k, g <= h)
 * is rn_md_raman_partial's I_k[g][h](f) of segment q's tapered increments, bins 1..num_bins of fftfreq(n),
 * num_bins = ceil(n/2) - 1.  intensities: host float64[Q][K][G(G+1)/2][num_bins] (average = 0) or
 * float64[K][G(G+1)/2][num_bins] (average = 1: the arithmetic mean over the segments, taken on the contracted cross-power
 * spectra before the inverse transform, summed per (row, frequency) by one thread in table order: repeated calls are
 * bit-identical), the pairs packed as in rn_md_raman_partial.  The mean costs 6 G Q forward FFTs and 2 K G(G+1)/2 more.
 * Checks, before any device work: a null pointer, G < 1 or > 16, N < 1, K < 1, segment_steps < 3 or > N + 1, Q < 1, a
 * wrong num_bins, average not 0 or 1, a start out of range (RN_ERR_INVALID_ARGUMENT each); then hipFFT
 * (RN_ERR_UNSUPPORTED) and the device (RN_ERR_NO_DEVICE).  workspace_limit (bytes, 0 = 4 GiB) bounds the device memory
 * besides the staged increments: segments go through the forward FFTs in blocks and rows through the back half in
 * sub-blocks; a limit that one segment and one row do not fit in returns RN_ERR_OUT_OF_MEMORY.  Work runs on the null
 * stream; the call returns when the intensities are on the host.
 */
int rn_md_raman_partial_segments(const double *increments, int64_t N, int G, int64_t segment_steps,
                                 const int64_t *starts, int64_t Q, const double *taper, const double *weights,
                                 int64_t K, int average, int device, size_t workspace_limit, double *intensities,
                                 int64_t num_bins);
/* The same for increments already in HBM (d_increments: device float64[N][G][9], produced on `stream`): the call
 * synchronises `stream` before it reads them; only the intensities travel to the host. */
int rn_md_raman_partial_segments_device(const double *d_increments, int64_t N, int G, int64_t segment_steps,
                                        const int64_t *starts, int64_t Q, const double *taper, const double *weights,
                                        int64_t K, int average, int device, size_t workspace_limit,
                                        double *intensities, int64_t num_bins, void *stream);

/*
 * Vibrational density of states (VDOS) of an MD run, whole and by atom group, on the wavenumber axis of the MD Raman
 * spectra of the same run.  positions: host float64[S][N][3], fractional, wrapped into the cell or not; lattices: host
 * float64[num_lattices][3][3], rows = lattice vectors, num_lattices = 1 (a fixed cell) or S (a lattice per frame);
 * masses: host float64[N], finite and positive; labels: host int32[N], the group of each atom in [0, G), 1 <= G <= 16;
 * starts: host int64[Q], the first frame of each segment of segment_steps = W frames (n = W - 1 steps),
 * 0 <= starts[q] <= S - W; taper: host float64[n].
 *   minimum-image step   df[t] = f[t+1] - f[t], df -= rint(df) (round to nearest even)
 *   Cartesian step       u[t] = df[t] @ M[t], M[t] = lattices[0], or (lattices[t] + lattices[t+1]) / 2 for a lattice per
 *                        frame (the motion relative to the deforming cell); not divided by the timestep
 *   segment series       x_{q,i,c}[t] = taper[t] sqrt(masses[i]) u[starts[q] + t][i][c], t = 0..n-1
 *   row (q, g)           D_{q,g}(f) = sum over the atoms i of group g and c = x, y, z of C(x_{q,i,c})(f), C = the real part
 *                        of the length-n transform of the positive lags of the autocorrelation (rn_md_raman_intensities'
 *                        transform of one series), bins 1..num_bins of fftfreq(n), num_bins = ceil(n/2) - 1
 * computed as P_{q,g}(w) = sum_{i in g, c} |X_{q,i,c}(w)|^2 on the zero-padded length L >= 2n - 1 followed by the back
 * half of rn_md_raman_segments (inverse transform, positive lags scaled by 1/L, length-n transform, real bins): 3 N
 * forward FFTs per segment and G back halves.  densities: host float64[Q][G][num_bins] (average = 0) or
 * float64[G][num_bins] (average = 1: the arithmetic mean over the segments, taken on P before the inverse transform).
 * The whole-run VDOS is the one segment starts = {0}, segment_steps = S, taper = 1.  Every (row, frequency) is summed by
 * one thread, segment by segment in table order and atom by atom in ascending index, without atomics: repeated calls
 * are bit-identical and the order does not depend on the block sizes below.
 * Checks, before any device work: a null pointer, N < 1, G < 1 or > 16, num_lattices other than 1 or S, segment_steps < 3
 * or > S, Q < 1, a wrong num_bins, average not 0 or 1, a start out of range, a label outside [0, G), a mass that is not
 * finite and positive (RN_ERR_INVALID_ARGUMENT each); then hipFFT (RN_ERR_UNSUPPORTED) and the device
 * (RN_ERR_NO_DEVICE).  workspace_limit (bytes, 0 = 4 GiB) bounds the device memory besides the staged positions and
 * lattices: atoms and segments go through the forward FFTs in blocks (all atoms of several segments, or some atoms of
 * one segment) and, when G rows do not fit, the groups in blocks; a limit that one atom of one segment and one row do
 * not fit in returns RN_ERR_OUT_OF_MEMORY.  Work runs on the null stream; the call returns when the densities are on the
 * host.
 */
int rn_md_vdos(const double *positions, const double *lattices, int64_t num_lattices, int64_t S, int32_t N,
               const double *masses, const int32_t *labels, int G, int64_t segment_steps, const int64_t *starts,
               int64_t Q, const double *taper, int average, int device, size_t workspace_limit, double *densities,
               int64_t num_bins);
/* The same for positions and lattices already in HBM (device float64[S][N][3] and [num_lattices][3][3], produced on
 * `stream`): the call synchronises `stream` before it reads them; masses, labels, starts and taper stay host arrays. */
int rn_md_vdos_device(const double *d_positions, const double *d_lattices, int64_t num_lattices, int64_t S, int32_t N,
                      const double *masses, const int32_t *labels, int G, int64_t segment_steps, const int64_t *starts,
                      int64_t Q, const double *taper, int average, int device, size_t workspace_limit,
                      double *densities, int64_t num_bins, void *stream);
/* Device time of the phases of the most recent rn_md_vdos / rn_md_vdos_device call (HIP events on the null stream):
 * millis[4] = series builder, forward FFTs, group power kernel, back half with its copies to the host.  Measured only
 * while enabled with rn_md_vdos_set_profiling(1); the events cost a few microseconds per launch. */
int rn_md_vdos_set_profiling(int enabled);
int rn_md_vdos_phase_times(double *millis);

/*
 * Mode-projected VDOS of an MD run: the power spectrum of the run's mass-weighted steps projected onto given vectors
 * (the harmonic eigenvectors: the normal-mode decomposition of MD), one row per vector, on the axis of rn_md_vdos.
 * positions, lattices, num_lattices, masses, starts, segment_steps = W (n = W - 1 steps) and taper as for rn_md_vdos;
 * vectors: host float64[M][N][3], finite, 1 <= M <= 3 N, applied as given (normalisation is the caller's).
 *   step                 u[t] exactly as in rn_md_vdos (minimum image, then the lattice or the midpoint of two)
 *   mode series          y_{q,k}[t] = taper[t] sum_{i,c} vectors[k][i][c] sqrt(masses[i]) u[starts[q] + t][i][c], t = 0..n-1
 *   row (q, k)           D_{q,k}(f) = C(y_{q,k})(f), C as in rn_md_vdos, bins 1..num_bins of fftfreq(n)
 * computed as P_{q,k}(w) = |Y_{q,k}(w)|^2 on the zero-padded length L >= 2n - 1 followed by the back half of
 * rn_md_raman_segments: M forward FFTs per segment and M back halves.  densities: host float64[Q][M][num_bins]
 * (average = 0) or float64[M][num_bins] (average = 1: the arithmetic mean over the segments, taken on P).  Scaling a
 * vector by c scales its row by c^2; for a complete orthonormal set (M = 3 N) the rows sum to the one-group row of
 * rn_md_vdos.  The sum over (i, c) has one fixed order (atoms ascending in tiles of 32, four columns at a time) that
 * does not depend on the block sizes below, and nothing is summed with atomics: repeated calls are bit-identical.
 * Checks, before any device work: a null pointer, N < 1, M < 1 or > 3 N, num_lattices other than 1 or S,
 * segment_steps < 3 or > S, Q < 1, a wrong num_bins, average not 0 or 1, a start out of range, a mass that is not
 * finite and positive, a vector entry that is not finite (RN_ERR_INVALID_ARGUMENT each); then hipFFT
 * (RN_ERR_UNSUPPORTED) and the device (RN_ERR_NO_DEVICE).  workspace_limit (bytes, 0 = 4 GiB) bounds the device memory
 * besides the staged positions and lattices: the modes go through in blocks when one segment's M series and M rows do
 * not fit, the segments in blocks of several; a limit that one series and one row do not fit in returns
 * RN_ERR_OUT_OF_MEMORY.  Work runs on the null stream; the call returns when the densities are on the host.
 */
int rn_md_mode_vdos(const double *positions, const double *lattices, int64_t num_lattices, int64_t S, int32_t N,
                    const double *masses, const double *vectors, int32_t M, int64_t segment_steps,
                    const int64_t *starts, int64_t Q, const double *taper, int average, int device,
                    size_t workspace_limit, double *densities, int64_t num_bins);
/* The same for positions and lattices already in HBM (device float64[S][N][3] and [num_lattices][3][3], produced on
 * `stream`): the call synchronises `stream` before it reads them; masses, vectors, starts and taper stay host arrays. */
int rn_md_mode_vdos_device(const double *d_positions, const double *d_lattices, int64_t num_lattices, int64_t S,
                           int32_t N, const double *masses, const double *vectors, int32_t M, int64_t segment_steps,
                           const int64_t *starts, int64_t Q, const double *taper, int average, int device,
                           size_t workspace_limit, double *densities, int64_t num_bins, void *stream);
/* Device time of the phases of the most recent rn_md_mode_vdos / rn_md_mode_vdos_device call (HIP events on the null
 * stream): millis[4] = projection kernel, forward FFTs, power kernel, back half with its copies to the host.  Measured
 * only while enabled with rn_md_mode_vdos_set_profiling(1). */
int rn_md_mode_vdos_set_profiling(int enabled);
int rn_md_mode_vdos_phase_times(double *millis);

/*
 * Many-channel MD Raman spectra: the self-spectrum of every channel of a set of increments (the phonon modes of
 * rn_potgnn_mode_increments_device) and the spectrum of their sum, per segment of a start table.  increments: host
 * float64[N][C][9], C >= 1 (unbounded: the pair spectra of rn_md_raman_partial_segments stop at 16 groups, these
 * diagonal ones do not); N, segment_steps = W (n = W - 1 increments), starts, taper, weights and K as for
 * rn_md_raman_partial_segments.
 *   row (q, k, c), c < C   rn_md_raman_partial_segments' I_k[g][g] taken on channel c alone (the self-spectrum)
 *   row (q, k, C)          the same form of the increments summed over all channels, in ascending channel order per
 *                          (step, entry): the whole spectrum
 * so that row C - sum_c row c is the interference between channels.  intensities: host float64[Q][K][C+1][num_bins]
 * (average = 0) or float64[K][C+1][num_bins] (average = 1: the mean over the segments, taken on the contracted power
 * spectra in table order by one thread per (row, frequency)).  The summed channel goes through the same kernels as one
 * more channel; channels are independent, so repeated calls and different blockings are bit-identical and a channel of
 * zeros gives rows that are exactly zero.  Checks, their order and the return codes are those of
 * rn_md_raman_partial_segments, with C >= 1 in place of 1 <= G <= 16.  workspace_limit (bytes, 0 = 4 GiB) bounds the
 * device memory besides the staged increments: the channels go through in blocks when one segment's 6 (C + 1) series and
 * K (C + 1) rows do not fit, the segments in blocks of several; a limit that one channel of one segment and one row do
 * not fit in returns RN_ERR_OUT_OF_MEMORY.  Work runs on the null stream; the call returns when the intensities are on
 * the host.
 */
int rn_md_raman_modes(const double *increments, int64_t N, int C, int64_t segment_steps, const int64_t *starts,
                      int64_t Q, const double *taper, const double *weights, int64_t K, int average, int device,
                      size_t workspace_limit, double *intensities, int64_t num_bins);
/* The same for increments already in HBM (d_increments: device float64[N][C][9], produced on `stream`): the call
 * synchronises `stream` before it reads them; only the intensities travel to the host. */
int rn_md_raman_modes_device(const double *d_increments, int64_t N, int C, int64_t segment_steps, const int64_t *starts,
                             int64_t Q, const double *taper, const double *weights, int64_t K, int average, int device,
                             size_t workspace_limit, double *intensities, int64_t num_bins, void *stream);
/* Device time of the phases of the most recent rn_md_raman_modes / rn_md_raman_modes_device call (HIP events on the null
 * stream): millis[4] = segment builder, forward FFTs, power kernel, back half with its copies to the host.  Measured
 * only while enabled with rn_md_raman_modes_set_profiling(1). */
int rn_md_raman_modes_set_profiling(int enabled);
int rn_md_raman_modes_phase_times(double *millis);

/*
 * Mode-by-mode interference matrices of MD Raman bands: the pair spectra between all C channels of a set of increments,
 * summed over weighted bins.  increments, N, C (>= 1, unbounded), segment_steps = W (n = W - 1), starts, Q, taper,
 * weights and K as for rn_md_raman_modes; bin_weights: host float64[B][num_bins], B >= 1, any finite values (a band
 * indicator times the corrections of its bins).  With I_k[m][n][bin] the segment-averaged pair spectrum of channels m
 * and n that rn_md_raman_partial_segments (average = 1) would return were there no cap on its groups,
 *   matrices[b][k][m][n] = sum_bin bin_weights[b][bin] I_k[m][n][bin]
 * host float64[B][K][C][C]: the full symmetric matrix, the lower triangle a bit-for-bit mirror of the upper.  There is
 * no summed channel: the band's whole intensity is the sum of all entries, entry (m, m) the band sum of channel m's
 * self-spectrum and the sum of row m channel m's share of the band with its cross terms.  Always of the segment mean.
 * The sum over bins is taken on the frequency side (the back half of the reducers is linear in the cross-power: see
 * csrc/spectrum_mode_matrix.hip), as one float64 matrix product on the matrix pipe.  Every entry is summed in one
 * order (segments in table order, frequencies ascending) whatever the blocking, without atomics: repeated calls and
 * different workspace_limits are bit-identical, and a channel of zeros gives a row and a column that are exactly zero.
 * Checks, their order and the return codes are those of rn_md_raman_modes, with B >= 1 and bin_weights non-null beside
 * them, and K and B at most 65535 each (grid dimensions).  workspace_limit (bytes, 0 = 4 GiB) bounds the device memory
 * besides the staged increments: the channels go
 * through in blocks of whole tiles, the segments in blocks of several; a limit that the series of one segment of one
 * pair of channel tiles and that pair's entries do not fit in returns RN_ERR_OUT_OF_MEMORY.  Work runs on the null
 * stream; the call returns when the matrices are on the host.
 */
int rn_md_raman_mode_matrix(const double *increments, int64_t N, int C, int64_t segment_steps, const int64_t *starts,
                            int64_t Q, const double *taper, const double *weights, int64_t K, const double *bin_weights,
                            int64_t B, int device, size_t workspace_limit, double *matrices, int64_t num_bins);
/* The same for increments already in HBM (d_increments: device float64[N][C][9], produced on `stream`): the call
 * synchronises `stream` before it reads them; only the matrices travel to the host. */
int rn_md_raman_mode_matrix_device(const double *d_increments, int64_t N, int C, int64_t segment_steps,
                                   const int64_t *starts, int64_t Q, const double *taper, const double *weights,
                                   int64_t K, const double *bin_weights, int64_t B, int device, size_t workspace_limit,
                                   double *matrices, int64_t num_bins, void *stream);
/* Device time of the phases of the most recent rn_md_raman_mode_matrix / rn_md_raman_mode_matrix_device call (HIP
 * events on the null stream): millis[4] = segment builder, forward FFTs, product kernel, copies of the matrices to the
 * host.  Measured only while enabled with rn_md_raman_mode_matrix_set_profiling(1). */
int rn_md_raman_mode_matrix_set_profiling(int enabled);
int rn_md_raman_mode_matrix_phase_times(double *millis);
/* Host only (no device is touched): the frequency-side weights that rn_md_raman_mode_matrix derives from bin_weights.
 * n = segment_steps - 1 >= 2, L the zero-padded transform length (the least power of two >= 2 n - 1), T[bin][f] =
 * (1/L) sum_{tau=0}^{n-1} cos(2 pi tau (f/L - (bin+1)/n)) and u_b[f] = sum_bin bin_weights[b][bin] T[bin][f]:
 *   response[b][f] = scale * (u_b[f] + u_b[L - f])  for 0 < f < L/2,   scale * u_b[f]  for f = 0 and f = L/2
 * the half-spectrum folded, as the series are real.  response: host float64[B][F], F = L/2 + 1 rounded up to a
 * multiple of 4, the tail zero.  num_bins must be (n + 1) / 2 - 1; RN_ERR_INVALID_ARGUMENT otherwise. */
int rn_md_raman_mode_matrix_response(int64_t n, const double *bin_weights, int64_t B, int64_t num_bins, double scale,
                                     double *response);

/* Introspection: bit 0 = the fused EdgeBlock kernel is in use (float32, Fn and Fe padded to
 * 64); bit 1 = every pass takes the folded-LayerNorm-scale triplet loop; bit 2 = the fused
 * kernels' matrix products run as split-f16 MFMA (default; RN_POTGNN_MFMA=f32 at create time
 * selects the exact-f32 MFMA); bit 3 = the narrow-width kernels (one lane per row; Fn, Fe <= 16 in
 * an instantiated pair, e.g. the documented Fn = 5, Fe = 14) are in use; bit 4 = split-f16 was
 * requested but the range guard refused it (a non-finite weight, or readout hidden activations
 * that the weights allow beyond 3e4): the exact-f32 MFMA instantiations run instead.  Weight
 * matrices of any finite scale are fine: each is prescaled by a power of two into f16's range;
 * bits 5 to 7 = reserved, 0.
 * bit 8 = every pass of a float32 evaluation takes the role-specialised fused EdgeBlock (edge_block_ps_kernel,
 * csrc/kernels_edge_ps.hip: producer waves + consumer waves in one 768-thread workgroup per CU; needs bits 0-2;
 * RN_POTGNN_EDGE_PS=0 at create time keeps the per-frame kernel of bit 0).
 * bit 9 = float32 evaluations take the atom-owning fused NodeBlock (node_block_atom_kernel, csrc/kernels_node_atom.hip:
 * tiles of 16 atoms, round r = their r-th in-edges, the gate on the MFMA accumulators; needs bits 0 and 2 and in-degrees
 * even enough that it pays; RN_POTGNN_NODE_ATOM=0 at create time keeps node_block_fused_kernel).
 * bit 10 = float32 evaluations keep the edge embedding in HBM as split-f16 operand pairs ([f16 hi x8][f16 lo x8] per eight
 * columns, hi = f16(x), lo = f16(x - hi): the MFMA operand itself, same 256 B per row) between the geometry kernel, the
 * EdgeBlocks, the NodeBlocks and the readout; needs bits 8 and 9; RN_POTGNN_PAIR_ROWS=0 at create time keeps float32 rows.
 * bit 11 = such evaluations compute the EdgeBlock's c2 branch once per atom pair in c2_pairs_kernel (csrc/kernels_c2_pairs.hip)
 * instead of once per edge inside the EdgeBlock; needs bit 10 and a graph whose pair rows fit the readout's buffer (at most
 * E / 2 pairs at Fe padded to 64: every edge has its reverse, as in a radius graph; a graph with more unpaired edges keeps the
 * branch in the EdgeBlock); RN_POTGNN_C2_PAIRS=0 at create time keeps it there always. */
int rn_potgnn_config_flags(const rn_potgnn *h);

/*
 * Host-only (no device is touched): the schedule check the library runs per atom tile before it lets the role-specialised
 * EdgeBlock (csrc/kernels_edge_ps.hip) take a graph.  rb[i], re[i] = first and end source row of destination i of the tile
 * (destinations sorted by atom, rows counted within the tile); back = rounds that may still read the ring when a step
 * rewrites it (2 .. 5 in handles the library creates; 1 .. 8 accepted here); ring_tiles = the ring's capacity in 16-row tiles (8; 7 for the GRAM instantiation).  Returns 1 when
 * the producers' schedule holds (never more than two source tiles per step, no ring slot rewritten under a round in
 * flight), 0 when not, a negative rn_status on bad arguments; *window (optional) = the most tiles one round's source rows span.
 */
int rn_potgnn_debug_ps_schedule(const int32_t *rb, const int32_t *re, int32_t num_destinations, int32_t back,
                                int32_t ring_tiles, int32_t *window);

/*
 * Host-only (no device is touched, none is needed): the plan rn_potgnn_create would make for this graph on a device with
 * num_cus compute units, under the RN_POTGNN_* knobs of the environment.  The arguments are validated as rn_potgnn_create
 * validates them (same status codes and texts through rn_potgnn_last_error(NULL)).  The plan is written as int32 values:
 *   FnP, FeP                                   padded widths
 *   five partition slots, in the order EdgeBlock (Graph::tile_begin), NodeBlock (nt_), a reserved slot (always 0, 0, 0, 0),
 *   reverse EdgeBlock (bt_), role-specialised EdgeBlock (pt_); each as
 *     L, begin[0 .. L), max_out_rows, max_in_rows, max_nodes      (L = tiles + 1, or 0: no such partition)
 *   nt_narrow, na_num, na_max_deg, pt_back, pt_gram, T
 *   use_fused, two reserved words (always 0), use_ps, use_narrow, use_node_fused, use_readout_fused, num_lanes
 *   out_ptr[N+1], in_ptr[N+1], in_edge[E], in_pos[E], rev_edge[E], trip_off[E+1]
 * *count = the number of values; when out is NULL or capacity < *count nothing is written and the call returns
 * RN_ERR_INVALID_ARGUMENT with *count set.
 */
int rn_potgnn_debug_plan(const rn_potgnn_config *cfg, const int32_t *edge_a, const int32_t *edge_b,
                         const int32_t *atom_types, int32_t num_cus, int32_t *out, size_t capacity, size_t *count);

/*
 * Host-only, validated like rn_potgnn_debug_plan: the atom-pair table of that plan, as int32 values
 *   NP, pair_of_edge[E], pair_a[NP], pair_b[NP].
 * Edge d and its reverse rev_edge[d] share the pair pair_of_edge[d]; an edge without a reverse is a pair of its own.  Pairs
 * are numbered in ascending order of their lower edge id, and pair_a / pair_b are that edge's atoms.  What depends on the
 * unordered atom pair alone (the EdgeBlock's c2 branch) need be computed once per pair.  *count and
 * the out == NULL / capacity protocol are those of rn_potgnn_debug_plan.
 */
int rn_potgnn_debug_plan_pairs(const rn_potgnn_config *cfg, const int32_t *edge_a, const int32_t *edge_b,
                               const int32_t *atom_types, int32_t num_cus, int32_t *out, size_t capacity, size_t *count);

/*
 * Host-only, validated like rn_potgnn_debug_plan: the dynamic LDS bytes each kernel family of that plan would ask for, from
 * the kernels' own footprint functions.  Written as int64 pairs (float32 instantiation, float64 instantiation), 0 where the
 * family does not run on this plan or has no such instantiation, in the order
 *   unfused EdgeBlock (edge_agg_kernel), reverse EdgeBlock (edge_bwd_tile2_kernel / edge_bwd_tile_kernel; 0: the per-row
 *   kernel without dynamic LDS takes the graph), narrow EdgeBlock, narrow NodeBlock, role-specialised EdgeBlock,
 *   atom-owning NodeBlock, row-ordered fused NodeBlock.
 * A compute unit has 163840 bytes; rn_potgnn_create accepts no graph for which an entry is larger.  *count and the
 * out == NULL / capacity protocol are those of rn_potgnn_debug_plan.
 */
int rn_potgnn_debug_plan_lds(const rn_potgnn_config *cfg, const int32_t *edge_a, const int32_t *edge_b,
                             const int32_t *atom_types, int32_t num_cus, int64_t *out, size_t capacity, size_t *count);

/*
 * Host-only (no device is touched, none is needed): the packed weight blob rn_potgnn_create / rn_potgnn_set_weights would
 * make of the state-dict-ordered `weights` for a model of this configuration, at the padded widths the library plans it
 * at under the RN_POTGNN_* knobs of the environment (csrc/weight_layout.hpp; no graph is needed).  cfg, weights and
 * num_weights are validated as rn_potgnn_create validates them (same status codes and texts through
 * rn_potgnn_last_error(NULL)).  Written, each *count entries long:
 *   packed   the float32 host master copy, derived entries included: the layout rn_potgnn_gradient_buffer exposes
 *   mask     1 where an entry is a trainable parameter (what rn_potgnn_adam_step updates), else 0
 *   writers  (optional, may be NULL) low nibble = state-dict elements stored at the entry, high nibble = derived ranges
 *            (transposed / centred copies, folded constants, prescale pairs, the second copy of readout bias 0) covering it
 * and flags[1 + num_message_passes]: flags[0] = the weights pass the split-f16 range guard (bit 4 of
 * rn_potgnn_config_flags is its negation), flags[1 + p] = pass p's triplet loop may take the folded-gate form.
 * RN_OK also means that the three ranges rn_potgnn_adam_step downloads in one piece each are contiguous in the layout.
 * When packed, mask or flags is NULL or capacity < *count nothing is written and the call returns
 * RN_ERR_INVALID_ARGUMENT with *count set.
 */
int rn_potgnn_debug_pack_weights(const rn_potgnn_config *cfg, const float *weights, size_t num_weights, float *packed,
                                 unsigned char *mask, unsigned char *writers, int32_t *flags, size_t capacity, size_t *count);

/*
 * Host-only inverse: a packed blob of num_packed entries (the *count of rn_potgnn_debug_pack_weights) back into state-dict
 * order, as rn_potgnn_get_weights (buffers != 0: the state dict's buffers -- Gaussian offsets, BatchNorm running
 * statistics -- keep their values) and the gradient download of rn_potgnn_train_backward (buffers == 0: zeros there) do
 * it.  *count = rn_potgnn_weight_count(cfg); the out == NULL / capacity protocol is the one above.
 */
int rn_potgnn_debug_unpack_weights(const rn_potgnn_config *cfg, const float *packed, size_t num_packed, int buffers,
                                   float *out, size_t capacity, size_t *count);

/* Number of edge triplets T of the frozen graph. */
int64_t rn_potgnn_num_triplets(const rn_potgnn *h);

/*
 * Writes the triplet index arrays exactly as the device kernels enumerate them, in
 * the order and meaning of the 7-tuple BatchTriplets holds (_utils.py:161-168):
 * idx_i, idx_j, idx_k, slot5 (= PyG idx_kj), slot6 (= PyG idx_ji); each host int32[T].
 * Produced by a device kernel that shares the enumeration code with the aggregation
 * kernel, so tests can check bit-exact index parity.
 */
int rn_potgnn_debug_triplets(rn_potgnn *h, int32_t *idx_i, int32_t *idx_j,
                             int32_t *idx_k, int32_t *slot5, int32_t *slot6);

/*
 * Copies one intermediate of the most recent evaluation's LAST chunk to the host,
 * un-padded: stage 0 = unit vectors+distance [rows,4], 1 = node embedding after pass
 * `index` (0 = initial) [S_c*N,Fn], 2 = edge embedding after pass `index` [S_c*E,Fe]
 * (only the most recent pass and pass 0... see DESIGN.md: intermediates are kept only
 * when the handle was created with RN_POTGNN_KEEP_STAGES=1 in the environment),
 * 3 = readout embedding [S_c*E,12], 4 = the snapshot stage 2 reads exactly as it lies in memory, padded columns included
 * [S_c*E,FeP] 32-bit words (rows in the kernels' own order; where the rows are split-f16 pairs, bit 10 of
 * rn_potgnn_config_flags, the words hold per eight columns 8 x f16 hi | 8 x f16 lo).  Returns rows written via *rows.
 * RN_POTGNN_KEEP_STAGES=1 puts the run on float32 edge rows and the readout on the layout stage 3 reads.
 * RN_POTGNN_KEEP_STAGES=2 keeps stages 1 and 2 only and leaves the run on the kernels it would take without
 * snapshots (frames are not spread over two lanes, nothing else changes): where its edge rows are split-f16
 * operand pairs (bit 10 of rn_potgnn_config_flags), stage 2 returns them decoded, x = hi + lo.
 */
int rn_potgnn_debug_stage(rn_potgnn *h, int stage, int index, float *out,
                          size_t out_capacity, int64_t *rows, int64_t *cols);

/* Per-kernel device time of the most recent evaluation (HIP events on the handle's
 * stream), accumulated over chunks; names[i] are static strings.  Enabled with
 * rn_potgnn_set_profiling(h, 1).  Returns the number of entries written (<= cap). */
int rn_potgnn_set_profiling(rn_potgnn *h, int enabled);
int rn_potgnn_kernel_times(rn_potgnn *h, const char **names, double *millis,
                           int64_t *launches, int cap);

const char *rn_potgnn_last_error(const rn_potgnn *h);
const char *rn_potgnn_version(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RN_POTGNN_H */
