// The forward engine of the evaluator (forward.hip) as the other host units see it, and what reverse.hip and training.hip
// give api.hip.  The templates are defined in their .hip and instantiated there for float and double.  Host only.
#pragma once
#include "handle.hpp"

namespace rn {

// ---- forward.hip: workspace sizing, weight upload, one chunk's stages, the evaluation, the staged host path
bool lean_workspace(const rn_potgnn *h);
size_t per_structure_elems(const rn_potgnn *h, bool lean);
size_t bufA_width(const rn_potgnn *h, bool lean);
template <typename T>
int chunk_frames(const rn_potgnn *h);  // frames per device work chunk in precision T
void size_chunk(rn_potgnn *h);
void refresh_mfma_mode(rn_potgnn *h);
template <typename T>
void refresh_pass_flags(rn_potgnn *h);
template <typename T>
void device_setup(rn_potgnn *h, T *w, hipStream_t st);
template <typename T>
void upload_weights(rn_potgnn *h);
template <typename T>
void ensure_precision(rn_potgnn *h);

// ensure + a blocking host-to-device copy
template <typename T>
T *stage(DeviceBuf &buf, const void *host, size_t bytes) {
  buf.ensure(bytes);
  HIP_TRY(hipMemcpy(buf.p, host, bytes, hipMemcpyHostToDevice));
  return buf.as<T>();
}
template <typename T>
const T *stage_lattices(rn_potgnn *h, const double *lat, int64_t S);
const int *stage_types(rn_potgnn *h, const int32_t *types, int64_t S);

// (xx, yy, zz, xy, xz, yz) of S standardised 3x3 tensors: dataset/torch/utils.py:44-60
template <typename T>
void pick_vec6(const double *raw, int64_t S, T *vec6) {
  const int pick[6] = {0, 4, 8, 1, 2, 5};
  for (int64_t s = 0; s < S; ++s)
    for (int k = 0; k < 6; ++k) vec6[s * 6 + k] = (T)raw[s * 9 + pick[k]];
}

// What an evaluation of S frames reads and writes: device arrays, frame-major; a null field is absent.
template <typename T>
struct ForwardIO {
  const double *pos = nullptr;     // [S][N][3] fractional positions ...
  const float *pos32 = nullptr;    // ... or, float32 evaluations only, the same as float32 (then pos is null)
  double *alpha = nullptr;         // [S][9] polarizabilities
  float *vec6 = nullptr;           // [S][6] standardised 6-vectors
  double *alpha_raw = nullptr;     // [S][9] the standardised tensor in float64
  const T *lat = nullptr;          // [S][9] per-frame lattices, or null: the reference structure's
  const int *types = nullptr;      // [S][N] per-frame atom types, or null: the reference structure's
  double *desc = nullptr;          // [S][Fe] structure descriptors: the mean of the final edge embedding's rows
  ForwardIO at(int64_t first, int N, int Fe) const {  // the frames from `first` on: the one place that knows the strides
    auto from = [first](auto *p, int64_t stride) { return p ? p + first * stride : nullptr; };
    ForwardIO o;
    o.pos = from(pos, 3 * (int64_t)N);
    o.pos32 = from(pos32, 3 * (int64_t)N);
    o.alpha = from(alpha, 9);
    o.vec6 = from(vec6, 6);
    o.alpha_raw = from(alpha_raw, 9);
    o.lat = from(lat, 9);
    o.types = from(types, N);
    o.desc = from(desc, Fe);
    return o;
  }
};

// One chunk of `S` frames on one lane, split into stages so that two chunks can be
// interleaved (see forward_device).  Mirrors PotGNN.forward (_gnn.py:641-665).
template <typename T>
struct ChunkRun {
  rn_potgnn *h;
  Lane<T> *ln;
  ForwardIO<T> io;  // this chunk's slice
  int S;
  RunChoices ch;  // which kernels this chunk takes
  int cur = 0;
  T *node[2], *edge[2], *unit4, *npc1, *np3, *bufA, *bufB;
  int64_t MN, ME;

  ChunkRun(rn_potgnn *h_, Lane<T> &l, const ForwardIO<T> &io_, int S_);
  hipStream_t st() const { return ln->stream.get(); }
  void target_tape(int slot, int which);
  void snapshot(int p);
  void begin();       // geometry + radial basis, initial node embedding
  void run_stages();  // begin + every pass: what is left is finish(), or the reverse pass over the tape
  void project(const T *X, int64_t R, int K, const T *WT, int NOUT, T *Y, const T *bias, int amode, const T *nd);
  void stage_project(int p);    // "G" stage of pass p: NodeBlock + every dense projection the EdgeBlock needs
  void stage_aggregate(int p);  // "V" stage of pass p: triplet aggregation of the EdgeBlock
  void edge_unfused_in_blocks(int p);
  void finish();  // readout
  T *tape_agg(int p);
};

void check_ps_fail(rn_potgnn *h);
template <typename T>
void behind_caller(rn_potgnn *h, hipStream_t user, Lane<T> *lanes, int n);
template <typename T>
void hand_back(rn_potgnn *h, hipStream_t user, Lane<T> *lanes, int n, bool sync, bool timers = false);
template <typename T>
void forward_device(rn_potgnn *h, const ForwardIO<T> &io, int64_t S, hipStream_t user, bool sync);
// A host entry's evaluation in precision T: stage positions (and lattices, atom types) into io_*, forward_device on the
// null stream, synchronised, and a blocking copy back -- polarizabilities [S][9] into `alpha`, or standardised 6-vectors
// into `vec6` (float32: the kernels' own; float64: picked from the standardised tensor).
template <typename T>
void host_forward(rn_potgnn *h, const double *lattices, const int32_t *types, const double *positions, int64_t S,
                  double *alpha, T *vec6);
template <typename T>
void host_descriptors(rn_potgnn *h, const double *lattices, const double *positions, int64_t S, double *desc, double *alpha);
void staged_forward(rn_potgnn *h, const double *positions, const double *lattices, int64_t S, double *d_alpha, bool sync);
void host_polarizabilities(rn_potgnn *h, const double *positions, const double *lattices, int64_t S, double *alpha);
void read_stage(rn_potgnn *h, int stage, int index, float *out, size_t out_capacity, int64_t *rows, int64_t *cols);

// ---- reverse.hip: the reverse pass over a taped forward and its users
constexpr size_t kTapeBudget = (size_t)4 << 30;

// Reverse pass over a taped forward of S frames with B cotangents per frame.
//   d_dout6   device [S*B, 6]  cotangents of the standardised 6-vectors
//   d_dpos    device f64 [S*B, N, 3] or null   -> d / d(fractional positions), ACCUMULATED (geom_bwd_kernel, the Jacobian)
//   grad      device packed-layout gradient blob or null -> parameter gradients (training)
//   train_bn  readout BatchNorm used batch statistics (z1 / bn_stats hold the taped values)
//   in_dpos / in_dlat  device f64 [S*B, N, 3] / [S*B, 9] or null -> input gradients of forward, WRITTEN (geom_input_bwd_kernel,
//             with the frame's own lattice); computed from the cotangents the pass leaves anyway, so they change nothing else
template <typename T>
struct Reverse {
  int S, B;
  const T *d_dout6;
  double *d_dpos;
  T *grad;
  bool train_bn;
  double *in_dpos = nullptr;
  double *in_dlat = nullptr;
};
template <typename T>
void reverse_pass(rn_potgnn *h, ChunkRun<T> &c, const Reverse<T> &rv);
template <typename T>
ChunkRun<T> taped_forward(rn_potgnn *h, const ForwardIO<T> &io /* pos, lat, types */, int S);
template <typename T>
void jacobian(rn_potgnn *h, const double *host_pos, double *host_jac /*[6][N*3]*/);
template <typename T>
void forward_vjp(rn_potgnn *h, const double *d_lat, const int32_t *d_types, const double *d_pos, int64_t S,
                 const double *d_dvec6, double *d_dpos, double *d_dlat, hipStream_t user);
template <typename T>
void group_increments(rn_potgnn *h, const double *d_pos, int64_t S, int G, size_t limit, double *d_out, hipStream_t user,
                      const double *d_lat = nullptr);
void mode_contract(const double *jac, int64_t frames, const double *pos, int N, const double *disp, const double *proj,
                   int M, const double *sigma, bool rest, int out_channels, double *out, hipStream_t st);
template <typename T>
void mode_increments(rn_potgnn *h, const double *d_pos, int64_t S, const double *disp, const double *proj, int M,
                     bool rest, size_t limit, double *d_out, hipStream_t user, const double *d_lat);
void partial_raman(rn_potgnn *h, const double *ref_positions, const double *displacements, int64_t M, int G, double *raman);

// ---- training.hip: one training step (forward, backward, Adam) in its host and its device-resident form
void reduce_over_ranks(rn_potgnn *h, double *dev, size_t n, hipStream_t st);
void sync_host(rn_potgnn *h);  // refresh `packed` (and the float64 copy, when it exists) from the device weights
template <typename T>
void train_forward(rn_potgnn *h, const double *host_pos, int S, T *vec6, T *batch_mean, T *batch_var,
                   const double *host_lat = nullptr /* [S][9] or null */, const int32_t *host_types = nullptr /* [S][N] or null */);
void train_forward_device(rn_potgnn *h, const double *d_pos, int S, const float *d_lat, const int32_t *d_types,
                          float *d_vec6, hipStream_t user);
template <typename T>
void train_backward(rn_potgnn *h, const T *dvec6, T *grads /* null: leave the gradients on the device */,
                    double *host_dpos = nullptr /* [S][N][3] or null */, double *host_dlat = nullptr /* [S][9] or null */);
void train_backward_device(rn_potgnn *h, const float *d_dvec6, hipStream_t user, double *d_dpos = nullptr,
                           double *d_dlat = nullptr);
void adam_step(rn_potgnn *h, double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step);

}  // namespace rn
