// Host orchestration + C ABI (include/rn_potgnn.h) for the gfx950 PotGNN evaluator.
//
// Planning -- validation of the create arguments, the CSRs, the atom tiles of every kernel family and the choice of the
// family -- is host-only code in graph_plan.hip (rn_potgnn_debug_plan runs it without a device); this file uploads the plan.
// The packed weight layout -- where each state-dict tensor lands, the derived entries, the trainable mask and the decisions
// read off the packed values -- is host-only code in weight_layout.hip (rn_potgnn_debug_pack_weights); this file uploads the blob.
// A handle owns: the frozen graph (CSR both ways, node tiles, triplet offsets), the
// weights re-laid-out for the kernels (weight_layout.hpp), and
// per-"lane" device workspaces (a lane = a HIP stream).  An evaluation walks the frames in
// chunks (hundreds to thousands of frames: large launches amortise launch gaps and tails).
// The fused pipeline (kernels_fused.hip) uses one lane; the unfused one alternates chunks
// between two lanes so that the HBM-bound projections of one chunk overlap the VALU-bound
// aggregation of the other (run_pair).
//
// In file order: weight upload and the flags read off the weights; ForwardIO (what an evaluation reads and writes, sliced per chunk in one place)
// and ChunkRun (one chunk's stages on one lane); forward_device and the reverse pass with their users (Jacobian, input
// gradients, atom groups, training); then the C entries.  The entries share their argument checks (check_batch,
// check_train_batch, check_pending, check_types), their staging (stage, stage_lattices, stage_types, lazy_stream,
// lazy_event) and the ordering bracket around work done for a caller's stream (behind_caller / hand_back).
// The error types, DeviceBuf, set_error and guarded() -- the lock and the try block every entry runs in -- are
// host_runtime.hpp's; the group table, the mode upload, the chunk walk and the checks of the increment entries are
// increments.hpp's, shared with the interpolation model (api_interp.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rn_potgnn.h"
#include "graph_plan.hpp"
#include "host_runtime.hpp"
#include "increments.hpp"
#include "kernels.hpp"
#include "weight_layout.hpp"

using namespace rn;

namespace {

std::string g_create_error;

enum KernelId {
  K_GEOM = 0, K_NODE_INIT, K_PROJ_NODE, K_PROJ_EDGE_C1, K_NODE_AGG, K_PROJ_EDGE_C3, K_PROJ_C2,
  K_EDGE_AGG, K_READOUT_MLP, K_READOUT_REDUCE, K_C2_PAIRS, K_COUNT
};
const char *kKernelNames[K_COUNT] = {
    "geom_rbf", "node_init", "proj_node", "proj_edge_c1", "node_agg", "proj_edge_c3",
    "proj_c2", "edge_agg", "readout_mlp", "readout_reduce", "c2_pairs"};

template <typename T>
struct Lane {
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  DeviceBuf unit4, node[2], edge[2], npc1, np3, bufA, bufB;
  DeviceBuf fbA, fbB;  // a block of frames' c2 / c3 edge projections for a pass the fused pipeline hands to the unfused EdgeBlock
};

template <typename T>
struct Precision {
  bool ready = false;
  DeviceBuf weights;     // packed, type T
  DeviceBuf lattice;     // [9] T
  std::vector<PassW<T>> pass;
  ReadoutW<T> ro{};
  const T *offsets = nullptr, *node_table = nullptr, *ones = nullptr;
  Lane<T> lanes[2];
  // stage snapshots (debug)
  std::vector<DeviceBuf> snap_node, snap_edge;
  // forward tape + cotangent workspace of the reverse pass (Jacobian d alpha / d r)
  std::vector<DeviceBuf> tape_node, tape_edge, tape_agg;
  DeviceBuf bw[18];
  hipStream_t side = nullptr;  // weight-gradient products of the reverse pass run here, beside the cotangent chain
  hipEvent_t ev_side[3] = {nullptr, nullptr, nullptr};
  DeviceBuf tn_arena;  // partial sums of the weight-gradient products (reverse_pass)
  DeviceBuf tape_z1, bn_stats, grad, seeds, mv, type_sums;  // training: pre-BatchNorm activations, batch sums, gradient blob
  DeviceBuf in_dcart, in_lat, in_grads;  // input gradients: per-edge Cartesian cotangents, a chunk's lattices, host-path outputs
  DeviceBuf eye_seeds;  // atom-group increments: one-hot cotangents [frames][6][6], filled once per size
  int eye_frames = 0;
  bool tape_on = false;
};

struct TimedLaunch {
  int kid;
  hipEvent_t a, b;
};

}  // namespace

struct rn_potgnn {
  mutable std::recursive_mutex lock;  // serialises the calls on this handle (guarded(), the small getters / setters, set_error)
  rn_potgnn_config cfg{};
  Dims d{};
  int chunk = 1;
  size_t f64_budget = 0;  // workspace bytes the float64 lanes may take (0: what the float32 lanes were given)
  bool keep_stages = false;
  bool snap_pairs = false;      // RN_POTGNN_KEEP_STAGES=2: the same snapshots of a run that keeps its kernels (edge rows stay split-f16
                                // pairs where they would be; rn_potgnn_debug_stage decodes them); stage 3 is not kept
  bool last_pair_rows = false;  // the last float32 run's edge rows were split-f16 pairs
  bool debug_sync = false;  // RN_POTGNN_DEBUG_SYNC=1: synchronise + check after every kernel
  GraphPlan plan;  // the graph's host arrays, its atom tiles, the kernel family and the lanes (graph_plan.hpp); `g` is its device image
  bool split_projections = true;  // RN_POTGNN_SPLIT_PROJ=0: the forward's stand-alone projections on the exact-f32 MFMA kernel
  bool want_pair_rows = true;   // RN_POTGNN_PAIR_ROWS at create time (ForwardRun::pair_rows decides per run)
  bool want_c2_pairs = true;    // RN_POTGNN_C2_PAIRS at create time (ChunkRun::c2_pairs decides per run)
  DeviceBuf step_seg, step_stage;  // segments / staging of the one download after a device-resident Adam step
  float *step_host = nullptr;      // its pinned host image
  bool tape_ps = true;          // RN_POTGNN_TAPE_PS: taped float32 runs on the role-specialised EdgeBlock / atom-owning NodeBlock
  bool mfma_f16 = true;  // fused kernels: split-f16 MFMA products are in use (requested and inside the safe range)
  bool mfma_f16_requested = true;   // RN_POTGNN_MFMA=f32 at create time: exact-f32 MFMA everywhere
  bool mfma_range_fallback = false; // split-f16 was requested but the range guard (mfma_f16_range_ok) refused it
  Graph g{};
  DeviceBuf g_ints;
  DeviceBuf ps_fail;  // [1] int: set by edge_block_ps_kernel when one of its bounded waits ran out
  double lattice[9], mean[9], stdv[9];
  DeviceBuf d_mean_std;  // [18] double
  std::vector<float> packed;  // host packed weights (float master copy)
  PackedLayout lay;
  Precision<float> f32;
  Precision<double> f64;
  // cached I/O staging for the host entry points
  DeviceBuf io_pos, io_alpha, io_vec6, io_lat, io_types;
  // pipelined host entry (rn_potgnn_calc_polarizabilities_async): two staging slots
  struct Slot {
    DeviceBuf pos, alpha;
    hipEvent_t copied = nullptr, done = nullptr;
    bool busy = false;
  } slots[2];
  hipStream_t copy_stream = nullptr, exec_stream = nullptr;
  int next_slot = 0;
  // host entry rn_potgnn_calc_polarizabilities: two page-locked buffers the caller's float64 positions are cast into
  // (float32) piece by piece, each with the event of its host-to-device copy
  struct HostStage {
    float *pin[2] = {nullptr, nullptr};
    size_t elems = 0;  // floats per buffer
    hipEvent_t copied[2] = {nullptr, nullptr};
    hipEvent_t done = nullptr;
    // The float32 positions on the device.  Only staged_forward writes them (behind `done`): a to-device call returns
    // with kernels that still read them, and the other host entries fill io_pos from the null stream, which does not
    // wait for the handle's non-blocking streams.
    DeviceBuf pos;
    DeviceBuf lat;  // the float32 lattices of a variable-cell call [S][9], under the same rules
    hipEvent_t caller = nullptr;  // the to-device entry: the caller's stream up to the call
    char *out_pin = nullptr;  // the result (+ the EdgeBlock's time-out word) of the synchronous host entry
    size_t out_bytes = 0;
  } hstage;
  int last_chunk_structs = 0;
  int train_S = 0;  // frames of the pending train_forward (0 = none)
  int train_prec = 4;  // sizeof of the precision it ran in
  bool train_lat = false, train_types = false;  // it ran with per-sample lattices / atom types (io_lat / io_types)
  bool tape_fused = true;
  // device-resident optimisation (rn_potgnn_adam_step): gradients stay in f32.grad, Adam moments and
  // the trainable mask live next to the weights; the host copy `packed` is refreshed on demand
  bool device_training = false;  // BatchNorm running statistics are updated on the device
  bool grads_on_device = false;  // f32.grad holds the gradients of the last backward
  bool host_stale = false;       // the device weights are ahead of `packed`
  DeviceBuf adam_m, adam_v, trainable_mask, derived_ops;
  int num_derived_ops = 0, derived_first_stage = 0;  // (ops after the first stage read what it wrote: second launch)
  double bn_count = 0;  // rows the pending step's BatchNorm statistics cover (all ranks)
  rn_potgnn_reduce_fn reducer = nullptr;  // data-parallel training: sums doubles over ranks
  void *reducer_ctx = nullptr;
  bool last_was_f64 = false;
  bool last_in_order = false;  // the last run kept its edge rows in (b, a) order (narrow kernels)
  // profiling
  int profiling = 0;
  std::vector<TimedLaunch> timed;
  double k_ms[K_COUNT] = {0};
  int64_t k_launches[K_COUNT] = {0};
  std::string error;
  hipEvent_t ev_start = nullptr;
  hipEvent_t ev_g[2] = {nullptr, nullptr};  // "projection stage done" per lane (run_pair)
  bool interleave = true;
  // atom-group contractions: the CSR permutation of the last labels (perm [N] | gptr [G+1]), Jacobian rows, staging
  GroupTable groups;
  DeviceBuf grp_jac, grp_disp, grp_out;
  DeviceBuf mode_vectors;  // rn_potgnn_mode_increments_device: D [M][N][3] | P [M][N][3]
  // variable-cell calls: the lattice rows of the Jacobian [frames][6][9], a trajectory's lattices in the arithmetic of a
  // float32 run (group increments), the float32 lattices of rn_potgnn_forward_cells_device
  DeviceBuf grp_jl, grp_lat, cells_lat;
  int device_index() const { return cfg.device; }
  static std::string &create_error() { return g_create_error; }
};

namespace {

// Frames per device work chunk in precision T.  The workspace budget is counted in bytes, so
// the float64 lanes (created on first use, next to the float32 ones) take half the frames.
bool lean_workspace(const rn_potgnn *h);
size_t per_structure_elems(const rn_potgnn *h, bool lean);
// The float32 chunk may have been sized from the LEAN workspace of the fused / narrow pipelines; float64 always runs the
// unfused chain on the full-width buffers, so its chunk is counted from that layout (8 bytes per element) against its own
// allowance (rn_potgnn::f64_budget; with an explicit chunk: the bytes the float32 lanes were given).
template <typename T>
int chunk_frames(const rn_potgnn *h) {
  if (sizeof(T) == 4) return h->chunk;
  const size_t budget = std::max(h->f64_budget, (size_t)h->chunk * per_structure_elems(h, lean_workspace(h)) * sizeof(float));
  const size_t per64 = per_structure_elems(h, false) * sizeof(double);
  return (int)std::max<size_t>(1, std::min<size_t>((size_t)h->chunk, budget / std::max<size_t>(per64, 1)));
}

template <typename T>
Precision<T> &prec(rn_potgnn *h);
template <>
Precision<float> &prec<float>(rn_potgnn *h) { return h->f32; }
template <>
Precision<double> &prec<double>(rn_potgnn *h) { return h->f64; }

// Sum `n` device doubles over the ranks of a data-parallel training run (no-op without a reducer).
void reduce_over_ranks(rn_potgnn *h, double *dev, size_t n, hipStream_t st) {
  if (!h->reducer) return;
  std::vector<double> host(n);
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipMemcpy(host.data(), dev, n * sizeof(double), hipMemcpyDeviceToHost));
  if (h->reducer(host.data(), (int64_t)n, h->reducer_ctx) != 0)
    throw HipError{hipErrorUnknown, "the statistics reducer (data-parallel training) failed"};
  HIP_TRY(hipMemcpy(dev, host.data(), n * sizeof(double), hipMemcpyHostToDevice));
}

// The fused and the narrow pipelines keep no per-edge projection in HBM: of the two projection buffers only
// the [S*E, 32] readout output (bufA) is left.  Taped runs (training, Jacobian) size the full-width buffers
// for their own, much smaller, batch (ensure_tape).
bool lean_workspace(const rn_potgnn *h) {
  return (h->plan.use_fused && h->plan.use_node_fused && h->plan.use_readout_fused) || h->plan.use_narrow;
}
size_t bufA_width(const rn_potgnn *h, bool lean) {
  return lean ? 32 : std::max<size_t>(std::max(2 * h->d.FnP, 2 * h->d.FeP), 32);
}
// The pair kernel's rows [S, NP, FeP] go into the readout's buffer bufA, which nothing touches before the readout: they fit
// when NP <= E / 2 at FeP = 64 (every edge has its reverse, as in a radius graph), so the workspace and the frames per
// launch stay what they were.  A graph with unpaired edges beyond that keeps c2 inside the EdgeBlock.
bool c2_rows_fit(const rn_potgnn *h) {
  return edge_ps_takes_c2_rows(h->g, true, h->mfma_f16) &&
         (size_t)h->g.NP * h->d.FeP <= (size_t)h->g.E * bufA_width(h, lean_workspace(h));
}
size_t per_structure_elems(const rn_potgnn *h, bool lean) {
  const size_t N = h->cfg.num_atoms, E = h->cfg.num_edges;
  const size_t FnP = h->d.FnP, FeP = h->d.FeP;
  return E * 4 + 2 * N * FnP + 2 * E * FeP + N * 2 * FnP + N * 6 * FeP + E * bufA_width(h, lean) +
         (lean ? 0 : E * 4 * FeP);
}

void refresh_mfma_mode(rn_potgnn *h) {
  const bool ok = mfma_f16_range_ok(h->lay, h->packed.data(), h->host_stale);
  h->mfma_f16 = h->mfma_f16_requested && ok;
  h->mfma_range_fallback = h->mfma_f16_requested && !ok;
}

// Per pass: may the EdgeBlock's triplet loop fold c3_norm_1's scale into its operands and
// drop the gate's overflow clamp (edge_agg_kernel, FASTG; folded_gate_ok decides from the weights)?
template <typename T>
void refresh_pass_flags(rn_potgnn *h) {
  Precision<T> &P = prec<T>(h);
  const bool off = getenv("RN_POTGNN_NO_FASTG") && atoi(getenv("RN_POTGNN_NO_FASTG")) != 0;
  for (size_t p = 0; p < h->lay.pass.size() && p < P.pass.size(); ++p) {
    const bool ok = !off && folded_gate_ok(h->lay, h->packed.data(), (int)p);
    // bit 0: fused EdgeBlock kernel; bit 1: unfused edge_agg_kernel -- there only with a
    // single lane: its 170 registers per lane shut the other lane's projection workgroups
    // out of the CU (150 do not), which costs more than the shorter loop gains
    P.pass[p].c3_fast = ok ? (h->plan.num_lanes == 1 ? 3 : 1) : 0;
  }
}

// ensure + a blocking host-to-device copy
template <typename T>
T *stage(DeviceBuf &buf, const void *host, size_t bytes) {
  buf.ensure(bytes);
  HIP_TRY(hipMemcpy(buf.p, host, bytes, hipMemcpyHostToDevice));
  return buf.as<T>();
}

template <typename T>
T *upload_packed(rn_potgnn *h) {  // the host master copy, in T, into the precision's weight blob
  const std::vector<T> host(h->packed.begin(), h->packed.end());
  return stage<T>(prec<T>(h).weights, host.data(), host.size() * sizeof(T));
}

// the frame-independent device precompute (node table, folded readout BatchNorm) on the weight blob `w`
template <typename T>
void device_setup(rn_potgnn *h, T *w, hipStream_t st) {
  const PackedLayout &L = h->lay;
  launch_setup<T>(w + L.emb, w + L.W2, w + L.b2, w + L.W4, w + L.b4, h->cfg.num_atom_types, h->d,
                  w + L.node_table, w + L.b0, w + L.bn_w, w + L.bn_b, w + L.bn_rm, w + L.bn_rv,
                  w + L.scale0, w + L.shift0, st);
}

template <typename T>
void upload_weights(rn_potgnn *h) {  // (re)upload the packed weights and redo the device precompute
  Precision<T> &P = prec<T>(h);
  device_setup<T>(h, upload_packed<T>(h), P.lanes[0].stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(P.lanes[0].stream));
  refresh_pass_flags<T>(h);
}

template <typename T>
void ensure_precision(rn_potgnn *h) {
  Precision<T> &P = prec<T>(h);
  if (P.ready) return;
  const PackedLayout &L = h->lay;
  T *w = upload_packed<T>(h);
  T lat[9];
  for (int i = 0; i < 9; ++i) lat[i] = (T)h->lattice[i];
  stage<T>(P.lattice, lat, sizeof(lat));
  WeightViews<T> v = bind_weights<T>(L, w);
  P.pass = std::move(v.pass);
  refresh_pass_flags<T>(h);
  P.ro = v.ro;
  P.offsets = v.offsets;
  P.node_table = v.node_table;
  P.ones = v.ones;

  const size_t N = h->cfg.num_atoms, E = h->cfg.num_edges, S = chunk_frames<T>(h);
  const size_t FnP = h->d.FnP, FeP = h->d.FeP;
  const bool lean = sizeof(T) == 4 && lean_workspace(h);
  const size_t bufA = bufA_width(h, lean);
  for (int l = 0; l < h->plan.num_lanes; ++l) {
    Lane<T> &ln = P.lanes[l];
    HIP_TRY(hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&ln.done, hipEventDisableTiming));
    ln.unit4.ensure(S * E * 4 * sizeof(T));
    for (int i = 0; i < 2; ++i) {
      ln.node[i].ensure(S * N * FnP * sizeof(T));
      ln.edge[i].ensure(S * E * FeP * sizeof(T));
    }
    ln.npc1.ensure(S * N * 2 * FnP * sizeof(T));
    ln.np3.ensure(S * N * 6 * FeP * sizeof(T));
    ln.bufA.ensure(S * E * bufA * sizeof(T));
    if (!lean) ln.bufB.ensure(S * E * 4 * FeP * sizeof(T));
  }
  if (h->keep_stages || h->snap_pairs) {
    const int np = h->cfg.num_message_passes + 1;
    P.snap_node.resize(np);
    P.snap_edge.resize(np);
    for (int i = 0; i < np; ++i) {
      P.snap_node[i].ensure(S * N * FnP * sizeof(T));
      P.snap_edge[i].ensure(S * E * FeP * sizeof(T));
    }
  }
  device_setup<T>(h, w, P.lanes[0].stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(P.lanes[0].stream));
  P.ready = true;
}

struct Timer {
  rn_potgnn *h;
  hipStream_t st;
  int kid;
  hipEvent_t a = nullptr, b = nullptr;
  bool on;
  Timer(rn_potgnn *h_, hipStream_t st_, int kid_) : h(h_), st(st_), kid(kid_) {
    // 1 = every kernel, 100 + k = kernel k only, 1000 + mask = the kernels whose bit is set
    on = h->profiling == 1 || (h->profiling >= 100 && h->profiling < 1000 && h->profiling - 100 == kid) ||
         (h->profiling >= 1000 && (((h->profiling - 1000) >> kid) & 1));
    if (on) {
      HIP_TRY(hipEventCreate(&a));
      HIP_TRY(hipEventCreate(&b));
      HIP_TRY(hipEventRecord(a, st));
    }
  }
  ~Timer() noexcept(false) {
    if (on) {
      (void)hipEventRecord(b, st);
      h->timed.push_back({kid, a, b});
    }
    if (h->debug_sync) {
      hipError_t e = hipGetLastError();
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (e != hipSuccess) throw HipError{e, kKernelNames[kid]};
    }
  }
};

void resolve_timers(rn_potgnn *h) {
  for (auto &t : h->timed) {
    float ms = 0;
    if (hipEventSynchronize(t.b) == hipSuccess && hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) {
      h->k_ms[t.kid] += ms;
      h->k_launches[t.kid] += 1;
    }
    (void)hipEventDestroy(t.a);
    (void)hipEventDestroy(t.b);
  }
  h->timed.clear();
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
  ForwardIO at(int64_t first, int N) const {  // the frames from `first` on: the one place that knows the strides
    auto from = [first](auto *p, int64_t stride) { return p ? p + first * stride : nullptr; };
    ForwardIO o;
    o.pos = from(pos, 3 * (int64_t)N);
    o.pos32 = from(pos32, 3 * (int64_t)N);
    o.alpha = from(alpha, 9);
    o.vec6 = from(vec6, 6);
    o.alpha_raw = from(alpha_raw, 9);
    o.lat = from(lat, 9);
    o.types = from(types, N);
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
  int cur = 0;
  T *node[2], *edge[2], *unit4, *npc1, *np3, *bufA, *bufB;
  int64_t MN, ME;

  ChunkRun(rn_potgnn *h_, Lane<T> &l, const ForwardIO<T> &io_, int S_) : h(h_), ln(&l), io(io_), S(S_) {
    node[0] = l.node[0].template as<T>();
    node[1] = l.node[1].template as<T>();
    edge[0] = l.edge[0].template as<T>();
    edge[1] = l.edge[1].template as<T>();
    unit4 = l.unit4.template as<T>();
    npc1 = l.npc1.template as<T>();
    np3 = l.np3.template as<T>();
    bufA = l.bufA.template as<T>();
    bufB = l.bufB.template as<T>();
    MN = (int64_t)S * h->g.N;
    ME = (int64_t)S * h->g.E;
  }
  hipStream_t st() const { return ln->stream; }
  // With the tape on, the embeddings after pass p are written straight into tape slot p+1 (the
  // ping-pong pair is re-pointed pass by pass), so recording costs no copies.
  void target_tape(int slot, int which) {
    Precision<T> &P = prec<T>(h);
    if (!P.tape_on) return;
    node[which] = P.tape_node[slot].template as<T>();
    edge[which] = P.tape_edge[slot].template as<T>();
  }
  void snapshot(int p) {
    Precision<T> &P = prec<T>(h);
    if (!h->keep_stages && !h->snap_pairs) return;
    HIP_TRY(hipMemcpyAsync(P.snap_node[p].p, node[cur], (size_t)MN * h->d.FnP * sizeof(T),
                           hipMemcpyDeviceToDevice, st()));
    HIP_TRY(hipMemcpyAsync(P.snap_edge[p].p, edge[cur], (size_t)ME * h->d.FeP * sizeof(T),
                           hipMemcpyDeviceToDevice, st()));
  }

  // geometry + radial basis, initial node embedding
  void begin() {
    Precision<T> &P = prec<T>(h);
    target_tape(0, 0);
    {
      Timer t(h, st(), K_GEOM);
      bool done = false;
      const T *lat = io.lat ? io.lat : P.lattice.template as<T>();
      const int lat_stride = io.lat ? 9 : 0;
      const T gauss = (T)h->cfg.gauss_coefficient;
      if constexpr (sizeof(T) == 4) {
        if (io.pos32) {
          if (pair_rows()) launch_geom_rbf_pairs_pos32(io.pos32, S, h->g, lat, lat_stride, P.offsets, gauss, h->d, unit4, edge[0], st());
          else launch_geom_rbf_pos32(io.pos32, S, h->g, lat, lat_stride, P.offsets, gauss, h->d, unit4, edge[0], st(), narrow());
          done = true;
        } else if (pair_rows()) {
          launch_geom_rbf_pairs(io.pos, S, h->g, lat, lat_stride, P.offsets, gauss, h->d, unit4, edge[0], st());
          done = true;
        }
      }
      if (!done) launch_geom_rbf<T>(io.pos, S, h->g, lat, lat_stride, P.offsets, gauss, h->d, unit4, edge[0], st(), narrow());
      h->last_in_order = narrow();  // (kernels_narrow.hip: edge rows in (b, a) order; rn_potgnn_debug_stage undoes it)
      h->last_pair_rows = pair_rows();
    }
    {
      Timer t(h, st(), K_NODE_INIT);
      launch_node_init<T>(P.node_table, S, h->g, h->d, node[0], io.types, st());
    }
    cur = 0;
    snapshot(0);
  }

  // begin + every pass: what is left is finish(), or the reverse pass over the tape
  void run_stages() {
    begin();
    for (int p = 0; p < h->cfg.num_message_passes; ++p) {
      stage_project(p);
      stage_aggregate(p);
    }
  }

  // Y[R rows] = X W (+ bias): float32 with the split-f16 products enabled -> rowgemm_split_kernel where it serves the shape
  // (K a multiple of 64), else the exact-f32 MFMA projection kernel
  void project(const T *X, int64_t R, int K, const T *WT, int NOUT, T *Y, const T *bias, int amode, const T *nd) {
    if constexpr (sizeof(T) == 4) {
      if (h->mfma_f16 && h->split_projections &&
          launch_rowgemm_split(X, K, K, R, WT, NOUT, Y, false, bias, amode, nd, h->g, st()))
        return;
    }
    launch_rowgemm<T>(X, R, K, WT, NOUT, Y, nullptr, bias, false, amode, nd, h->g, st());
  }

  // "G" stage of pass p: NodeBlock + every dense projection the EdgeBlock needs
  // (matrix pipe / HBM bound)
  void stage_project(int p) {
    const PassW<T> &w = prec<T>(h).pass[p];
    const Graph &g = h->g;
    const Dims d = h->d;
    const int nxt = cur ^ 1;
    target_tape(p + 1, nxt);
    if constexpr (sizeof(T) == 4) {
      if (narrow()) {  // the whole NodeBlock, projections included, in one launch
        Timer t(h, st(), K_NODE_AGG);
        launch_node_narrow(edge[cur], node[cur], node[nxt], S, g, d, w, st());
        return;
      }
    }
    {
      Timer t(h, st(), K_PROJ_NODE);
      if (node_centred()) project(node[cur], MN, d.FnP, w.c1_WnT_c, 2 * d.FnP, npc1, w.c1_bias_c, 0, nullptr);  // zero row mean
      else project(node[cur], MN, d.FnP, w.c1_WnT, 2 * d.FnP, npc1, w.c1_bias, 0, nullptr);
    }
    bool node_fused = false;
    if constexpr (sizeof(T) == 4) {
      if (fused() && h->plan.use_node_fused) {  // c1 edge projection + aggregation in one launch
        Timer t(h, st(), K_NODE_AGG);
        if (node_centred() && g.na_num > 0) launch_node_atom(edge[cur], node[cur], npc1, node[nxt], S, g, d, w, st(), pair_rows());
        else launch_node_fused(edge[cur], node[cur], npc1, node[nxt], S, g, d, w, h->mfma_f16, node_centred(), st());
        node_fused = true;
      }
    }
    if (!node_fused) {
      {
        Timer t(h, st(), K_PROJ_EDGE_C1);
        project(edge[cur], ME, d.FeP, w.c1_WeT, 2 * d.FnP, bufA, nullptr, 0, nullptr);
      }
      {
        Timer t(h, st(), K_NODE_AGG);
        launch_node_agg<T>(npc1, bufA, node[cur], node[nxt], S, g, d, w, st());
      }
    }
    {  // EdgeBlock uses the UPDATED node embedding (_gnn.py:649-650)
      Timer t(h, st(), K_PROJ_NODE);
      if (role_split(w)) project(node[nxt], MN, d.FnP, w.c3_WnT_c, 6 * d.FeP, np3, w.c3_nshift_c, 0, nullptr);  // zero row mean
      else project(node[nxt], MN, d.FnP, w.c3_WnT, 6 * d.FeP, np3, w.c3_nshift, 0, nullptr);
    }
    if (!fused()) {
      {
        Timer t(h, st(), K_PROJ_EDGE_C3);
        project(edge[cur], ME, d.FeP, w.c3_WeT, 4 * d.FeP, bufB, nullptr, 0, nullptr);
      }
      {
        Timer t(h, st(), K_PROJ_C2);
        project(nullptr, ME, d.FnP, w.c2_WT, 2 * d.FeP, bufA, w.c2_bias, 1, node[nxt]);
      }
    }
  }

  // "V" stage of pass p: triplet aggregation of the EdgeBlock (VALU bound)
  void stage_aggregate(int p) {
    const PassW<T> &w = prec<T>(h).pass[p];
    const int nxt = cur ^ 1;
    const float *c2_rows = nullptr;
    if constexpr (sizeof(T) == 4) {
      if (c2_pairs(w)) {  // the c2 branch once per atom pair, into the readout's buffer (idle until finish())
        Timer t(h, st(), K_C2_PAIRS);
        launch_c2_pairs(node[nxt], bufA, S, h->g, h->d, w, st());
        c2_rows = bufA;
      }
    }
    {
      Timer t(h, st(), K_EDGE_AGG);
      if constexpr (sizeof(T) == 4) {
        if (narrow()) launch_edge_narrow(edge[cur], edge[nxt], node[nxt], S, h->g, h->d, w, st());
        else if (role_split(w)) launch_edge_ps(edge[cur], edge[nxt], node[nxt], np3, tape_agg(p), S, h->g, h->d, w, h->ps_fail.as<int>(), st(), pair_rows(), h->mfma_f16, c2_rows);
        else if (fused()) edge_unfused_in_blocks(p);
        else HIP_TRY(launch_edge_agg<T>(bufB, np3, bufA, edge[cur], edge[nxt], S, h->g, h->d, w, tape_agg(p), st()));
      } else {
        HIP_TRY(launch_edge_agg<T>(bufB, np3, bufA, edge[cur], edge[nxt], S, h->g, h->d, w, tape_agg(p), st()));
      }
    }
    cur = nxt;
    snapshot(p + 1);
  }

  // A pass of the FUSED pipeline that the role-specialised EdgeBlock does not serve (a graph its ring refuses, a pass
  // without the folded gate scale, exact-f32 products, RN_POTGNN_EDGE_PS=0 / RN_POTGNN_TAPE_PS=0): the unfused EdgeBlock --
  // the two per-edge projections + edge_agg_kernel, what the float64 instantiation always runs -- block of frames by block
  // of frames, because the fused pipeline's lean workspace holds no per-edge projection buffers (6 FeP floats per edge).
  // Through round 4 these passes took the per-frame fused kernel (retired; see profiles/r04/mfma_k32.txt and git history).
  void edge_unfused_in_blocks(int p) {
    const PassW<T> &w = prec<T>(h).pass[p];
    const Graph &g = h->g;
    const Dims d = h->d;
    const int nxt = cur ^ 1;
    const size_t per_frame = (size_t)g.E * (size_t)(6 * d.FeP) * sizeof(T);
    int block = (int)std::max<size_t>(1, std::min<size_t>((size_t)S, ((size_t)1 << 30) / std::max<size_t>(per_frame, 1)));
    if (const char *e = getenv("RN_POTGNN_UNFUSED_BLOCK_FRAMES")) block = std::max(1, std::min(block, atoi(e)));  // test knob: several blocks on a small batch
    ln->fbA.ensure((size_t)block * g.E * 2 * d.FeP * sizeof(T));
    ln->fbB.ensure((size_t)block * g.E * 4 * d.FeP * sizeof(T));
    T *fa = ln->fbA.template as<T>(), *fb = ln->fbB.template as<T>();
    T *agg = tape_agg(p);
    for (int s0 = 0; s0 < S; s0 += block) {
      const int sb = std::min(block, S - s0);
      const int64_t rows = (int64_t)sb * g.E;
      const T *e_in = edge[cur] + (size_t)s0 * g.E * d.FeP, *nd = node[nxt] + (size_t)s0 * g.N * d.FnP;
      project(e_in, rows, d.FeP, w.c3_WeT, 4 * d.FeP, fb, nullptr, 0, nullptr);
      project(nullptr, rows, d.FnP, w.c2_WT, 2 * d.FeP, fa, w.c2_bias, 1, nd);
      HIP_TRY(launch_edge_agg<T>(fb, np3 + (size_t)s0 * g.N * 6 * d.FeP, fa, e_in, edge[nxt] + (size_t)s0 * g.E * d.FeP, sb, g, d, w,
                                 agg ? agg + (size_t)s0 * g.E * d.FeP : nullptr, st()));
    }
  }

  // readout MLP (_gnn.py:532-539): bufA <- ssp(BN(L0 edge)), bufB <- ssp(L3 .), bufA <- L5 .
  void finish() {
    Precision<T> &P = prec<T>(h);
    const Graph &g = h->g;
    const Dims d = h->d;
    if constexpr (sizeof(T) == 4) {
      if (narrow()) {  // readout MLP + edge tensors + per-frame mean in one launch
        Timer t(h, st(), K_READOUT_MLP);
        const double *ms = h->d_mean_std.as<double>();
        launch_readout_narrow(edge[cur], unit4, S, g, d, P.ro, ms, ms + 9, io.vec6, io.alpha, io.alpha_raw,
                              h->keep_stages ? bufA : nullptr, st());
        HIP_TRY(hipGetLastError());
        return;
      }
    }
    int pol_stride = 32;
    {
      Timer t(h, st(), K_READOUT_MLP);
      const int HP = std::max(d.FeP, 32);
      bool done = false;
      if constexpr (sizeof(T) == 4) {
        if (fused() && h->plan.use_readout_fused) {  // the three layers in one launch; whole 64-byte rows of the 16 columns it writes
          pol_stride = h->keep_stages ? 32 : 16;  // (the stage snapshots read the unfused chain's 32-column layout)
          launch_readout_fused(edge[cur], ME, P.ro, bufA, h->mfma_f16, st(), pair_rows(), pol_stride);
          done = true;
        }
      }
      if (!done) {
        launch_rowgemm<T>(edge[cur], ME, d.FeP, P.ro.W0T, HP, bufA, P.ro.scale0, P.ro.shift0, true, 0,
                          nullptr, g, st());
        launch_rowgemm<T>(bufA, ME, HP, P.ro.W3T, HP, bufB, P.ones, P.ro.b3, true, 0, nullptr, g, st());
        launch_rowgemm<T>(bufB, ME, HP, P.ro.W5T, 32, bufA, nullptr, P.ro.b5, false, 0, nullptr, g,
                          st());
      }
    }
    {
      Timer t(h, st(), K_READOUT_REDUCE);
      const double *ms = h->d_mean_std.as<double>();
      launch_readout_reduce<T>(bufA, unit4, S, g, ms, ms + 9, io.vec6, io.alpha, io.alpha_raw, st(), pol_stride);
    }
    HIP_TRY(hipGetLastError());
  }
  // (the fused kernels also serve taped float32 runs: the EdgeBlock kernel records the one extra
  //  array the reverse pass needs; RN_POTGNN_TAPE_FUSED=0 keeps those runs on the unfused kernels)
  bool fused() const { return sizeof(T) == 4 && h->plan.use_fused && (!prec<T>(h).tape_on || h->tape_fused); }
  bool narrow() const { return sizeof(T) == 4 && h->plan.use_narrow && !prec<T>(h).tape_on; }
  // the fused NodeBlock on the centred copy of c1_linear (evaluation runs, split-f16 products)
  bool node_centred() const {
    static const bool on = !(getenv("RN_POTGNN_NODE_CENTRED") && atoi(getenv("RN_POTGNN_NODE_CENTRED")) == 0);
    return sizeof(T) == 4 && on && fused() && h->plan.use_node_fused && h->mfma_f16 && (!prec<T>(h).tape_on || h->tape_ps);
  }
  // the role-specialised EdgeBlock (kernels_edge_ps.hip): split-f16 products and the folded gate scale only.  Taped runs
  // take it too (round 4: it records the pre-LayerNorm sums like the per-frame kernel, and the reverse pass recomputes
  // every projection from the taped node / edge rows, so it never sees the centred copies); RN_POTGNN_TAPE_PS=0 keeps
  // them on the per-frame kernel and the row-ordered NodeBlock
  bool role_split(const PassW<T> &w) const {
    // (round 5: also with exact-f32 products -- RN_POTGNN_MFMA=f32, the range guard's fallback -- on the kernel's F16 = false form)
    return sizeof(T) == 4 && fused() && h->plan.use_ps && (w.c3_fast & 1) != 0 && (!prec<T>(h).tape_on || h->tape_ps);
  }
  // Edge rows as split-f16 pairs (kernels.hpp: launch_geom_rbf_pairs): when EVERY kernel that touches them in this run is one
  // that speaks the format -- the role-specialised EdgeBlock in every pass, the atom-owning NodeBlock, the fused readout --
  // and nothing else looks at them (no tape, no stage snapshots).  RN_POTGNN_PAIR_ROWS=0 keeps plain float32 rows.
  bool pair_rows() const {
    if (sizeof(T) != 4 || !h->want_pair_rows || h->keep_stages || prec<T>(h).tape_on || !node_centred() || h->g.na_num <= 0 || !h->plan.use_readout_fused) return false;
    for (const auto &w : prec<T>(h).pass)
      if (!role_split(w)) return false;
    return true;
  }
  // The EdgeBlock's c2 branch once per atom pair in a kernel of its own (kernels_c2_pairs.hip) instead of once per edge inside
  // the role-specialised EdgeBlock: evaluation runs on pair rows with split-f16 products, on a graph whose pair rows fit the
  // readout's buffer (c2_rows_fit).  Every other run keeps c2 inside the EdgeBlock.  RN_POTGNN_C2_PAIRS=0 at create time:
  // always.  (rn_potgnn_config_flags bit 11 reports the choice.)
  bool c2_pairs(const PassW<T> &w) const {
    if (sizeof(T) != 4 || !h->want_c2_pairs || !role_split(w) || !pair_rows()) return false;
    return c2_rows_fit(h);
  }
  T *tape_agg(int p) {  // where the EdgeBlock's pre-LayerNorm sums are recorded (taped runs only)
    Precision<T> &P = prec<T>(h);
    return P.tape_on ? P.tape_agg[p].template as<T>() : nullptr;
  }
};

template <typename T>
void run_chunk(ChunkRun<T> c) {
  c.run_stages();
  c.finish();
}

// Two chunks A, B on the two lanes with their stages forced to alternate:
//   lane A:  G_A(0)  V_A(0)  G_A(1)  V_A(1) ...
//   lane B:          G_B(0)  V_B(0)  G_B(1) ...
// G_B(p) waits for G_A(p) and G_A(p+1) waits for G_B(p), so the two G stages never run
// together while each V stage (VALU-bound triplet loop) has the other chunk's G stage
// (matrix pipe + HBM streams) as its only companion on the chip.
template <typename T>
void run_pair(rn_potgnn *h, ChunkRun<T> &a, ChunkRun<T> &b) {
  const int P = h->cfg.num_message_passes;
  a.begin();
  b.begin();
  for (int p = 0; p < P; ++p) {
    if (p > 0) HIP_TRY(hipStreamWaitEvent(a.st(), h->ev_g[1], 0));  // after G_B(p-1)
    a.stage_project(p);
    HIP_TRY(hipEventRecord(h->ev_g[0], a.st()));
    a.stage_aggregate(p);
    HIP_TRY(hipStreamWaitEvent(b.st(), h->ev_g[0], 0));             // after G_A(p)
    b.stage_project(p);
    HIP_TRY(hipEventRecord(h->ev_g[1], b.st()));
    b.stage_aggregate(p);
  }
  a.finish();
  b.finish();
}

// The role-specialised EdgeBlock bounds its spin waits: a wait that runs out sets a word in HBM (and poisons the rows the
// workgroup stores from then on with NaN) instead of hanging the GPU.  Every entry point that synchronises with the device
// anyway looks at the word here, right after its synchronisation -- evaluation, the pipelined host entry's rn_potgnn_wait,
// the taped forward / backward of a training step, the Jacobian, the Adam step -- and clears it, so a timeout is reported by
// the call it happened in (or the first synchronising call behind it), never by an unrelated later one.  Entry points that do
// not synchronise (device buffers with synchronize = 0) hand back NaN rows in that case.
void check_ps_fail(rn_potgnn *h) {
  if (!h->plan.use_ps || !h->ps_fail.p) return;
  int fail = 0;
  HIP_TRY(hipMemcpy(&fail, h->ps_fail.p, sizeof(int), hipMemcpyDeviceToHost));
#ifdef RN_PS_TIMING
  {
    long long t[40];
    HIP_TRY(hipMemcpy(t, (const char *)h->ps_fail.p + 64, sizeof(t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset((char *)h->ps_fail.p + 64, 0, sizeof(t)));
    static const char *names[20] = {"P sched+dma_wait", "P loads+split", "P split sync", "P seeds", "P request", "P guard",
                                    "P P'+c2", "P Q' (product, loads landed + finish)", "P norm sync+publish", "P ring guard", "C ready wait", "C prologue", "C loop",
                                    "C epilogue+done", "", "", "C(set B) ready wait", "C(set B) prologue", "C(set B) loop", "C(set B) epilogue+done"};
    for (int i = 0; i < 20; ++i)
      if (t[2 * i + 1]) fprintf(stderr, "[ps timing] %-22s %10.1f cycles x %lld\n", names[i], (double)t[2 * i] / (double)t[2 * i + 1], t[2 * i + 1]);
  }
#endif
#ifdef RN_PS_GRAM_DEBUG
  {
    int cnt = 0;
    HIP_TRY(hipMemcpy(&cnt, (const char *)h->ps_fail.p + 127 * 4, sizeof(int), hipMemcpyDeviceToHost));
    float dbg[144];
    HIP_TRY(hipMemcpy(dbg, (const char *)h->ps_fail.p + 128 * 4, sizeof(dbg), hipMemcpyDeviceToHost));
    fprintf(stderr, "[gram debug] %d mismatches\n", cnt);
    for (int k = 0; k < std::min(cnt, 12); ++k)
      fprintf(stderr, "  ref %g tab %g parts %g %g %g %g  d %g er %g tl %g urow %g r %g gr %g\n", dbg[12 * k], dbg[12 * k + 1], dbg[12 * k + 2],
              dbg[12 * k + 3], dbg[12 * k + 4], dbg[12 * k + 5], dbg[12 * k + 6], dbg[12 * k + 7], dbg[12 * k + 8], dbg[12 * k + 9],
              dbg[12 * k + 10], dbg[12 * k + 11]);
    HIP_TRY(hipMemset((char *)h->ps_fail.p + 127 * 4, 0, 4 + sizeof(dbg)));
  }
#endif
  if (fail == 0) return;
  HIP_TRY(hipMemset(h->ps_fail.p, 0, sizeof(int)));
  // (which wait: 1 = the producers' split sync, 2 = a producer waiting for round g - 2's P' / c2 rows to be taken,
  //  3 = a producer waiting for round g - back - 1 to be finished, 4 = a consumer waiting for its round,
  //  6 = a consumer waiting for the earlier arrivals of its round parity before it adds its own to c_rd)
  static const char *const which[7] = {
      "role-specialised EdgeBlock: a wait between producer and consumer waves timed out",
      "role-specialised EdgeBlock: the producers' split sync timed out",
      "role-specialised EdgeBlock: a producer's wait for the consumers to take the rows of an earlier round timed out",
      "role-specialised EdgeBlock: a producer's wait for the consumers to finish an earlier round (ring rows) timed out",
      "role-specialised EdgeBlock: a consumer's wait for its round timed out",
      "role-specialised EdgeBlock: a wait between producer and consumer waves timed out",
      "role-specialised EdgeBlock: a consumer's round-ordered wait before releasing its ring rows (c_rd) timed out"};
  throw HipError{hipErrorLaunchFailure, which[fail >= 0 && fail <= 6 ? fail : 0]};
}

// The bracket around work the handle's lanes do for a caller's stream.  behind_caller: the first `n` lanes start behind
// what `user` holds so far.  hand_back: `user` continues behind what they hold now; with `sync` it is synchronised and the
// EdgeBlock's time-out word is read (an evaluation resolves its kernel timers there too: `timers`).
template <typename T>
void behind_caller(rn_potgnn *h, hipStream_t user, Lane<T> *lanes, int n) {
  HIP_TRY(hipEventRecord(h->ev_start, user));
  for (int l = 0; l < n; ++l) HIP_TRY(hipStreamWaitEvent(lanes[l].stream, h->ev_start, 0));
}
template <typename T>
void hand_back(rn_potgnn *h, hipStream_t user, Lane<T> *lanes, int n, bool sync, bool timers = false) {
  for (int l = 0; l < n; ++l) {
    HIP_TRY(hipEventRecord(lanes[l].done, lanes[l].stream));
    HIP_TRY(hipStreamWaitEvent(user, lanes[l].done, 0));
  }
  if (!sync) return;
  HIP_TRY(hipStreamSynchronize(user));
  if (timers) resolve_timers(h);
  check_ps_fail(h);
}

template <typename T>
void forward_device(rn_potgnn *h, const ForwardIO<T> &io, int64_t S, hipStream_t user, bool sync) {
  ensure_precision<T>(h);
  Precision<T> &P = prec<T>(h);
  const int N = h->cfg.num_atoms;
  const int lanes = h->plan.num_lanes;
  behind_caller(h, user, P.lanes, lanes);
  auto make = [&](int lane, int64_t first, int s) { return ChunkRun<T>(h, P.lanes[lane], io.at(first, N), s); };
  int64_t done = 0;
  // Work chunks of EQUAL size: as many as the workspace demands, the frames split evenly among them (10 000 frames at a
  // capacity of 2344: five launches of 2000 instead of four of 2344 and one of 624, whose persistent workgroups idle through
  // a tail as long as a full launch's).  Results do not depend on the chunking (bit-identical: tests).
  const int capacity = chunk_frames<T>(h);
  const int64_t pieces = (S + capacity - 1) / capacity;
  const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(capacity, (S + pieces - 1) / std::max<int64_t>(pieces, 1)));
  h->train_S = 0;  // lane 0's workspace is about to be overwritten: a pending train_forward is void
  while (done < S) {
    const int64_t left = S - done;
    if (lanes == 2 && h->interleave && !h->keep_stages && !h->snap_pairs && left > 1) {
      // split what is left of this round evenly over the two lanes
      const int64_t both = std::min<int64_t>(left, 2 * (int64_t)chunk);
      const int sa = (int)((both + 1) / 2), sb = (int)(both - sa);
      ChunkRun<T> a = make(0, done, sa), b = make(1, done + sa, sb);
      run_pair<T>(h, a, b);
      h->last_chunk_structs = sa;
      done += both;
    } else {
      const int s = (int)std::min<int64_t>(chunk, left);
      run_chunk(make(0, done, s));
      h->last_chunk_structs = s;
      done += s;
    }
  }
  h->last_was_f64 = sizeof(T) == 8;
  hand_back(h, user, P.lanes, lanes, sync, true);
}

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

enum { DE0, DE1, DN0, DN1, DNX, DPQ, DNP3, DC2, DPROD, DBC1, DNPC1, DPOL, DUNIT, DH, POL, DOUT, DPROD2, BWN };

template <typename T>
void reverse_pass(rn_potgnn *h, ChunkRun<T> &c, const Reverse<T> &rv) {
  Precision<T> &P = prec<T>(h);
  const PackedLayout &L = h->lay;
  const Graph &g = h->g;
  const Dims d = h->d;
  const int N = g.N, E = g.E, NP = h->cfg.num_message_passes;
  const int S = rv.S, B = rv.B, C = S * B;
  const int HP = std::max(d.FeP, 32);
  hipStream_t st = c.st();
  const size_t ce = (size_t)C * E, cn = (size_t)C * N, fe = (size_t)S * E, fn = (size_t)S * N;
  const size_t sizes[BWN] = {ce * d.FeP, ce * d.FeP, cn * d.FnP, cn * d.FnP, cn * d.FnP,
                             ce * 4 * d.FeP, cn * 6 * d.FeP, ce * std::max(2 * d.FeP, HP), ce * d.FnP,
                             ce * 2 * d.FnP, cn * 2 * d.FnP, ce * 32, ce * 4, ce * HP, fe * 32,
                             (size_t)C * 6, rv.grad ? fe * d.FnP : 0};
  T *b[BWN];
  for (int i = 0; i < BWN; ++i) {
    P.bw[i].ensure(sizes[i] * sizeof(T));
    b[i] = P.bw[i].template as<T>();
  }
  T *bufA = c.bufA, *bufB = c.bufB, *unit4 = c.unit4;
  T *G = rv.grad;
  T *Wd = P.weights.template as<T>();
  // dX[R, K] (+)= dY[R, N] * W^T with W = the forward's [K][N] matrix at `w_off`, its
  // transposed copy at `t_off`: MFMA projection kernel in float32, simple kernel otherwise
  // (float32 with the split-f16 products enabled: rowgemm_split_kernel where the shape allows)
  const bool split_gemm = sizeof(T) == 4 && h->mfma_f16;
  auto back_gemm = [&](const T *dY, int64_t R, int N, size_t w_off, size_t t_off, int K, T *dX,
                       bool accumulate) {
    if constexpr (sizeof(T) == 4) {
      if (split_gemm && launch_rowgemm_split(dY, N, N, R, Wd + t_off, K, dX, accumulate, nullptr, 0, nullptr, g, st)) return;
      if (launch_rowgemm_blocks(dY, N, N, R, Wd + t_off, K, dX, accumulate, g, st)) return;
    }
    launch_gemm_nt<T>(dY, R, N, Wd + w_off, N, K, dX, accumulate, st);
  };
  // Y = X W (+ bias): a recomputed forward projection of the pass
  auto project = [&](const T *X, int64_t R, int K, const T *WT, int NOUT, T *Y, const T *bias, int amode, const T *node) {
    if constexpr (sizeof(T) == 4) {
      if (split_gemm && launch_rowgemm_split(X, K, K, R, WT, NOUT, Y, false, bias, amode, node, g, st)) return;
    }
    launch_rowgemm<T>(X, R, K, WT, NOUT, Y, nullptr, bias, false, amode, node, g, st);
  };

  // weight-gradient products (float32): per-workgroup partial sums into an arena, ONE reduction at the end
  TnDeferred tn_store, *tn = nullptr;
  if constexpr (sizeof(T) == 4) {
    static const bool tn_atomic = getenv("RN_POTGNN_TN_ATOMIC") && atoi(getenv("RN_POTGNN_TN_ATOMIC")) != 0;
    if (G && !tn_atomic) {
      size_t need = tn_partial_elems(ce, HP, 32) + tn_partial_elems(ce, HP, HP) + tn_partial_elems(ce, d.FeP, HP);
      const size_t per_pass = tn_partial_elems(ce, d.FeP, 4 * d.FeP) + tn_partial_elems(cn, d.FnP, 6 * d.FeP) +
                              tn_partial_elems(ce, d.FnP, 2 * d.FeP) + tn_partial_elems(ce, d.FeP, 2 * d.FnP) +
                              tn_partial_elems(cn, d.FnP, 2 * d.FnP);
      need += per_pass * (size_t)NP;
      P.tn_arena.ensure(need * sizeof(float));
      tn_store.arena = P.tn_arena.template as<float>();
      tn_store.capacity = need;
      tn = &tn_store;
    }
  }

  // The weight-gradient products dW^T = X^T dY of a pass hang off the cotangent chain: nothing reads them before the final
  // reduction.  They run on a SIDE stream, ordered behind the kernel that produced their dY and joined before the next pass
  // overwrites it (and before the reduction) -- small latency-bound launches under the chain's small latency-bound launches.
  // (RN_POTGNN_TN_SIDE=0: in line on the chain's stream, as through round 5.)
  static const bool want_side = !(getenv("RN_POTGNN_TN_SIDE") && atoi(getenv("RN_POTGNN_TN_SIDE")) == 0);
  const bool overlap = G != nullptr && sizeof(T) == 4 && want_side;
  hipStream_t sd = st;
  if (overlap) {
    if (!P.side) {
      HIP_TRY(hipStreamCreateWithFlags(&P.side, hipStreamNonBlocking));
      for (auto &e : P.ev_side) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    sd = P.side;
  }
  auto side_after_chain = [&](int which) {  // what the chain has enqueued so far precedes what the side stream gets next
    if (!overlap) return;
    HIP_TRY(hipEventRecord(P.ev_side[which], st));
    HIP_TRY(hipStreamWaitEvent(sd, P.ev_side[which], 0));
  };
  auto chain_after_side = [&]() {  // ... and the other way round
    if (!overlap) return;
    HIP_TRY(hipEventRecord(P.ev_side[2], sd));
    HIP_TRY(hipStreamWaitEvent(st, P.ev_side[2], 0));
  };

  // ---- readout: recompute h1 (bufA), h2 (bufB), pol; then reverse
  const T *edgeP = P.tape_edge[NP].template as<T>();
  if (rv.train_bn) {
    // (the column sums of train_forward are still in bn_stats, already reduced over ranks)
    launch_bn_train_apply<T>(P.tape_z1.template as<T>(), fe, HP, d.Fe, P.bn_stats.template as<double>(),
                             h->bn_count, Wd + L.bn_w, Wd + L.bn_b, bufA, b[DH] /*scratch for mean/var*/, st);
  } else {
    launch_rowgemm<T>(edgeP, fe, d.FeP, P.ro.W0T, HP, bufA, P.ro.scale0, P.ro.shift0, true, 0, nullptr, g, st);
  }
  launch_rowgemm<T>(bufA, fe, HP, P.ro.W3T, HP, bufB, P.ones, P.ro.b3, true, 0, nullptr, g, st);
  launch_rowgemm<T>(bufB, fe, HP, P.ro.W5T, 32, b[POL], nullptr, P.ro.b5, false, 0, nullptr, g, st);
  launch_readout_bwd<T>(rv.d_dout6, b[POL], unit4, C, B, g, b[DPOL], b[DUNIT], st);
  if (G) launch_gemm_tn<T>(bufB, HP, b[DPOL], 32, ce, HP, 32, G + L.W5T, 32, G + L.b5, 0, nullptr, g, st, tn);
  back_gemm(b[DPOL], ce, 32, L.W5T, L.t_W5, HP, b[DH], false);                     // d h2
  launch_ssp_bwd<T>(b[DH], bufB, nullptr, E, HP, C, B, st);                        // d z2
  if (G) launch_gemm_tn<T>(bufA, HP, b[DH], HP, ce, HP, HP, G + L.W3T, HP, G + L.b3, 0, nullptr, g, st, tn);
  back_gemm(b[DH], ce, HP, L.W3T, L.t_W3, HP, b[DC2], false);                      // d h1
  if (rv.train_bn) {
    launch_ssp_bwd<T>(b[DC2], bufA, nullptr, E, HP, C, B, st);                     // d (BN output)
    double *stats = P.bn_stats.template as<double>(), *sums = stats + 2 * HP, *own = stats + 4 * HP;
    launch_bn_bwd_sums<T>(b[DC2], P.tape_z1.template as<T>(), fe, HP, d.Fe, stats, h->bn_count, sums, st);
    HIP_TRY(hipMemcpyAsync(own, sums, sizeof(double) * 2 * HP, hipMemcpyDeviceToDevice, st));
    reduce_over_ranks(h, sums, (size_t)2 * HP, st);
    launch_bn_bwd_apply<T>(b[DC2], P.tape_z1.template as<T>(), fe, HP, d.Fe, stats, h->bn_count, sums, own,
                           Wd + L.bn_w, G + L.bn_w, G + L.bn_b, st);               // d z1
    launch_gemm_tn<T>(edgeP, d.FeP, b[DC2], HP, ce, d.FeP, HP, G + L.W0T, HP, G + L.b0p, 0, nullptr, g, st, tn);
  } else {
    launch_ssp_bwd<T>(b[DC2], bufA, P.ro.scale0, E, HP, C, B, st);                 // d acc1
  }
  back_gemm(b[DC2], ce, HP, L.W0T, L.t_W0, d.FeP, b[DE0], false);                  // d edge_P
  HIP_TRY(hipMemsetAsync(b[DN0], 0, cn * d.FnP * sizeof(T), st));                  // d node_P = 0

  int cur = 0;  // b[DE0 + cur], b[DN0 + cur] hold the cotangents of (edge, node)_{p+1}
  for (int p = NP - 1; p >= 0; --p) {
    const PassW<T> &w = P.pass[p];
    PassW<T> gw = w;  // the same offsets inside the gradient blob
    if (G) {
      const auto &q = L.pass[p];
      gw.c1_norm = {G + q.c1n_g, G + q.c1n_b};
      gw.final_norm = {G + q.fin_g, G + q.fin_b};
      gw.c2_norm_1 = {G + q.c2n1_g, G + q.c2n1_b};
      gw.c2_norm_2 = {G + q.c2n2_g, G + q.c2n2_b};
      gw.c3_norm_1 = {G + q.c3n1_g, G + q.c3n1_b};
      gw.c3_norm_2 = {G + q.c3n2_g, G + q.c3n2_b};
    }
    const T *node0 = P.tape_node[p].template as<T>(), *node1 = P.tape_node[p + 1].template as<T>();
    const T *edge0 = P.tape_edge[p].template as<T>(), *edge1 = P.tape_edge[p + 1].template as<T>();
    T *de_next = b[DE0 + cur], *de_prev = b[DE0 + (cur ^ 1)];
    T *dn_next = b[DN0 + cur], *dn_prev = b[DN0 + (cur ^ 1)];
    // recompute this pass's projections from the tape
    project(node0, fn, d.FnP, w.c1_WnT, 2 * d.FnP, c.npc1, w.c1_bias, 0, nullptr);
    project(node1, fn, d.FnP, w.c3_WnT, 6 * d.FeP, c.np3, w.c3_nshift, 0, nullptr);
    project(edge0, fe, d.FeP, w.c3_WeT, 4 * d.FeP, bufB, nullptr, 0, nullptr);
    project(nullptr, fe, d.FnP, w.c2_WT, 2 * d.FeP, bufA, w.c2_bias, 1, node1);
    // EdgeBlock
    chain_after_side();  // (the previous pass's products have read the dY buffers this pass overwrites)
    HIP_TRY(launch_edge_bwd<T>(bufB, c.np3, bufA, edge1, P.tape_agg[p].template as<T>(), de_next, de_prev, b[DPQ],
                               b[DNP3], b[DC2], C, B, g, d, w, G ? &gw : nullptr, st));
    side_after_chain(0);
    back_gemm(b[DPQ], ce, 4 * d.FeP, L.pass[p].c3_WeT, L.pass[p].t_c3We, d.FeP, de_prev, true);
    // node_{p+1} cotangent: incoming + projections + c2 operand
    // (accumulated in place: dn_next is dead once this pass's NodeBlock has consumed it)
    back_gemm(b[DNP3], cn, 6 * d.FeP, L.pass[p].c3_WnT, L.pass[p].t_c3Wn, d.FnP, dn_next, true);
    back_gemm(b[DC2], ce, 2 * d.FeP, L.pass[p].c2_WT, L.pass[p].t_c2W, d.FnP, b[DPROD], false);
    launch_prod_bwd<T>(b[DPROD], node1, dn_next, C, B, g, d, st);
    if (G) {
      const auto &q = L.pass[p];
      launch_gemm_tn<T>(edge0, d.FeP, b[DPQ], 4 * d.FeP, ce, d.FeP, 4 * d.FeP, G + q.c3_WeT, 4 * d.FeP, nullptr, 0, nullptr, g, sd, tn);
      launch_gemm_tn<T>(node1, d.FnP, b[DNP3], 6 * d.FeP, cn, d.FnP, 6 * d.FeP, G + q.c3_WnT, 6 * d.FeP, G + q.c3_nshift, 0, nullptr, g, sd, tn);
      // the c2 operand node[b]*node[a], read as plain rows: into d prod's buffer once that is consumed -- or, beside the chain,
      // into a buffer of its own
      T *prod = overlap ? b[DPROD2] : b[DPROD];
      launch_prod_fwd<T>(node1, prod, fe, g, d, sd);
      launch_gemm_tn<T>(prod, d.FnP, b[DC2], 2 * d.FeP, ce, d.FnP, 2 * d.FeP, G + q.c2_WT, 2 * d.FeP, G + q.c2_bias, 0, nullptr, g, sd, tn);
    }
    // NodeBlock (needs bc1 = We edge_p, recomputed into bufA now that c2pre is consumed)
    project(edge0, fe, d.FeP, w.c1_WeT, 2 * d.FnP, bufA, nullptr, 0, nullptr);
    launch_node_bwd<T>(c.npc1, bufA, node1, dn_next, dn_prev, b[DBC1], b[DNPC1], C, B, g, d, w,
                       G ? &gw : nullptr, st);
    side_after_chain(1);
    back_gemm(b[DBC1], ce, 2 * d.FnP, L.pass[p].c1_WeT, L.pass[p].t_c1We, d.FeP, de_prev, true);
    back_gemm(b[DNPC1], cn, 2 * d.FnP, L.pass[p].c1_WnT, L.pass[p].t_c1Wn, d.FnP, dn_prev, true);
    if (G) {
      const auto &q = L.pass[p];
      launch_gemm_tn<T>(edge0, d.FeP, b[DBC1], 2 * d.FnP, ce, d.FeP, 2 * d.FnP, G + q.c1_WeT, 2 * d.FnP, nullptr, 0, nullptr, g, sd, tn);
      launch_gemm_tn<T>(node0, d.FnP, b[DNPC1], 2 * d.FnP, cn, d.FnP, 2 * d.FnP, G + q.c1_WnT, 2 * d.FnP, G + q.c1_bias, 0, nullptr, g, sd, tn);
    }
    cur ^= 1;
  }
  chain_after_side();
  if (tn) launch_tn_reduce(*tn, st);
  if (G) {
    P.type_sums.ensure((size_t)h->cfg.num_atom_types * d.Fn * sizeof(T));
    launch_node_embed_bwd<T>(b[DN0 + cur], S, g, d, h->cfg.num_atom_types, Wd + L.emb, Wd + L.W2, Wd + L.b2,
                             Wd + L.W4, G + L.emb, G + L.W2, G + L.b2, G + L.W4, G + L.b4,
                             P.type_sums.template as<T>(), c.io.types, st);
  }
  if (rv.d_dpos)
    launch_geom_bwd<T>(b[DE0 + cur], b[DUNIT], unit4, P.lattice.template as<T>(), P.offsets,
                       (T)h->cfg.gauss_coefficient, C, B, g, d, rv.d_dpos, st);
  if (rv.in_dpos || rv.in_dlat) {
    P.in_dcart.ensure((size_t)C * E * 3 * sizeof(double));
    launch_geom_input_bwd<T>(b[DE0 + cur], b[DUNIT], unit4, c.io.pos, c.io.lat ? c.io.lat : P.lattice.template as<T>(),
                             c.io.lat ? 9 : 0, P.offsets, (T)h->cfg.gauss_coefficient, C, B, g, d,
                             P.in_dcart.template as<double>(), rv.in_dpos, rv.in_dlat, st);
  }
  HIP_TRY(hipGetLastError());
}

template <typename T>
void ensure_tape(rn_potgnn *h, int S) {
  Precision<T> &P = prec<T>(h);
  const int NP = h->cfg.num_message_passes;
  P.tape_node.resize(NP + 1);
  P.tape_edge.resize(NP + 1);
  P.tape_agg.resize(NP + 1);
  for (int p = 0; p <= NP; ++p) {
    P.tape_node[p].ensure((size_t)S * h->g.N * h->d.FnP * sizeof(T));
    P.tape_edge[p].ensure((size_t)S * h->g.E * h->d.FeP * sizeof(T));
    P.tape_agg[p].ensure((size_t)S * h->g.E * h->d.FeP * sizeof(T));
  }
  // the reverse pass and the training-mode readout work on full-width projections of the taped batch
  Lane<T> &ln = P.lanes[0];
  ln.bufA.ensure((size_t)S * h->g.E * bufA_width(h, false) * sizeof(T));
  ln.bufB.ensure((size_t)S * h->g.E * 4 * h->d.FeP * sizeof(T));
}

// forward of S frames on lane 0 with the per-pass embeddings recorded
template <typename T>
ChunkRun<T> taped_forward(rn_potgnn *h, const ForwardIO<T> &io /* pos, lat, types */, int S) {
  Precision<T> &P = prec<T>(h);
  ensure_tape<T>(h, S);
  P.tape_on = true;
  ChunkRun<T> c(h, P.lanes[0], io, S);
  try {
    c.run_stages();
  } catch (...) {
    P.tape_on = false;
    throw;
  }
  P.tape_on = false;
  return c;
}

// d(standardised 6-vector)/d(fractional positions) at ONE structure: six cotangents (one
// per component) pushed back through readout, P x (EdgeBlock, NodeBlock), radial basis and
// geometry.
template <typename T>
void jacobian(rn_potgnn *h, const double *host_pos, double *host_jac /*[6][N*3]*/) {
  ensure_precision<T>(h);
  const int N = h->g.N;
  h->train_S = 0;  // the tape and lane 0 are reused: a pending train_forward is void
  ForwardIO<T> io;
  io.pos = stage<double>(h->io_pos, host_pos, (size_t)N * 3 * sizeof(double));
  ChunkRun<T> c = taped_forward<T>(h, io, 1);
  hipStream_t st = c.st();
  DeviceBuf dposbuf, seeds;
  dposbuf.ensure((size_t)6 * N * 3 * sizeof(double));
  seeds.ensure(36 * sizeof(T));
  HIP_TRY(hipMemsetAsync(dposbuf.p, 0, (size_t)6 * N * 3 * sizeof(double), st));
  std::vector<T> eye(36, (T)0);
  for (int k = 0; k < 6; ++k) eye[k * 6 + k] = (T)1;
  HIP_TRY(hipMemcpyAsync(seeds.p, eye.data(), sizeof(T) * 36, hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  Reverse<T> rv{1, 6, seeds.as<T>(), dposbuf.as<double>(), nullptr, false};
  reverse_pass<T>(h, c, rv);
  HIP_TRY(hipStreamSynchronize(st));
  check_ps_fail(h);
  HIP_TRY(hipMemcpy(host_jac, dposbuf.p, (size_t)6 * N * 3 * sizeof(double), hipMemcpyDeviceToHost));
}

// Frames per taped chunk of the input-gradient entry: the handle's work chunk, further bounded so that the tape, lane 0's
// full-width buffers and the reverse pass's workspace of one chunk stay within kTapeBudget bytes (38 MB per frame of
// config 3's shape -- 256 atoms, 4608 edges, Fn = Fe = 64, four passes -- in float32: 111 frames a chunk).
constexpr size_t kTapeBudget = (size_t)4 << 30;
size_t tape_elems(const rn_potgnn *h) {  // the tape of one frame (ensure_tape)
  const size_t N = h->cfg.num_atoms, E = h->cfg.num_edges, NP = h->cfg.num_message_passes;
  return (NP + 1) * (N * h->d.FnP + 2 * E * h->d.FeP);
}
size_t reverse_elems(const rn_potgnn *h) {  // the reverse pass's workspace for one cotangent row of one frame (reverse_pass: sizes)
  const size_t N = h->cfg.num_atoms, E = h->cfg.num_edges;
  const size_t FnP = h->d.FnP, FeP = h->d.FeP, HP = std::max<size_t>(FeP, 32);
  return E * (2 * FeP + 4 * FeP + std::max(2 * FeP, HP) + FnP + 2 * FnP + 32 + 4 + HP + 32) + N * (3 * FnP + 6 * FeP + 2 * FnP);
}
template <typename T>
int tape_frames(const rn_potgnn *h) {
  const size_t E = h->cfg.num_edges;
  const size_t per = (tape_elems(h) + per_structure_elems(h, false) + reverse_elems(h)) * sizeof(T) + E * 3 * sizeof(double);
  return (int)std::max<size_t>(1, std::min<size_t>((size_t)chunk_frames<T>(h), kTapeBudget / std::max<size_t>(per, 1)));
}

// Input gradients of the evaluation-mode forward (rn_potgnn_forward_vjp_device): per chunk of frames, the taped forward on
// lane 0 and one reverse pass with one cotangent per frame, in precision T.  Ordered after `user`; `user` waits for the
// work and is synchronised once at the end (the EdgeBlock's time-out word is read there).
template <typename T>
void forward_vjp(rn_potgnn *h, const double *d_lat /* [S][9] or null */, const int32_t *d_types /* [S][N] or null */,
                 const double *d_pos, int64_t S, const double *d_dvec6, double *d_dpos, double *d_dlat, hipStream_t user) {
  ensure_precision<T>(h);
  Precision<T> &P = prec<T>(h);
  const int N = h->g.N;
  h->train_S = 0;  // the tape and lane 0 are reused: a pending train_forward is void
  hipStream_t st = P.lanes[0].stream;
  behind_caller(h, user, P.lanes, 1);
  const int chunk = tape_frames<T>(h);
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    const int s = (int)std::min<int64_t>(chunk, S - s0);
    ForwardIO<T> io;
    io.pos = d_pos + s0 * N * 3;
    io.types = d_types ? d_types + s0 * N : nullptr;
    if (d_lat) {  // in the arithmetic of the run, as the forward casts them
      P.in_lat.ensure((size_t)s * 9 * sizeof(T));
      launch_cast_from_f64<T>(d_lat + s0 * 9, P.in_lat.template as<T>(), (int64_t)s * 9, st);
      io.lat = P.in_lat.template as<T>();
    }
    ChunkRun<T> c = taped_forward<T>(h, io, s);
    P.seeds.ensure((size_t)s * 6 * sizeof(T));
    launch_cast_from_f64<T>(d_dvec6 + s0 * 6, P.seeds.template as<T>(), (int64_t)s * 6, st);
    Reverse<T> rv{s, 1, P.seeds.template as<T>(), nullptr, nullptr, false};
    rv.in_dpos = d_dpos ? d_dpos + s0 * N * 3 : nullptr;
    rv.in_dlat = d_dlat ? d_dlat + s0 * 9 : nullptr;
    reverse_pass<T>(h, c, rv);
  }
  hand_back(h, user, P.lanes, 1, true);
}

// ---- atom-group contractions (rn_potgnn_group_increments_device, rn_potgnn_partial_raman_tensors); G <= kMaxGroups (kernels.hpp)

// The group table h->groups (increments.hpp) is updated with nothing to wait for: every increments call returns
// synchronised through hand_back(..., true), and partial_raman_tensors synchronises lane 0 before it stages, so no work
// enqueued earlier still reads the old permutation.

// Frames per taped chunk of the group entries in precision T: the tape, lane 0's buffers and the reverse pass of six
// cotangent rows per frame (their per-edge Cartesian cotangents and Jacobian rows included) of F frames, plus one frame of
// Jacobian rows carried over, within `limit` bytes; 0 when not even one frame fits.
template <typename T>
int group_frames(const rn_potgnn *h, size_t limit, bool cells = false) {
  const size_t N = h->cfg.num_atoms, E = h->cfg.num_edges;
  const size_t rows = (6 * N * 3 + (cells ? 6 * 9 : 0)) * sizeof(double);  // (a variable cell: the lattice rows too)
  const size_t per = (tape_elems(h) + per_structure_elems(h, false) + 6 * reverse_elems(h) + 36) * sizeof(T) +
                     6 * E * 3 * sizeof(double) + rows;
  if (limit < per + rows) return 0;
  return (int)std::min<size_t>((size_t)chunk_frames<T>(h), (limit - rows) / per);
}

// d vec6_c / d x of s frames (device float64 [s][N][3]) -> d_jac device float64 [s][6][N][3]: the taped forward on lane 0
// and one reverse pass with six one-hot cotangent rows per frame (geom_input_bwd_kernel: every entry written, no atomics).
// d_lat (device T [s][9], or null: the reference structure's lattice): each frame is evaluated and differentiated at its
// own lattice; d_jl (or null) then receives d vec6_c / d L, float64 [s][6][9].
template <typename T>
void jacobian_rows(rn_potgnn *h, const double *d_pos, int s, double *d_jac, const T *d_lat = nullptr, double *d_jl = nullptr) {
  Precision<T> &P = prec<T>(h);
  if (P.eye_frames < s) {
    std::vector<T> eye((size_t)s * 36, (T)0);
    for (int f = 0; f < s; ++f)
      for (int k = 0; k < 6; ++k) eye[(size_t)f * 36 + k * 6 + k] = (T)1;
    HIP_TRY(hipStreamSynchronize(P.lanes[0].stream));  // (an earlier chunk may still read the old seeds)
    P.eye_seeds.ensure(eye.size() * sizeof(T));
    HIP_TRY(hipMemcpy(P.eye_seeds.p, eye.data(), eye.size() * sizeof(T), hipMemcpyHostToDevice));
    P.eye_frames = s;
  }
  ForwardIO<T> io;
  io.pos = d_pos;
  io.lat = d_lat;
  ChunkRun<T> c = taped_forward<T>(h, io, s);
  Reverse<T> rv{s, 6, P.eye_seeds.template as<T>(), nullptr, nullptr, false};
  rv.in_dpos = d_jac;
  rv.in_dlat = d_jl;
  reverse_pass<T>(h, c, rv);
}

// The chunk walk of every increment entry (increments.hpp: walk_chunks): the S frames d_pos (device float64 [S][N][3]) go
// through in chunks of F = group_frames steps, and contract(jac, pos, f, out, st) launches the contraction of a chunk's f
// steps (jac [f+1][6][N][3], pos the chunk's first frame, out its first step's row of d_out [S-1][out_channels][9]) on
// lane 0's stream.  Ordered after `user`; `user` waits for the work and is synchronised once at the end.
// d_lat (device float64 [S][9], or null): a lattice per frame.  The Jacobian rows are then taken at each frame's own
// lattice (cast to T, as the forward casts it), their lattice rows J_L [6][9] are carried over chunk boundaries with them,
// and channel `cell_channel` of d_out is the cell's share 1/2 (J_L(t) + J_L(t+1)) : (L_{t+1} - L_t).
template <typename T, class Contract>
void chunked_increments(rn_potgnn *h, const double *d_pos, int64_t S, size_t limit, int out_channels, int cell_channel,
                        double *d_out, hipStream_t user, const double *d_lat, const char *too_small, Contract contract) {
  ensure_precision<T>(h);
  Precision<T> &P = prec<T>(h);
  const int N = h->g.N;
  const int F = group_frames<T>(h, limit, d_lat != nullptr);
  if (F < 1) throw HipError{hipErrorOutOfMemory, too_small};
  h->train_S = 0;  // the tape and lane 0 are reused: a pending train_forward is void
  hipStream_t st = P.lanes[0].stream;
  behind_caller(h, user, P.lanes, 1);
  const int64_t rows = (int64_t)6 * N * 3;
  h->grp_jac.ensure((size_t)(F + 1) * rows * sizeof(double));
  double *jac = h->grp_jac.as<double>();
  const double *sigma = h->d_mean_std.as<double>() + 9;
  const T *lat = nullptr;  // the lattices as the kernels of this precision read them
  double *jl = nullptr;
  if (d_lat) {
    h->grp_jl.ensure((size_t)(F + 1) * 54 * sizeof(double));
    jl = h->grp_jl.as<double>();
    if constexpr (sizeof(T) == 8) {
      lat = d_lat;
    } else {
      h->grp_lat.ensure((size_t)S * 9 * sizeof(T));
      launch_cast_from_f64<T>(d_lat, h->grp_lat.as<T>(), S * 9, st);
      lat = h->grp_lat.as<T>();
    }
  }
  walk_chunks(
      S, F, rows, jac, st,
      [&](int64_t first, int64_t count, double *to, double *to_jl) {
        jacobian_rows<T>(h, d_pos + first * N * 3, (int)count, to, lat ? lat + first * 9 : nullptr, to_jl);
      },
      [&](int64_t t0, int64_t f) {
        contract(jac, d_pos + t0 * N * 3, (int)f, d_out + t0 * out_channels * 9, st);
        if (jl) launch_cell_increments(jl, d_lat + t0 * 9, f, cell_channel, out_channels, sigma, d_out + t0 * out_channels * 9, st);
      },
      jl, 54);
  hand_back(h, user, P.lanes, 1, true);
}

// Trapezoid increments per atom group -> d_out [S-1][G][9], or, with a lattice per frame, [S-1][G+1][9]: channel G is
// the cell's share.
template <typename T>
void group_increments(rn_potgnn *h, const double *d_pos, int64_t S, int G, size_t limit, double *d_out,
                      hipStream_t user, const double *d_lat = nullptr) {
  const int N = h->g.N;
  const int *perm = h->groups.perm(), *gptr = perm + N;
  const double *sigma = h->d_mean_std.as<double>() + 9;
  const int out_groups = d_lat ? G + 1 : G;
  chunked_increments<T>(h, d_pos, S, limit, out_groups, G, d_out, user, d_lat,
                        "group_increments: one step does not fit the workspace limit",
                        [&](const double *jac, const double *pos, int f, double *out, hipStream_t st) {
                          launch_group_increments(jac, (int64_t)6 * N * 3, pos, nullptr, 0.0, f, N, perm, gptr, G, sigma,
                                                  out, st, out_groups);
                        });
}

// The contraction of one chunk of Jacobian rows with M modes (both mode entries): channels 0 .. M-1 and, with `rest`,
// channel M of out [frames-1][out_channels][9]; everything a device pointer.
void mode_contract(const double *jac, int64_t frames, const double *pos, int N, const double *disp, const double *proj,
                   int M, const double *sigma, bool rest, int out_channels, double *out, hipStream_t st) {
  launch_mode_increments(jac, pos, frames - 1, N, disp, proj, M, sigma, out_channels, out, st);
  if (rest) launch_mode_rest(jac, pos, frames - 1, N, M, sigma, out_channels, out, st);
}

// Trapezoid increments per phonon mode -> d_out [S-1][M + rest (+ 1)][9]: the modes, the rest and, with a lattice per
// frame, the cell.  disp / proj: host [M][N][3], uploaded once and counted against `limit`.
template <typename T>
void mode_increments(rn_potgnn *h, const double *d_pos, int64_t S, const double *disp, const double *proj, int M,
                     bool rest, size_t limit, double *d_out, hipStream_t user, const double *d_lat) {
  const int N = h->g.N;
  ensure_precision<T>(h);
  const ModeVectors modes = upload_modes(h->mode_vectors, disp, proj, M, N, limit, prec<T>(h).lanes[0].stream);
  const double *sigma = h->d_mean_std.as<double>() + 9;
  const int channels = M + (rest ? 1 : 0);
  const int out_channels = channels + (d_lat ? 1 : 0);
  chunked_increments<T>(h, d_pos, S, limit - modes.bytes, out_channels, channels, d_out, user, d_lat,
                        "mode_increments: one step does not fit the workspace limit",
                        [&](const double *jac, const double *pos, int f, double *out, hipStream_t st2) {
                          mode_contract(jac, (int64_t)f + 1, pos, N, modes.disp, modes.proj, M, sigma, rest, out_channels, out, st2);
                        });
}

// refresh `packed` (and the float64 copy, when it exists) from the device weights
void sync_host(rn_potgnn *h) {
  if (!h->host_stale) return;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h->packed.data(), h->f32.weights.p, h->packed.size() * sizeof(float), hipMemcpyDeviceToHost));
  h->host_stale = false;
  if (h->f64.ready) upload_weights<double>(h);
}

// Per-sample lattices [S][9] (cast to the arithmetic of the run: the reference's forward computes in its default dtype) and
// atom types [S][N] of the host entries, into h->io_lat / h->io_types; null stays null.
template <typename T>
const T *stage_lattices(rn_potgnn *h, const double *lat, int64_t S) {
  if (!lat) return nullptr;
  if constexpr (sizeof(T) == 8) {
    return stage<T>(h->io_lat, lat, (size_t)S * 9 * sizeof(double));
  } else {
    const std::vector<float> lat32(lat, lat + S * 9);
    return stage<T>(h->io_lat, lat32.data(), lat32.size() * sizeof(float));
  }
}
const int *stage_types(rn_potgnn *h, const int32_t *types, int64_t S) {
  return types ? stage<int>(h->io_types, types, (size_t)S * h->cfg.num_atoms * sizeof(int32_t)) : nullptr;
}

// ---- training: forward with batch-statistics BatchNorm, then parameter gradients (float32 for
// the product path; float64 for validating the reverse pass against float64 autograd)
// The taped forward + the training-mode readout (batch-statistics BatchNorm) over the S structures whose positions (and, per
// h->train_lat / h->train_types, lattices and atom types) sit in h->io_pos / io_lat / io_types; everything is enqueued on lane
// 0's stream, the standardised 6-vectors end up in h->io_vec6 / io_alpha and the batch statistics in P.mv.
template <typename T>
ForwardIO<T> train_io(rn_potgnn *h) {  // what the pending (or starting) train_forward runs with
  ForwardIO<T> io;
  io.pos = h->io_pos.as<double>();
  io.lat = h->train_lat ? h->io_lat.as<T>() : nullptr;
  io.types = h->train_types ? h->io_types.as<int>() : nullptr;
  return io;
}
template <typename T>
ChunkRun<T> train_forward_core(rn_potgnn *h, int S) {
  Precision<T> &P = prec<T>(h);
  const PackedLayout &L = h->lay;
  const Graph &g = h->g;
  const Dims d = h->d;
  const int HP = std::max(d.FeP, 32);
  ChunkRun<T> c = taped_forward<T>(h, train_io<T>(h), S);
  hipStream_t st = c.st();
  const int64_t R = (int64_t)S * g.E;
  T *Wd = P.weights.template as<T>();
  P.tape_z1.ensure((size_t)R * HP * sizeof(T));
  P.bn_stats.ensure(sizeof(double) * 6 * HP);  // forward sums (+ row count during the reduction) | backward sums | own copy
  DeviceBuf &mv = P.mv;
  mv.ensure(sizeof(T) * 2 * HP);
  const T *edgeP = P.tape_edge[h->cfg.num_message_passes].template as<T>();
  // z1 = edge W0^T + b0 ; h1 = ssp(BN_batch(z1)) ; then the rest of the readout as in eval
  launch_rowgemm<T>(edgeP, R, d.FeP, P.ro.W0T, HP, P.tape_z1.template as<T>(), nullptr, Wd + L.b0p, false, 0,
                    nullptr, g, st);
  {
    // batch statistics over every row of the batch -- of all ranks in a data-parallel run
    double *stats = P.bn_stats.template as<double>();
    launch_bn_col_sums<T>(P.tape_z1.template as<T>(), R, HP, stats, st);
    h->bn_count = (double)R;
    if (h->reducer) {
      const double rows = (double)R;  // slot 2HP is outside the range col_sums clears
      HIP_TRY(hipMemcpy(stats + 2 * HP, &rows, sizeof(double), hipMemcpyHostToDevice));
      reduce_over_ranks(h, stats, (size_t)2 * HP + 1, st);  // [sum z | sum z^2 | rows]
      HIP_TRY(hipMemcpy(&h->bn_count, stats + 2 * HP, sizeof(double), hipMemcpyDeviceToHost));
    }
    launch_bn_train_apply<T>(P.tape_z1.template as<T>(), R, HP, d.Fe, stats, h->bn_count, Wd + L.bn_w, Wd + L.bn_b,
                             c.bufA, mv.template as<T>(), st);
  }
  launch_rowgemm<T>(c.bufA, R, HP, P.ro.W3T, HP, c.bufB, P.ones, P.ro.b3, true, 0, nullptr, g, st);
  launch_rowgemm<T>(c.bufB, R, HP, P.ro.W5T, 32, c.bufA, nullptr, P.ro.b5, false, 0, nullptr, g, st);
  h->io_vec6.ensure((size_t)S * 6 * sizeof(float));
  h->io_alpha.ensure((size_t)S * 9 * sizeof(double));
  const double *ms = h->d_mean_std.as<double>();
  launch_readout_reduce<T>(c.bufA, c.unit4, S, g, ms, ms + 9, h->io_vec6.as<float>(), nullptr,
                           h->io_alpha.as<double>() /* standardised 3x3 in double */, st);
  HIP_TRY(hipGetLastError());
  return c;
}
// The kernels that rewrite the float32 weights on the device run on lane 0.  An evaluation that returned unfinished (the
// to-device entry, a device entry without synchronisation) may still read them on lane 1, whose last kernels of a lane pair
// are ordered behind nothing on lane 0: `st` waits for the other lanes' last evaluation first.
inline void after_other_lanes(rn_potgnn *h, hipStream_t st) {
  for (auto &ln : h->f32.lanes)
    if (ln.stream && ln.stream != st && ln.done) HIP_TRY(hipStreamWaitEvent(st, ln.done, 0));
}

// running statistics where the weights live (torch: momentum 0.1, unbiased variance) and everything derived from them
inline void train_running_stats(rn_potgnn *h, hipStream_t st) {
  Precision<float> &P = h->f32;
  const PackedLayout &L = h->lay;
  const Dims d = h->d;
  const int HP = std::max(d.FeP, 32);
  float *Wd = P.weights.as<float>();
  const double rows = h->bn_count;
  after_other_lanes(h, st);
  launch_bn_running(Wd + L.bn_rm, Wd + L.bn_rv, P.mv.as<float>(), P.mv.as<float>() + HP, d.Fe, 0.1,
                    rows / std::max(rows - 1.0, 1.0), st);
  device_setup<float>(h, Wd, st);
  h->host_stale = true;
}

template <typename T>
void train_forward(rn_potgnn *h, const double *host_pos, int S, T *vec6, T *batch_mean, T *batch_var,
                   const double *host_lat = nullptr /* [S][9] or null */, const int32_t *host_types = nullptr /* [S][N] or null */) {
  ensure_precision<T>(h);
  Precision<T> &P = prec<T>(h);
  const Graph &g = h->g;
  const Dims d = h->d;
  const int HP = std::max(d.FeP, 32);
  stage<double>(h->io_pos, host_pos, (size_t)S * g.N * 3 * sizeof(double));
  // per-sample lattices (in the arithmetic of the run, as the reference's forward casts them) and atom types: the graph
  // topology stays the reference structure's (_gnn.py:603-611, 541-557)
  stage_lattices<T>(h, host_lat, S);
  stage_types(h, host_types, S);
  h->train_lat = host_lat != nullptr;
  h->train_types = host_types != nullptr;
  ChunkRun<T> c = train_forward_core<T>(h, S);
  hipStream_t st = c.st();
  DeviceBuf &mv = P.mv;
  HIP_TRY(hipStreamSynchronize(st));
  check_ps_fail(h);
  if constexpr (sizeof(T) == 4) {
    HIP_TRY(hipMemcpy(vec6, h->io_vec6.p, (size_t)S * 6 * sizeof(float), hipMemcpyDeviceToHost));
  } else {  // (xx,yy,zz,xy,xz,yz) of the standardised tensor, at full precision
    std::vector<double> raw((size_t)S * 9);
    HIP_TRY(hipMemcpy(raw.data(), h->io_alpha.p, raw.size() * sizeof(double), hipMemcpyDeviceToHost));
    const int pick[6] = {0, 4, 8, 1, 2, 5};
    for (int s = 0; s < S; ++s)
      for (int k = 0; k < 6; ++k) vec6[(size_t)s * 6 + k] = (T)raw[(size_t)s * 9 + pick[k]];
  }
  if constexpr (sizeof(T) == 4) {
    if (h->device_training) {
      train_running_stats(h, st);
      HIP_TRY(hipStreamSynchronize(st));
    }
  }
  std::vector<T> mvh(2 * HP);
  HIP_TRY(hipMemcpy(mvh.data(), mv.p, sizeof(T) * 2 * HP, hipMemcpyDeviceToHost));
  for (int k = 0; k < d.Fe; ++k) {
    batch_mean[k] = mvh[k];
    batch_var[k] = mvh[HP + k];
  }
  h->train_S = S;
  h->train_prec = (int)sizeof(T);
}

// The same step with everything where it already is (device-resident training, float32): positions [S][N][3] float64,
// optional lattices [S][9] float32 and atom types [S][N] int32, and the [S][6] result are DEVICE buffers; work is ordered
// after `user` and `user` is made to wait for it; no host round trip, no synchronisation.
inline void train_forward_device(rn_potgnn *h, const double *d_pos, int S, const float *d_lat, const int32_t *d_types,
                                 float *d_vec6, hipStream_t user) {
  ensure_precision<float>(h);
  Precision<float> &P = h->f32;
  const Graph &g = h->g;
  hipStream_t st = P.lanes[0].stream;
  behind_caller(h, user, P.lanes, 1);
  const size_t pb = (size_t)S * g.N * 3 * sizeof(double);
  h->io_pos.ensure(pb);  // (the reverse pass reads the positions again)
  HIP_TRY(hipMemcpyAsync(h->io_pos.p, d_pos, pb, hipMemcpyDeviceToDevice, st));
  if (d_lat) {
    h->io_lat.ensure((size_t)S * 9 * sizeof(float));
    HIP_TRY(hipMemcpyAsync(h->io_lat.p, d_lat, (size_t)S * 9 * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  if (d_types) {
    h->io_types.ensure((size_t)S * g.N * sizeof(int32_t));
    HIP_TRY(hipMemcpyAsync(h->io_types.p, d_types, (size_t)S * g.N * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  }
  h->train_lat = d_lat != nullptr;
  h->train_types = d_types != nullptr;
  (void)train_forward_core<float>(h, S);
  HIP_TRY(hipMemcpyAsync(d_vec6, h->io_vec6.p, (size_t)S * 6 * sizeof(float), hipMemcpyDeviceToDevice, st));
  train_running_stats(h, st);
  hand_back(h, user, P.lanes, 1, false);
  h->train_S = S;
  h->train_prec = 4;
}

template <typename T>
void train_backward(rn_potgnn *h, const T *dvec6, T *grads /* null: leave the gradients on the device */,
                    double *host_dpos = nullptr /* [S][N][3] or null */, double *host_dlat = nullptr /* [S][9] or null */) {
  Precision<T> &P = prec<T>(h);
  const int S = h->train_S;
  if (S <= 0 || h->train_prec != (int)sizeof(T))
    throw HipError{hipErrorInvalidValue, "train_backward without a train_forward of the same precision"};
  ChunkRun<T> c(h, P.lanes[0], train_io<T>(h), S);
  hipStream_t st = c.st();
  const T *seeds = stage<T>(P.seeds, dvec6, (size_t)S * 6 * sizeof(T));
  P.grad.ensure(h->lay.total * sizeof(T));
  HIP_TRY(hipMemsetAsync(P.grad.p, 0, h->lay.total * sizeof(T), st));
  Reverse<T> rv{S, 1, seeds, nullptr, P.grad.template as<T>(), true};
  const size_t npos = (size_t)S * h->g.N * 3;
  if (host_dpos || host_dlat) {  // input gradients from the same reverse pass (device scratch, copied out below)
    P.in_grads.ensure((npos + (size_t)S * 9) * sizeof(double));
    rv.in_dpos = host_dpos ? P.in_grads.template as<double>() : nullptr;
    rv.in_dlat = host_dlat ? P.in_grads.template as<double>() + npos : nullptr;
  }
  reverse_pass<T>(h, c, rv);
  HIP_TRY(hipStreamSynchronize(st));
  h->train_S = 0;  // (the pending forward is consumed whether or not the check below throws)
  check_ps_fail(h);
  if (host_dpos) HIP_TRY(hipMemcpy(host_dpos, rv.in_dpos, npos * sizeof(double), hipMemcpyDeviceToHost));
  if (host_dlat) HIP_TRY(hipMemcpy(host_dlat, rv.in_dlat, (size_t)S * 9 * sizeof(double), hipMemcpyDeviceToHost));
  if (sizeof(T) == 4) h->grads_on_device = true;
  if (!grads) return;
  std::vector<T> gp(h->lay.total);
  HIP_TRY(hipMemcpy(gp.data(), P.grad.p, gp.size() * sizeof(T), hipMemcpyDeviceToHost));
  unpack_weights<T>(h->lay, gp.data(), grads, false);
}

// Reverse pass of a pending train_forward(_device) with the cotangents [S][6] in a DEVICE buffer; the gradients stay in HBM
// (device-resident training), nothing is synchronised: `user` waits for the lane, the Adam step runs on the lane's stream.
inline void train_backward_device(rn_potgnn *h, const float *d_dvec6, hipStream_t user, double *d_dpos = nullptr,
                                  double *d_dlat = nullptr) {
  Precision<float> &P = h->f32;
  const int S = h->train_S;
  if (S <= 0 || h->train_prec != 4)
    throw HipError{hipErrorInvalidValue, "train_backward without a train_forward of the same precision"};
  ChunkRun<float> c(h, P.lanes[0], train_io<float>(h), S);
  hipStream_t st = c.st();
  behind_caller(h, user, P.lanes, 1);
  P.seeds.ensure((size_t)S * 6 * sizeof(float));
  HIP_TRY(hipMemcpyAsync(P.seeds.p, d_dvec6, (size_t)S * 6 * sizeof(float), hipMemcpyDeviceToDevice, st));
  P.grad.ensure(h->lay.total * sizeof(float));
  HIP_TRY(hipMemsetAsync(P.grad.p, 0, h->lay.total * sizeof(float), st));
  Reverse<float> rv{S, 1, P.seeds.as<float>(), nullptr, P.grad.as<float>(), true};
  rv.in_dpos = d_dpos;  // (input gradients, when asked for, from the same reverse pass)
  rv.in_dlat = d_dlat;
  reverse_pass<float>(h, c, rv);
  hand_back(h, user, P.lanes, 1, false);
  h->train_S = 0;
  h->grads_on_device = true;
}

// ---- what the entries share: argument checks (each returns kGo, or the status the entry returns at once) and lazily
// created streams / events

constexpr int kGo = 1;  // (no rn_status is positive)

int refuse(rn_potgnn *h, const char *text) {
  set_error(h, "%s", text);
  return RN_ERR_INVALID_ARGUMENT;
}

// A batch of S >= 0 frames: refused with `text` when S is negative or, for S > 0, one of `needed` is null; an empty batch is
// RN_OK with nothing touched.  (A null handle is refused without a text: there is nowhere to keep one.)
int check_batch(rn_potgnn *h, int64_t S, std::initializer_list<const void *> needed, const char *text) {
  if (!h) return RN_ERR_INVALID_ARGUMENT;
  bool ok = S >= 0;
  if (S > 0)
    for (const void *p : needed) ok = ok && p;
  if (!ok) return refuse(h, text);
  return S == 0 ? RN_OK : kGo;
}

// Host lattices [S][9] of a variable-cell call (null: the fixed cell, nothing to check): every entry finite and no
// determinant of zero -- |det| <= 1e-12 |a| |b| |c|, so that vectors that are dependent up to rounding count as well --
// before any device work; the text names the first offending frame.
constexpr double kSingularVolume = 1e-12;  // zero within the rounding of the determinant's nine products (dynamics.py: the same)
int check_lattices(rn_potgnn *h, const double *lattices, int64_t S) {
  if (!lattices) return kGo;
  for (int64_t s = 0; s < S; ++s) {
    const double *L = lattices + s * 9;
    for (int i = 0; i < 9; ++i)
      if (!std::isfinite(L[i])) {
        set_error(h, "lattice of frame %lld has a non-finite entry", (long long)s);
        return RN_ERR_INVALID_ARGUMENT;
      }
    const double det = L[0] * (L[4] * L[8] - L[5] * L[7]) - L[1] * (L[3] * L[8] - L[5] * L[6]) + L[2] * (L[3] * L[7] - L[4] * L[6]);
    double edges = 1.0;  // |a| |b| |c|: the volume of the box the vectors would span at right angles
    for (int r = 0; r < 3; ++r) edges *= std::sqrt(L[3 * r] * L[3 * r] + L[3 * r + 1] * L[3 * r + 1] + L[3 * r + 2] * L[3 * r + 2]);
    if (!(std::fabs(det) > kSingularVolume * edges) || !std::isfinite(det)) {
      set_error(h, "lattice of frame %lld is singular (its determinant is %g)", (long long)s, det);
      return RN_ERR_INVALID_ARGUMENT;
    }
  }
  return kGo;
}

int check_types(rn_potgnn *h, const int32_t *atom_types, int64_t S) {
  if (!atom_types) return kGo;
  const size_t SN = (size_t)S * h->cfg.num_atoms;
  for (size_t i = 0; i < SN; ++i)
    if (atom_types[i] < 0 || atom_types[i] >= h->cfg.num_atom_types) {
      set_error(h, "atom type %d of sample %zu, atom %zu is outside [0,%d)", atom_types[i], i / h->cfg.num_atoms,
                i % h->cfg.num_atoms, h->cfg.num_atom_types);
      return RN_ERR_INVALID_ARGUMENT;
    }
  return kGo;
}

// The training entries read handle state in their checks: they take the handle's lock there and keep it through their
// guarded() (`hold` lives in the entry).
struct Checked {
  int rc;
  std::unique_lock<std::recursive_mutex> hold;
};

// Which training step an entry belongs to: float32 or float64 through host buffers, or the device-resident float32 one
// (which needs rn_potgnn_set_device_training).
enum TrainKind { kHostF32, kHostF64, kDeviceF32 };

// A train_forward entry `name`: every pointer of `needed` given, 1 <= S <= the chunk of its precision and, for the
// device-resident form, device training switched on.
Checked check_train_batch(rn_potgnn *h, int64_t S, std::initializer_list<const void *> needed, const char *name,
                          TrainKind kind) {
  const bool f64 = kind == kHostF64, device = kind == kDeviceF32;
  bool ok = h && S > 0;
  for (const void *p : needed) ok = ok && p;
  if (!ok) {
    set_error(h, "invalid arguments to %s", name);
    return {RN_ERR_INVALID_ARGUMENT, {}};
  }
  Checked c{kGo, std::unique_lock<std::recursive_mutex>(h->lock)};
  if (device && !h->device_training) {
    set_error(h, "%s needs device-resident training (rn_potgnn_set_device_training)", name);
    c.rc = RN_ERR_INVALID_ARGUMENT;
  } else if (f64 && S > chunk_frames<double>(h)) {
    set_error(h, "training batch of %lld frames exceeds the float64 chunk of %d frames", (long long)S, chunk_frames<double>(h));
    c.rc = RN_ERR_INVALID_ARGUMENT;
  } else if (!f64 && S > h->chunk) {
    set_error(h, "training batch of %lld frames exceeds max_chunk_structures = %d", (long long)S, h->chunk);
    c.rc = RN_ERR_INVALID_ARGUMENT;
  }
  return c;
}

// A backward entry (`args_ok`: its own null-pointer rule; `name` for that text): the pending train_forward must have run in
// the precision of `kind` -- and, device-resident, with device training on -- else `text`.
Checked check_pending(rn_potgnn *h, bool args_ok, const char *name, TrainKind kind, const char *text) {
  const int prec_bytes = kind == kHostF64 ? 8 : 4;
  const bool device = kind == kDeviceF32;
  if (!h || !args_ok) {
    set_error(h, "invalid arguments to %s", name);
    return {RN_ERR_INVALID_ARGUMENT, {}};
  }
  Checked c{kGo, std::unique_lock<std::recursive_mutex>(h->lock)};
  if ((device && !h->device_training) || h->train_S <= 0 || h->train_prec != prec_bytes) c.rc = refuse(h, text);
  return c;
}

void lazy_stream(hipStream_t &s) {
  if (!s) HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
}
void lazy_event(hipEvent_t &e) {
  if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
}

// fn(T{}) in the precision asked for; float64 first brings the host master copy, from which its weights are made, up to date
template <typename F>
void with_precision(rn_potgnn *h, bool use_float64, F fn) {
  if (use_float64) {
    sync_host(h);
    fn(double{});
  } else {
    fn(float{});
  }
}
}  // namespace

// ================================================================================ C ABI
extern "C" {

const char *rn_potgnn_version(void) { return "ramannoodle_amd-potgnn 0.1 (gfx950)"; }

size_t rn_potgnn_weight_count(const rn_potgnn_config *c) {
  try {
    return state_dict_count(c);
  } catch (const std::exception &) {  // (a pass count no table fits in memory for)
    return 0;
  }
}

const char *rn_potgnn_last_error(const rn_potgnn *h) {
  return h ? h->error.c_str() : g_create_error.c_str();
}

// Packs the plan's int arrays into one device allocation (each padded to 16 bytes) and points a Graph at them.
static Graph upload(const GraphPlan &plan, DeviceBuf &buf) {
  std::vector<int> ints;
  auto push = [&](const std::vector<int> &v) {
    size_t o = ints.size();
    ints.insert(ints.end(), v.begin(), v.end());
    while (ints.size() % 4) ints.push_back(0);
    return o;
  };
  const size_t o_a = push(plan.edge_a), o_b = push(plan.edge_b), o_op = push(plan.out_ptr),
               o_ip = push(plan.in_ptr), o_ie = push(plan.in_edge), o_at = push(plan.atom_type),
               o_tb = push(plan.tile.begin), o_to = push(plan.trip_off), o_rv = push(plan.rev_edge),
               o_nt = push(plan.nt.begin), o_bt = push(plan.bt.begin), o_pt = push(plan.pt.begin), o_ipos = push(plan.in_pos),
               o_pe = push(plan.pair_of_edge), o_pa = push(plan.pair_a), o_pb = push(plan.pair_b);
  buf.ensure(ints.size() * sizeof(int));
  HIP_TRY(hipMemcpy(buf.p, ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice));
  const int *base = buf.as<int>();
  Graph g = plan.scalars();
  g.edge_a = base + o_a;
  g.edge_b = base + o_b;
  g.out_ptr = base + o_op;
  g.in_ptr = base + o_ip;
  g.in_edge = base + o_ie;
  g.in_pos = base + o_ipos;
  g.atom_type = base + o_at;
  g.rev_edge = base + o_rv;
  g.pair_of_edge = base + o_pe;
  g.pair_a = base + o_pa;
  g.pair_b = base + o_pb;
  g.tile_begin = base + o_tb;
  g.trip_off = base + o_to;
  g.nt_begin = base + o_nt;
  g.pt_begin = base + o_pt;
  g.bt_begin = base + o_bt;
  return g;
}

// Chunk size.  Throughput rises monotonically with the frames per launch
// (profiles/r01_chunk_sweep.txt, profiles/r01/overlap_experiments.txt section 7) and the
// Infinity Cache does not reward small chunks.  The fused kernels take a whole CU each, so a
// second lane has nothing to overlap with: ONE lane with an 8 GiB workspace (of 288 GB HBM)
// beats two lanes of 1.5 GiB (63.7 k vs 62.1 k structures/s at 4000 frames).  The unfused
// pipeline keeps two alternating lanes of 1.5 GiB (GraphPlan::num_lanes).
static void size_chunk(rn_potgnn *h) {
  int chunk = h->cfg.max_chunk_structures;
  if (const char *e = getenv("RN_POTGNN_CHUNK")) chunk = atoi(e);
  if (chunk <= 0) {
    const size_t per = per_structure_elems(h, lean_workspace(h)) * sizeof(float);
    size_t budget = (h->plan.use_fused || h->plan.use_narrow) ? ((size_t)8192 << 20) : ((size_t)1536 << 20);
    size_t free_b = 0, total_b = 0;  // on a shared GPU: at most 1/8 of what is free right now
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0)
      budget = std::min(budget, std::max<size_t>(free_b / 8 / (size_t)h->plan.num_lanes, (size_t)64 << 20));
    chunk = (int)std::max<size_t>(1, budget / std::max<size_t>(per, 1));
    chunk = std::min(chunk, 4096);
    // the float64 lanes (created on first use) get their own allowance against the same "an eighth of what is free"
    // rule: up to 24 GiB of the full-width float64 layout (1270 frames at 256 atoms, Fn = Fe = 64), so that the phonon
    // finite differences of config 4 -- 1536 cells -- still run in two launches (chunk_frames<double>)
    h->f64_budget = (size_t)24 << 30;
    if (free_b > 0) h->f64_budget = std::min(h->f64_budget, std::max<size_t>(free_b / 8 / (size_t)h->plan.num_lanes, (size_t)64 << 20));
  }
  h->chunk = chunk;
}

int rn_potgnn_create(const rn_potgnn_config *cfg, const int32_t *edge_a, const int32_t *edge_b,
                     const int32_t *atom_types, const double *lattice, const float *weights,
                     size_t num_weights, const double *mean, const double *stddev,
                     rn_potgnn **out) {
  if (!out) return RN_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  std::string invalid;
  int rc = validate_create_args(cfg, edge_a, edge_b, atom_types, !lattice || !weights || !mean || !stddev, &num_weights, invalid);
  if (rc != RN_OK) {
    set_error<rn_potgnn>(nullptr, "%s", invalid.c_str());
    return rc;
  }

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 ||
      cfg->device >= ndev) {
    set_error<rn_potgnn>(nullptr, "no usable HIP device (count=%d, requested=%d)", ndev, cfg->device);
    return RN_ERR_NO_DEVICE;
  }
  int cus = 256;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
  }

  std::unique_ptr<rn_potgnn> h(new rn_potgnn());
  h->cfg = *cfg;
  std::memcpy(h->lattice, lattice, sizeof(h->lattice));
  std::memcpy(h->mean, mean, sizeof(h->mean));
  std::memcpy(h->stdv, stddev, sizeof(h->stdv));
  h->snap_pairs = getenv("RN_POTGNN_KEEP_STAGES") && atoi(getenv("RN_POTGNN_KEEP_STAGES")) == 2;
  h->keep_stages = getenv("RN_POTGNN_KEEP_STAGES") && atoi(getenv("RN_POTGNN_KEEP_STAGES")) != 0 && !h->snap_pairs;
  h->debug_sync = getenv("RN_POTGNN_DEBUG_SYNC") && atoi(getenv("RN_POTGNN_DEBUG_SYNC")) != 0;
  if (const char *e = getenv("RN_POTGNN_INTERLEAVE")) h->interleave = atoi(e) != 0;
  if (const char *e = getenv("RN_POTGNN_MFMA")) h->mfma_f16_requested = !(e[0] == 'f' && e[1] == '3');
  h->mfma_f16 = h->mfma_f16_requested;
  if (const char *e = getenv("RN_POTGNN_TAPE_FUSED")) h->tape_fused = atoi(e) != 0;
  if (const char *e = getenv("RN_POTGNN_TAPE_PS")) h->tape_ps = atoi(e) != 0;
  h->split_projections = getenv("RN_POTGNN_SPLIT_PROJ") ? atoi(getenv("RN_POTGNN_SPLIT_PROJ")) != 0 : true;
  h->want_pair_rows = !(getenv("RN_POTGNN_PAIR_ROWS") && atoi(getenv("RN_POTGNN_PAIR_ROWS")) == 0);
  h->want_c2_pairs = !(getenv("RN_POTGNN_C2_PAIRS") && atoi(getenv("RN_POTGNN_C2_PAIRS")) == 0);

  const PlanKnobs knobs = read_plan_knobs();
  h->d = plan_dims(*cfg, knobs);
  h->plan = plan_graph(*cfg, h->d, edge_a, edge_b, atom_types, cus, knobs);

  rn_potgnn *hp = h.get();
  rc = guarded<rn_potgnn>(nullptr, [&]() {
    HIP_TRY(hipSetDevice(cfg->device));
    HIP_TRY(hipEventCreateWithFlags(&hp->ev_start, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&hp->ev_g[0], hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&hp->ev_g[1], hipEventDisableTiming));
    hp->g = upload(hp->plan, hp->g_ints);
    double ms[18];
    std::memcpy(ms, hp->mean, sizeof(hp->mean));
    std::memcpy(ms + 9, hp->stdv, sizeof(hp->stdv));
    hp->d_mean_std.ensure(sizeof(ms));
    HIP_TRY(hipMemcpy(hp->d_mean_std.p, ms, sizeof(ms), hipMemcpyHostToDevice));
    hp->lay = layout_weights(hp->cfg, hp->d);
    pack_weights(hp->lay, weights, hp->packed);
    refresh_mfma_mode(hp);
    hp->ps_fail.ensure(2048);  // [0] the failure word; timing builds (RN_PS_TIMING) keep their cycle counters from byte 64 on
    HIP_TRY(hipMemset(hp->ps_fail.p, 0, 2048));
    size_chunk(hp);
    ensure_precision<float>(hp);
  });
  if (rc != RN_OK) return rc;
  *out = h.release();
  return RN_OK;
}

int rn_potgnn_debug_plan(const rn_potgnn_config *cfg, const int32_t *edge_a, const int32_t *edge_b,
                         const int32_t *atom_types, int32_t num_cus, int32_t *out, size_t capacity, size_t *count) {
  if (!count || num_cus <= 0) return RN_ERR_INVALID_ARGUMENT;
  *count = 0;
  std::string invalid;
  const int rc = validate_create_args(cfg, edge_a, edge_b, atom_types, false, nullptr, invalid);
  if (rc != RN_OK) {
    set_error<rn_potgnn>(nullptr, "%s", invalid.c_str());
    return rc;
  }
  try {
    const PlanKnobs knobs = read_plan_knobs();
    const std::vector<int32_t> flat = plan_graph(*cfg, plan_dims(*cfg, knobs), edge_a, edge_b, atom_types, num_cus, knobs).flat();
    *count = flat.size();
    if (!out || capacity < flat.size()) {
      set_error<rn_potgnn>(nullptr, "out holds %zu values, the plan has %zu", out ? capacity : (size_t)0, flat.size());
      return RN_ERR_INVALID_ARGUMENT;
    }
    std::memcpy(out, flat.data(), flat.size() * sizeof(int32_t));
    return RN_OK;
  } catch (const std::bad_alloc &) {
    set_error<rn_potgnn>(nullptr, "host allocation failed");
    return RN_ERR_OUT_OF_MEMORY;
  }
}

int rn_potgnn_debug_plan_pairs(const rn_potgnn_config *cfg, const int32_t *edge_a, const int32_t *edge_b,
                               const int32_t *atom_types, int32_t num_cus, int32_t *out, size_t capacity, size_t *count) {
  if (!count || num_cus <= 0) return RN_ERR_INVALID_ARGUMENT;
  *count = 0;
  std::string invalid;
  const int rc = validate_create_args(cfg, edge_a, edge_b, atom_types, false, nullptr, invalid);
  if (rc != RN_OK) {
    set_error<rn_potgnn>(nullptr, "%s", invalid.c_str());
    return rc;
  }
  try {
    const PlanKnobs knobs = read_plan_knobs();
    const std::vector<int32_t> flat = plan_graph(*cfg, plan_dims(*cfg, knobs), edge_a, edge_b, atom_types, num_cus, knobs).flat_pairs();
    *count = flat.size();
    if (!out || capacity < flat.size()) {
      set_error<rn_potgnn>(nullptr, "out holds %zu values, the pair table has %zu", out ? capacity : (size_t)0, flat.size());
      return RN_ERR_INVALID_ARGUMENT;
    }
    std::memcpy(out, flat.data(), flat.size() * sizeof(int32_t));
    return RN_OK;
  } catch (const std::bad_alloc &) {
    set_error<rn_potgnn>(nullptr, "host allocation failed");
    return RN_ERR_OUT_OF_MEMORY;
  }
}

int rn_potgnn_debug_plan_lds(const rn_potgnn_config *cfg, const int32_t *edge_a, const int32_t *edge_b,
                             const int32_t *atom_types, int32_t num_cus, int64_t *out, size_t capacity, size_t *count) {
  if (!count || num_cus <= 0) return RN_ERR_INVALID_ARGUMENT;
  *count = 0;
  std::string invalid;
  const int rc = validate_create_args(cfg, edge_a, edge_b, atom_types, false, nullptr, invalid);
  if (rc != RN_OK) {
    set_error<rn_potgnn>(nullptr, "%s", invalid.c_str());
    return rc;
  }
  try {
    const PlanKnobs knobs = read_plan_knobs();
    const std::vector<int64_t> lds = plan_graph(*cfg, plan_dims(*cfg, knobs), edge_a, edge_b, atom_types, num_cus, knobs).lds_requests();
    *count = lds.size();
    if (!out || capacity < lds.size()) {
      set_error<rn_potgnn>(nullptr, "out holds %zu values, the table has %zu", out ? capacity : (size_t)0, lds.size());
      return RN_ERR_INVALID_ARGUMENT;
    }
    std::memcpy(out, lds.data(), lds.size() * sizeof(int64_t));
    return RN_OK;
  } catch (const std::bad_alloc &) {
    set_error<rn_potgnn>(nullptr, "host allocation failed");
    return RN_ERR_OUT_OF_MEMORY;
  }
}

// The packed layout of a model of `cfg` alone (no graph), after the configuration checks of rn_potgnn_create.
static int debug_layout(const rn_potgnn_config *cfg, bool others_null, const size_t *num_weights, PackedLayout &L) {
  std::string invalid;
  const int rc = validate_config(cfg, others_null, num_weights, invalid);
  if (rc != RN_OK) {
    set_error<rn_potgnn>(nullptr, "%s", invalid.c_str());
    return rc;
  }
  L = layout_weights(*cfg, plan_dims(*cfg, read_plan_knobs()));
  return RN_OK;
}
static int debug_failed(const std::exception &e) {
  const bool memory = dynamic_cast<const std::bad_alloc *>(&e) != nullptr;
  set_error<rn_potgnn>(nullptr, memory ? "host allocation failed" : "internal error: %s", e.what());
  return memory ? RN_ERR_OUT_OF_MEMORY : RN_ERR_HIP;
}

int rn_potgnn_debug_pack_weights(const rn_potgnn_config *cfg, const float *weights, size_t num_weights, float *packed,
                                 unsigned char *mask, unsigned char *writers, int32_t *flags, size_t capacity, size_t *count) {
  if (!count) return RN_ERR_INVALID_ARGUMENT;
  *count = 0;
  try {
    PackedLayout L;
    if (const int rc = debug_layout(cfg, !weights, &num_weights, L); rc != RN_OK) return rc;
    *count = L.total;
    if (!packed || !mask || !flags || capacity < L.total) {
      set_error<rn_potgnn>(nullptr, "out holds %zu values, the packed blob has %zu", packed && mask && flags ? capacity : (size_t)0, L.total);
      return RN_ERR_INVALID_ARGUMENT;
    }
    std::vector<float> o;
    pack_weights(L, weights, o);
    std::memcpy(packed, o.data(), o.size() * sizeof(float));
    const std::vector<unsigned char> m = trainable_mask(L);
    std::memcpy(mask, m.data(), m.size());
    if (writers) {
      const std::vector<unsigned char> w = packed_writers(L);
      std::memcpy(writers, w.data(), w.size());
    }
    flags[0] = mfma_f16_range_ok(L, o.data(), false);
    for (int p = 0; p < L.P; ++p) {
      flags[1 + p] = folded_gate_ok(L, o.data(), p);
      (void)L.c3_norm_1(p), (void)L.mfma_scales(p);  // (throw when the layout broke what rn_potgnn_adam_step fetches in one piece)
    }
    (void)L.readout();
    return RN_OK;
  } catch (const std::exception &e) {
    return debug_failed(e);
  }
}

int rn_potgnn_debug_unpack_weights(const rn_potgnn_config *cfg, const float *packed, size_t num_packed, int buffers,
                                   float *out, size_t capacity, size_t *count) {
  if (!count) return RN_ERR_INVALID_ARGUMENT;
  *count = 0;
  try {
    PackedLayout L;
    if (const int rc = debug_layout(cfg, !packed, nullptr, L); rc != RN_OK) return rc;
    *count = L.weight_count();
    if (num_packed != L.total) {
      set_error<rn_potgnn>(nullptr, "packed has %zu floats, expected %zu", num_packed, L.total);
      return RN_ERR_INVALID_ARGUMENT;
    }
    if (!out || capacity < L.weight_count()) {
      set_error<rn_potgnn>(nullptr, "out holds %zu values, the state dict has %zu", out ? capacity : (size_t)0, L.weight_count());
      return RN_ERR_INVALID_ARGUMENT;
    }
    unpack_weights<float>(L, packed, out, buffers != 0);
    return RN_OK;
  } catch (const std::exception &e) {
    return debug_failed(e);
  }
}

void rn_potgnn_destroy(rn_potgnn *h) {
  if (!h) return;
  (void)hipSetDevice(h->cfg.device);
  (void)hipDeviceSynchronize();
  resolve_timers(h);
  for (int l = 0; l < 2; ++l) {
    if (h->f32.lanes[l].stream) (void)hipStreamDestroy(h->f32.lanes[l].stream);
    if (h->f32.lanes[l].done) (void)hipEventDestroy(h->f32.lanes[l].done);
    if (h->f64.lanes[l].stream) (void)hipStreamDestroy(h->f64.lanes[l].stream);
    if (h->f64.lanes[l].done) (void)hipEventDestroy(h->f64.lanes[l].done);
  }
  if (h->f32.side) (void)hipStreamDestroy(h->f32.side);
  if (h->f64.side) (void)hipStreamDestroy(h->f64.side);
  for (int i = 0; i < 3; ++i) {
    if (h->f32.ev_side[i]) (void)hipEventDestroy(h->f32.ev_side[i]);
    if (h->f64.ev_side[i]) (void)hipEventDestroy(h->f64.ev_side[i]);
  }
  for (auto &sl : h->slots) {
    if (sl.copied) (void)hipEventDestroy(sl.copied);
    if (sl.done) (void)hipEventDestroy(sl.done);
  }
  if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
  if (h->exec_stream) (void)hipStreamDestroy(h->exec_stream);
  if (h->ev_start) (void)hipEventDestroy(h->ev_start);
  for (int i = 0; i < 2; ++i)
    if (h->ev_g[i]) (void)hipEventDestroy(h->ev_g[i]);
  if (h->step_host) (void)hipHostFree(h->step_host);
  for (int b = 0; b < 2; ++b) {
    if (h->hstage.pin[b]) (void)hipHostFree(h->hstage.pin[b]);
    if (h->hstage.copied[b]) (void)hipEventDestroy(h->hstage.copied[b]);
  }
  if (h->hstage.done) (void)hipEventDestroy(h->hstage.done);
  if (h->hstage.caller) (void)hipEventDestroy(h->hstage.caller);
  if (h->hstage.out_pin) (void)hipHostFree(h->hstage.out_pin);
  delete h;
}

// float64 -> float32, round to nearest even: what the device's (float)double does.  Large batches on a few threads
// (the cast reads 8 and writes 4 bytes per coordinate: at the narrow models' rates one core is the bottleneck).
static void cast_to_float(const double *src, float *dst, size_t n) {
  auto run = [](const double *s, float *d, size_t m) {
    for (size_t i = 0; i < m; ++i) d[i] = (float)s[i];
  };
  const size_t per_thread = (size_t)1 << 17;  // (1 MiB of float64 per thread and more: a 1250-frame block of a trajectory that is
                                              //  not in the CPU's caches casts at DRAM rate, ~1 ms on one core, 0.3 on four)
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const size_t nt = std::min<size_t>(std::min<size_t>(4, hw), n / per_thread);
  if (nt < 2) return run(src, dst, n);
  std::vector<std::thread> pool;
  const size_t share = (n + nt - 1) / nt;
  for (size_t t = 1; t < nt; ++t) {
    const size_t lo = t * share, hi = std::min(n, lo + share);
    if (lo < hi) pool.emplace_back(run, src + lo, dst + lo, hi - lo);
  }
  run(src, dst, std::min(n, share));
  for (auto &t : pool) t.join();
}

// Float32 evaluation of caller-owned (usually pageable) float64 host positions into a device array of polarizabilities.
// A float32 evaluation casts the positions to float32 before any arithmetic (_gnn.py:709), so they are cast HERE, into
// page-locked staging, and cross PCIe as float32: half the bytes, no pageable copy, and results bit-identical to a float64
// upload.  The batch goes through in pieces (below: whole work chunks): this thread casts piece k + 1 while piece k crosses
// PCIe on the copy stream and the kernels of piece k - 1 run on the handle's streams behind h->exec_stream.
// `lattices` (host float64 [S][9], or null: the reference structure's): a lattice per frame, cast like the positions -- each
// piece's lattices are cast into the same page-locked piece, behind its positions, and copied with them.
static void staged_forward(rn_potgnn *h, const double *positions, const double *lattices, int64_t S, double *d_alpha, bool sync) {
  const size_t per_frame = (size_t)h->cfg.num_atoms * 3;
  const size_t pin_frame = per_frame + (lattices ? 9 : 0);  // floats of a frame in a page-locked piece
  const int64_t chunk = std::max<int64_t>(1, h->chunk);
  lazy_stream(h->exec_stream);
  lazy_stream(h->copy_stream);
  // Pieces are whole work chunks: a batch that fits one chunk goes through in ONE piece.  Measured on config 3's 1250-frame
  // share of an 8-GPU run (profiles/r06/host_boundary.txt): with the positions crossing as float32 from page-locked memory the
  // cast + copy of the whole block is 0.3 ms of 20, and every extra launch of the persistent kernels costs more in tails than
  // overlapping it saves -- one piece 0.994 of the resident rate, two 0.97, three 0.95, four equal ones 0.93 (round 5, a pageable
  // float64 copy in front of the kernels: 0.76).  Longer batches overlap naturally: piece k + 1 is cast and copied under the
  // kernels of piece k.  RN_POTGNN_HOST_PIECE = frames per piece (the bit-identity test forces small ones).
  int64_t fixed_piece = (S + ((S + chunk - 1) / chunk) - 1) / ((S + chunk - 1) / chunk);  // (equal pieces: forward_device's rule)
  if (const char *e = getenv("RN_POTGNN_HOST_PIECE")) fixed_piece = std::max<int64_t>(1, std::min<int64_t>(chunk, atoll(e)));
  std::vector<int64_t> pieces;
  for (int64_t left = S; left > 0; left -= pieces.back()) pieces.push_back(std::min<int64_t>(fixed_piece, left));
  const int64_t piece = *std::max_element(pieces.begin(), pieces.end());
  auto &hs = h->hstage;
  // A previous call through the to-device entry returned with its copies and kernels still enqueued: its staging buffers
  // must have left the host before they are overwritten, and its kernels must have read their float32 positions before
  // this call's copies land in the same device buffer.
  for (int b = 0; b < 2; ++b)
    if (hs.copied[b]) HIP_TRY(hipEventSynchronize(hs.copied[b]));
  if (hs.done) HIP_TRY(hipStreamWaitEvent(h->copy_stream, hs.done, 0));
  if (hs.elems < (size_t)piece * pin_frame) {
    for (int b = 0; b < 2; ++b) {
      if (hs.pin[b]) (void)hipHostFree(hs.pin[b]);
      hs.pin[b] = nullptr;
      HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&hs.pin[b]), (size_t)piece * pin_frame * sizeof(float), hipHostMallocDefault));
      lazy_event(hs.copied[b]);
    }
    hs.elems = (size_t)piece * pin_frame;
  }
  const size_t pos_bytes = (size_t)S * per_frame * sizeof(float);
  if (hs.pos.bytes < pos_bytes && hs.done) HIP_TRY(hipEventSynchronize(hs.done));  // (growing frees what it may still read)
  hs.pos.ensure(pos_bytes);
  float *d_pos32 = hs.pos.as<float>();
  float *d_lat32 = nullptr;
  if (lattices) {
    const size_t lat_bytes = (size_t)S * 9 * sizeof(float);
    if (hs.lat.bytes < lat_bytes && hs.done) HIP_TRY(hipEventSynchronize(hs.done));
    hs.lat.ensure(lat_bytes);
    d_lat32 = hs.lat.as<float>();
  }
  int b = 0;
  int64_t first = 0;
  static const bool timing = getenv("RN_POTGNN_HOST_TIMING") && atoi(getenv("RN_POTGNN_HOST_TIMING")) != 0;
  auto now = []() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_begin = now();
  double t_cast = 0, t_wait = 0;
  for (size_t k = 0; k < pieces.size(); first += pieces[k], ++k, b ^= 1) {
    const int64_t n = pieces[k];
    const double t0 = now();
    if (k >= 2) HIP_TRY(hipEventSynchronize(hs.copied[b]));  // this buffer's previous copy has left it
    const double t1 = now();
    cast_to_float(positions + first * per_frame, hs.pin[b], (size_t)n * per_frame);
    t_wait += t1 - t0;
    t_cast += now() - t1;
    HIP_TRY(hipMemcpyAsync(d_pos32 + first * per_frame, hs.pin[b], (size_t)n * per_frame * sizeof(float), hipMemcpyHostToDevice,
                           h->copy_stream));
    if (lattices) {
      float *pin_lat = hs.pin[b] + (size_t)n * per_frame;
      for (int64_t i = 0; i < n * 9; ++i) pin_lat[i] = (float)lattices[first * 9 + i];
      HIP_TRY(hipMemcpyAsync(d_lat32 + first * 9, pin_lat, (size_t)n * 9 * sizeof(float), hipMemcpyHostToDevice, h->copy_stream));
    }
    HIP_TRY(hipEventRecord(hs.copied[b], h->copy_stream));
    HIP_TRY(hipStreamWaitEvent(h->exec_stream, hs.copied[b], 0));
    ForwardIO<float> io;
    io.pos32 = d_pos32 + first * per_frame;
    io.lat = lattices ? d_lat32 + first * 9 : nullptr;
    io.alpha = d_alpha + first * 9;
    forward_device<float>(h, io, n, h->exec_stream, sync && first + n >= S);
  }
  lazy_event(hs.done);
  HIP_TRY(hipEventRecord(hs.done, h->exec_stream));  // (everything this call enqueued, on every lane, precedes it)
  if (timing)
    fprintf(stderr, "[host timing] S=%lld pieces=%zu total %.0f us: cast %.0f, buffer waits %.0f, rest (enqueue%s) %.0f\n", (long long)S,
            pieces.size(), now() - t_begin, t_cast, t_wait, sync ? " + final sync" : "", now() - t_begin - t_cast - t_wait);
}

int rn_potgnn_forward_device(rn_potgnn *h, const double *d_positions, int64_t S, double *d_alpha,
                             float *d_vec6, void *stream, int synchronize) {
  if (const int rc = check_batch(h, S, {d_positions}, "invalid positions / S"); rc != kGo) return rc;
  return guarded(h, [&]() {
    ForwardIO<float> io;
    io.pos = d_positions;
    io.alpha = d_alpha;
    io.vec6 = d_vec6;
    forward_device<float>(h, io, S, (hipStream_t)stream, synchronize != 0);
  });
}

int rn_potgnn_forward_device_f64(rn_potgnn *h, const double *d_positions, int64_t S, double *d_alpha,
                                 void *stream, int synchronize) {
  if (const int rc = check_batch(h, S, {d_positions, d_alpha}, "invalid positions / alpha / S"); rc != kGo) return rc;
  return guarded(h, [&]() {
    sync_host(h);  // the float64 copy of the weights is made from the host master copy
    ForwardIO<double> io;
    io.pos = d_positions;
    io.alpha = d_alpha;
    forward_device<double>(h, io, S, (hipStream_t)stream, synchronize != 0);
  });
}

// The float32 host-to-host evaluation behind rn_potgnn_calc_polarizabilities and, with lattices, its _cells form.
static int host_polarizabilities(rn_potgnn *h, const double *positions, const double *lattices, int64_t S, double *alpha) {
  return guarded(h, [&]() {
    const size_t per_frame = (size_t)h->cfg.num_atoms * 3;
    h->io_alpha.ensure((size_t)S * 9 * sizeof(double));
    lazy_stream(h->exec_stream);
    const int64_t chunk = std::max<int64_t>(1, h->chunk);
    static const bool stage_f32 = !(getenv("RN_POTGNN_HOST_F32") && atoi(getenv("RN_POTGNN_HOST_F32")) == 0);
    if (!stage_f32 && !lattices) {
      // (the round-5 form, kept for A/B runs: float64 positions, one blocking copy per work chunk)
      h->io_pos.ensure((size_t)S * per_frame * sizeof(double));
      for (int64_t first = 0; first < S; first += chunk) {
        const int64_t n = std::min<int64_t>(chunk, S - first);
        double *d_pos = h->io_pos.as<double>() + first * per_frame;
        HIP_TRY(hipMemcpy(d_pos, positions + first * per_frame, (size_t)n * per_frame * sizeof(double), hipMemcpyHostToDevice));
        ForwardIO<float> io;
        io.pos = d_pos;
        io.alpha = h->io_alpha.as<double>() + first * 9;
        forward_device<float>(h, io, n, h->exec_stream, first + n >= S);
      }
      HIP_TRY(hipMemcpy(alpha, h->io_alpha.p, (size_t)S * 9 * sizeof(double), hipMemcpyDeviceToHost));
      return;
    }
    // ONE synchronisation per call: the result and the role-specialised EdgeBlock's time-out word come down into page-locked
    // memory behind the kernels (a blocking hipMemcpy each, after a stream synchronisation of its own, was 30 of the ~450 us
    // of a one-structure call: the reference's unchanged Phonons loop makes 2 M of those, dynamics/_phonon.py:93-106)
    staged_forward(h, positions, lattices, S, h->io_alpha.as<double>(), false);
    auto &hs = h->hstage;
    const size_t out_bytes = (size_t)S * 9 * sizeof(double);
    if (hs.out_bytes < out_bytes + 16) {
      if (hs.out_pin) (void)hipHostFree(hs.out_pin);
      hs.out_pin = nullptr;
      hs.out_bytes = 0;
      HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&hs.out_pin), out_bytes + 16, hipHostMallocDefault));
      hs.out_bytes = out_bytes + 16;
    }
    int *fail_pin = reinterpret_cast<int *>(hs.out_pin + out_bytes);
    *fail_pin = 0;
    HIP_TRY(hipMemcpyAsync(hs.out_pin, h->io_alpha.p, out_bytes, hipMemcpyDeviceToHost, h->exec_stream));
    const bool watch = h->plan.use_ps && h->ps_fail.p;
    if (watch) HIP_TRY(hipMemcpyAsync(fail_pin, h->ps_fail.p, sizeof(int), hipMemcpyDeviceToHost, h->exec_stream));
    HIP_TRY(hipStreamSynchronize(h->exec_stream));
    resolve_timers(h);
    if (watch && *fail_pin != 0) check_ps_fail(h);  // (reads the word again, clears it and throws)
    std::memcpy(alpha, hs.out_pin, out_bytes);
  });
}

int rn_potgnn_calc_polarizabilities(rn_potgnn *h, const double *positions, int64_t S,
                                    double *alpha) {
  if (const int rc = check_batch(h, S, {positions, alpha}, "invalid positions / alpha / S"); rc != kGo) return rc;
  return host_polarizabilities(h, positions, nullptr, S, alpha);
}

static int host_polarizabilities_f64(rn_potgnn *h, const double *positions, const double *lattices, int64_t S, double *alpha);

int rn_potgnn_calc_polarizabilities_cells(rn_potgnn *h, const double *positions, const double *lattices, int64_t S,
                                          int use_float64, double *alpha) {
  if (const int rc = check_batch(h, S, {positions, alpha}, "invalid positions / alpha / S"); rc != kGo) return rc;
  if (const int rc = check_lattices(h, lattices, S); rc != kGo) return rc;
  return use_float64 ? host_polarizabilities_f64(h, positions, lattices, S, alpha)
                     : host_polarizabilities(h, positions, lattices, S, alpha);
}

static int host_polarizabilities_to_device(rn_potgnn *h, const double *positions, const double *lattices, int64_t S,
                                           double *d_alpha, void *stream) {
  return guarded(h, [&]() {
    // The evaluation starts behind what the caller queued on `stream` before the call: an earlier reader of d_alpha (the
    // previous all-gather on the same tensor, the last user of a block torch's caching allocator handed out again).
    auto &hs = h->hstage;
    lazy_stream(h->exec_stream);
    lazy_event(hs.caller);
    HIP_TRY(hipEventRecord(hs.caller, (hipStream_t)stream));
    HIP_TRY(hipStreamWaitEvent(h->exec_stream, hs.caller, 0));
    staged_forward(h, positions, lattices, S, d_alpha, false);
    // the caller's stream continues behind the evaluation (e.g. the RCCL all-gather of ramannoodle_amd.parallel)
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, hs.done, 0));
  });
}

int rn_potgnn_calc_polarizabilities_to_device(rn_potgnn *h, const double *positions, int64_t S, double *d_alpha, void *stream) {
  if (const int rc = check_batch(h, S, {positions, d_alpha}, "invalid positions / d_alpha / S"); rc != kGo) return rc;
  return host_polarizabilities_to_device(h, positions, nullptr, S, d_alpha, stream);
}

int rn_potgnn_calc_polarizabilities_cells_to_device(rn_potgnn *h, const double *positions, const double *lattices, int64_t S,
                                                    double *d_alpha, void *stream) {
  if (const int rc = check_batch(h, S, {positions, d_alpha}, "invalid positions / d_alpha / S"); rc != kGo) return rc;
  if (const int rc = check_lattices(h, lattices, S); rc != kGo) return rc;
  return host_polarizabilities_to_device(h, positions, lattices, S, d_alpha, stream);
}

int rn_potgnn_forward_cells_device(rn_potgnn *h, const double *d_positions, const double *d_lattices, int64_t S, int use_float64,
                                   double *d_alpha, void *stream, int synchronize) {
  if (const int rc = check_batch(h, S, {d_positions, d_alpha}, "invalid positions / alpha / S"); rc != kGo) return rc;
  if (!d_lattices)
    return use_float64 ? rn_potgnn_forward_device_f64(h, d_positions, S, d_alpha, stream, synchronize)
                       : rn_potgnn_forward_device(h, d_positions, S, d_alpha, nullptr, stream, synchronize);
  return guarded(h, [&]() {
    hipStream_t user = (hipStream_t)stream;
    if (use_float64) {
      sync_host(h);  // the float64 copy of the weights is made from the host master copy
      ForwardIO<double> io;
      io.pos = d_positions;
      io.lat = d_lattices;
      io.alpha = d_alpha;
      forward_device<double>(h, io, S, user, synchronize != 0);
      return;
    }
    // float32: the lattices are cast on the caller's stream into a buffer of the handle's, behind the kernels of an
    // earlier call that may still read it (every entry leaves its lanes' `done` recorded behind its last kernel)
    ensure_precision<float>(h);
    for (auto &ln : h->f32.lanes)
      if (ln.done) HIP_TRY(hipStreamWaitEvent(user, ln.done, 0));
    h->cells_lat.ensure((size_t)S * 9 * sizeof(float));
    launch_cast_from_f64<float>(d_lattices, h->cells_lat.as<float>(), S * 9, user);
    ForwardIO<float> io;
    io.pos = d_positions;
    io.lat = h->cells_lat.as<float>();
    io.alpha = d_alpha;
    forward_device<float>(h, io, S, user, synchronize != 0);
  });
}

int rn_potgnn_calc_polarizabilities_f64(rn_potgnn *h, const double *positions, int64_t S, double *alpha) {
  if (const int rc = check_batch(h, S, {positions, alpha}, "invalid positions / alpha / S"); rc != kGo) return rc;
  return host_polarizabilities_f64(h, positions, nullptr, S, alpha);
}

static int host_polarizabilities_f64(rn_potgnn *h, const double *positions, const double *lattices, int64_t S, double *alpha) {
  return guarded(h, [&]() {
    sync_host(h);  // the float64 copy of the weights is made from the host master copy
    ForwardIO<double> io;
    io.pos = stage<double>(h->io_pos, positions, (size_t)S * h->cfg.num_atoms * 3 * sizeof(double));
    io.lat = stage_lattices<double>(h, lattices, S);
    h->io_alpha.ensure((size_t)S * 9 * sizeof(double));
    io.alpha = h->io_alpha.as<double>();
    forward_device<double>(h, io, S, nullptr, true);
    HIP_TRY(hipMemcpy(alpha, h->io_alpha.p, (size_t)S * 9 * sizeof(double), hipMemcpyDeviceToHost));
  });
}

int rn_potgnn_calc_polarizabilities_async(rn_potgnn *h, const double *positions, int64_t S, double *alpha) {
  if (const int rc = check_batch(h, S, {positions, alpha}, "invalid positions / alpha / S"); rc != kGo) return rc;
  return guarded(h, [&]() {
    lazy_stream(h->copy_stream);  // (the streams may exist already: the synchronous host entry uses them too)
    lazy_stream(h->exec_stream);
    for (auto &sl : h->slots) {
      lazy_event(sl.copied);
      lazy_event(sl.done);
    }
    auto &sl = h->slots[h->next_slot];
    h->next_slot ^= 1;
    if (sl.busy) HIP_TRY(hipEventSynchronize(sl.done));  // its staging buffers are about to be reused
    const size_t pb = (size_t)S * h->cfg.num_atoms * 3 * sizeof(double);
    sl.pos.ensure(pb);
    sl.alpha.ensure((size_t)S * 9 * sizeof(double));
    HIP_TRY(hipMemcpyAsync(sl.pos.p, positions, pb, hipMemcpyHostToDevice, h->copy_stream));
    HIP_TRY(hipEventRecord(sl.copied, h->copy_stream));
    HIP_TRY(hipStreamWaitEvent(h->exec_stream, sl.copied, 0));
    ForwardIO<float> io;
    io.pos = sl.pos.as<double>();
    io.alpha = sl.alpha.as<double>();
    forward_device<float>(h, io, S, h->exec_stream, false);
    HIP_TRY(hipMemcpyAsync(alpha, sl.alpha.p, (size_t)S * 9 * sizeof(double), hipMemcpyDeviceToHost,
                           h->exec_stream));
    HIP_TRY(hipEventRecord(sl.done, h->exec_stream));
    sl.busy = true;
  });
}

int rn_potgnn_wait(rn_potgnn *h) {
  if (!h) return RN_ERR_INVALID_ARGUMENT;
  return guarded(h, [&]() {
    for (auto &sl : h->slots)
      if (sl.busy) {
        HIP_TRY(hipEventSynchronize(sl.done));
        sl.busy = false;
      }
    resolve_timers(h);
    check_ps_fail(h);
  });
}

int rn_host_buffer_alloc(size_t bytes, int device, void **out) {
  if (!out || bytes == 0) return RN_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    set_error<rn_potgnn>(nullptr, "no usable HIP device (count=%d, requested=%d)", ndev, device);
    return RN_ERR_NO_DEVICE;
  }
  return guarded<rn_potgnn>(nullptr, [&]() {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocPortable));
  });
}

void rn_host_buffer_free(void *p) {
  if (p) (void)hipHostFree(p);
}

int rn_potgnn_forward(rn_potgnn *h, const double *positions, int64_t S, float *vec6) {
  return rn_potgnn_forward_samples(h, nullptr, nullptr, positions, S, vec6);
}

int rn_potgnn_forward_lattices(rn_potgnn *h, const double *lattices, const double *positions, int64_t S,
                               float *vec6) {
  if (const int rc = check_batch(h, S, {lattices, positions, vec6}, "invalid lattices / positions / vec6 / S"); rc != kGo) return rc;
  return rn_potgnn_forward_samples(h, lattices, nullptr, positions, S, vec6);
}

int rn_potgnn_forward_samples(rn_potgnn *h, const double *lattices, const int32_t *atom_types,
                              const double *positions, int64_t S, float *vec6) {
  if (const int rc = check_batch(h, S, {positions, vec6}, "invalid positions / vec6 / S"); rc != kGo) return rc;
  if (const int rc = check_types(h, atom_types, S); rc != kGo) return rc;
  return guarded(h, [&]() {
    ForwardIO<float> io;
    io.pos = stage<double>(h->io_pos, positions, (size_t)S * h->cfg.num_atoms * 3 * sizeof(double));
    io.lat = stage_lattices<float>(h, lattices, S);  // the reference's forward computes in float32
    io.types = stage_types(h, atom_types, S);
    h->io_vec6.ensure((size_t)S * 6 * sizeof(float));
    io.vec6 = h->io_vec6.as<float>();
    forward_device<float>(h, io, S, nullptr, true);
    HIP_TRY(hipMemcpy(vec6, h->io_vec6.p, (size_t)S * 6 * sizeof(float), hipMemcpyDeviceToHost));
  });
}

int rn_potgnn_forward_samples_f64(rn_potgnn *h, const double *lattices, const int32_t *atom_types,
                                  const double *positions, int64_t S, double *vec6) {
  if (const int rc = check_batch(h, S, {positions, vec6}, "invalid positions / vec6 / S"); rc != kGo) return rc;
  if (const int rc = check_types(h, atom_types, S); rc != kGo) return rc;
  return guarded(h, [&]() {
    sync_host(h);  // the float64 copy of the weights is made from the host master copy
    ForwardIO<double> io;
    io.pos = stage<double>(h->io_pos, positions, (size_t)S * h->cfg.num_atoms * 3 * sizeof(double));
    io.lat = stage_lattices<double>(h, lattices, S);
    io.types = stage_types(h, atom_types, S);
    // the standardised tensor (what PotGNN.forward returns as a 6-vector) is the reduction's value before alpha * sigma + mu
    h->io_alpha.ensure((size_t)S * 9 * sizeof(double));
    io.alpha_raw = h->io_alpha.as<double>();
    forward_device<double>(h, io, S, nullptr, true);
    std::vector<double> raw((size_t)S * 9);
    HIP_TRY(hipMemcpy(raw.data(), h->io_alpha.p, raw.size() * sizeof(double), hipMemcpyDeviceToHost));
    const int pick[6] = {0, 4, 8, 1, 2, 5};  // (xx, yy, zz, xy, xz, yz): dataset/torch/utils.py:44-60
    for (int64_t s = 0; s < S; ++s)
      for (int k = 0; k < 6; ++k) vec6[s * 6 + k] = raw[(size_t)s * 9 + pick[k]];
  });
}

int rn_potgnn_raman_tensors(rn_potgnn *h, const double *ref_positions, const double *displacements,
                            int64_t M, double delta, double *raman) {
  if (!h) return RN_ERR_INVALID_ARGUMENT;
  if (M < 0 || delta == 0.0 || !ref_positions || (M > 0 && (!displacements || !raman))) {
    set_error(h, "invalid arguments to raman_tensors");
    return RN_ERR_INVALID_ARGUMENT;
  }
  if (M == 0) return RN_OK;
  return guarded(h, [&]() {
    const size_t n3 = (size_t)h->cfg.num_atoms * 3;
    // frames 2m / 2m+1 = ref +/- delta * d_m   (_phonon.py:95-101)
    std::vector<double> pos((size_t)2 * M * n3);
    for (int64_t m = 0; m < M; ++m)
      for (size_t i = 0; i < n3; ++i) {
        const double eps = displacements[m * n3 + i] * delta;
        pos[(2 * m) * n3 + i] = ref_positions[i] + eps;
        pos[(2 * m + 1) * n3 + i] = ref_positions[i] - eps;
      }
    sync_host(h);  // (device-resident training may have moved the weights ahead of the float64 copy)
    ForwardIO<double> io;
    io.pos = stage<double>(h->io_pos, pos.data(), pos.size() * sizeof(double));
    h->io_alpha.ensure((size_t)2 * M * 9 * sizeof(double));
    io.alpha = h->io_alpha.as<double>();
    forward_device<double>(h, io, 2 * M, nullptr, true);
    std::vector<double> a((size_t)2 * M * 9);
    HIP_TRY(hipMemcpy(a.data(), h->io_alpha.p, a.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t m = 0; m < M; ++m)
      for (int i = 0; i < 9; ++i)
        raman[m * 9 + i] = (a[(2 * m) * 9 + i] - a[(2 * m + 1) * 9 + i]) / delta;  // _phonon.py:106
  });
}

int rn_potgnn_alpha_jacobian(rn_potgnn *h, const double *positions, int use_float64, double *jac) {
  if (!h || !positions || !jac) {
    set_error(h, "invalid arguments to alpha_jacobian");
    return RN_ERR_INVALID_ARGUMENT;
  }
  return guarded(h, [&]() { with_precision(h, use_float64, [&](auto t) { jacobian<decltype(t)>(h, positions, jac); }); });
}

int rn_potgnn_raman_tensors_analytic(rn_potgnn *h, const double *ref_positions,
                                     const double *displacements, int64_t M, double *raman) {
  if (!h || M < 0 || !ref_positions || (M > 0 && (!displacements || !raman))) {
    set_error(h, "invalid arguments to raman_tensors_analytic");
    return RN_ERR_INVALID_ARGUMENT;
  }
  if (M == 0) return RN_OK;
  return guarded(h, [&]() {
    const size_t n3 = (size_t)h->cfg.num_atoms * 3;
    std::vector<double> jac(6 * n3);
    sync_host(h);
    jacobian<double>(h, ref_positions, jac.data());
    // R_m = 2 * sigma (.) (J d_m): the reference divides its +-delta difference by delta, not
    // 2 delta (dynamics/_phonon.py:106), i.e. it returns twice the directional derivative
    const int map[9] = {0, 3, 4, 3, 1, 5, 4, 5, 2};
    for (int64_t m = 0; m < M; ++m) {
      double v[6] = {0, 0, 0, 0, 0, 0};
      const double *dm = displacements + m * n3;
      for (int k = 0; k < 6; ++k) {
        const double *j = jac.data() + k * n3;
        double acc = 0;
        for (size_t i = 0; i < n3; ++i) acc += j[i] * dm[i];
        v[k] = acc;
      }
      for (int i = 0; i < 9; ++i) raman[m * 9 + i] = 2.0 * h->stdv[i] * v[map[i]];
    }
  });
}

int rn_potgnn_set_weights(rn_potgnn *h, const float *weights, size_t num_weights) {
  if (!h || !weights || num_weights != h->lay.weight_count()) {
    set_error(h, "invalid arguments to set_weights");
    return RN_ERR_INVALID_ARGUMENT;
  }
  return guarded(h, [&]() {
    HIP_TRY(hipDeviceSynchronize());
    pack_weights(h->lay, weights, h->packed);
    refresh_mfma_mode(h);
    h->host_stale = false;
    h->grads_on_device = false;
    if (h->f32.ready) upload_weights<float>(h);
    if (h->f64.ready) upload_weights<double>(h);
  });
}

int rn_potgnn_train_forward(rn_potgnn *h, const double *positions, int64_t S, float *vec6,
                            float *batch_mean, float *batch_var) {
  const Checked c = check_train_batch(h, S, {positions, vec6, batch_mean, batch_var}, "train_forward", kHostF32);
  if (c.rc != kGo) return c.rc;
  return guarded(h, [&]() { train_forward<float>(h, positions, (int)S, vec6, batch_mean, batch_var); });
}

int rn_potgnn_train_forward_samples(rn_potgnn *h, const double *lattices, const int32_t *atom_types, const double *positions,
                                    int64_t S, float *vec6, float *batch_mean, float *batch_var) {
  const Checked c = check_train_batch(h, S, {positions, vec6, batch_mean, batch_var}, "train_forward_samples", kHostF32);
  if (c.rc != kGo) return c.rc;
  if (const int rc = check_types(h, atom_types, S); rc != kGo) return rc;
  return guarded(h, [&]() { train_forward<float>(h, positions, (int)S, vec6, batch_mean, batch_var, lattices, atom_types); });
}

int rn_potgnn_train_forward_samples_f64(rn_potgnn *h, const double *lattices, const int32_t *atom_types,
                                        const double *positions, int64_t S, double *vec6, double *batch_mean,
                                        double *batch_var) {
  const Checked c = check_train_batch(h, S, {positions, vec6, batch_mean, batch_var}, "train_forward_samples_f64", kHostF64);
  if (c.rc != kGo) return c.rc;
  if (const int rc = check_types(h, atom_types, S); rc != kGo) return rc;
  return guarded(h, [&]() {
    sync_host(h);
    train_forward<double>(h, positions, (int)S, vec6, batch_mean, batch_var, lattices, atom_types);
  });
}

int rn_potgnn_train_forward_samples_device(rn_potgnn *h, const float *d_lattices, const int32_t *d_atom_types,
                                           const double *d_positions, int64_t S, float *d_vec6, void *stream) {
  const Checked c = check_train_batch(h, S, {d_positions, d_vec6}, "train_forward_samples_device", kDeviceF32);
  if (c.rc != kGo) return c.rc;
  return guarded(h, [&]() { train_forward_device(h, d_positions, (int)S, d_lattices, d_atom_types, d_vec6, (hipStream_t)stream); });
}

int rn_potgnn_train_backward_samples_device(rn_potgnn *h, const float *d_dvec6, void *stream) {
  const Checked c = check_pending(h, d_dvec6, "train_backward_samples_device", kDeviceF32,
                                  "train_backward_samples_device needs device-resident training and a preceding float32 train_forward");
  if (c.rc != kGo) return c.rc;
  return guarded(h, [&]() { train_backward_device(h, d_dvec6, (hipStream_t)stream); });
}

int rn_potgnn_forward_samples_device(rn_potgnn *h, const float *d_lattices, const int32_t *d_atom_types,
                                     const double *d_positions, int64_t S, float *d_vec6, void *stream, int synchronize) {
  if (const int rc = check_batch(h, S, {d_positions, d_vec6}, "invalid positions / vec6 / S"); rc != kGo) return rc;
  return guarded(h, [&]() {
    ForwardIO<float> io;
    io.pos = d_positions;
    io.lat = d_lattices;
    io.types = d_atom_types;
    io.vec6 = d_vec6;
    forward_device<float>(h, io, S, (hipStream_t)stream, synchronize != 0);
  });
}

int rn_potgnn_forward_vjp_device(rn_potgnn *h, const double *d_lattices, const int32_t *d_atom_types,
                                 const double *d_positions, int64_t S, const double *d_dvec6, int use_float64,
                                 double *d_dpos, double *d_dlat, void *stream) {
  if (!h) return RN_ERR_INVALID_ARGUMENT;
  if (S < 0 || (S > 0 && (!d_positions || !d_dvec6)) || (!d_dpos && !d_dlat)) {
    set_error(h, "invalid arguments to forward_vjp_device (positions, cotangents, S, or neither dpos nor dlat)");
    return RN_ERR_INVALID_ARGUMENT;
  }
  if (S == 0) return RN_OK;
  return guarded(h, [&]() {
    with_precision(h, use_float64, [&](auto t) {
      forward_vjp<decltype(t)>(h, d_lattices, d_atom_types, d_positions, S, d_dvec6, d_dpos, d_dlat, (hipStream_t)stream);
    });
  });
}

int rn_potgnn_group_increments_device(rn_potgnn *h, const double *d_positions, int64_t S, const int32_t *labels, int G,
                                      int use_float64, size_t workspace_limit, double *d_out, void *stream) {
  if (const int rc = check_group_entry(h, S, d_positions, labels, d_out, G)) return rc;
  return guarded(h, [&]() {
    h->groups.set(h, "group_increments_device", labels, h->g.N, G, nullptr);
    const size_t limit = workspace_limit ? workspace_limit : kTapeBudget;
    with_precision(h, use_float64, [&](auto t) {
      group_increments<decltype(t)>(h, d_positions, S, G, limit, d_out, (hipStream_t)stream);
    });
  });
}

int rn_potgnn_group_increments_cells_device(rn_potgnn *h, const double *d_positions, const double *d_lattices, int64_t S,
                                            const int32_t *labels, int G, int use_float64, size_t workspace_limit,
                                            double *d_out, void *stream) {
  if (!d_lattices) return rn_potgnn_group_increments_device(h, d_positions, S, labels, G, use_float64, workspace_limit, d_out, stream);
  if (!h) return RN_ERR_INVALID_ARGUMENT;
  if (S < 2 || !d_positions || !labels || !d_out || G < 1 || G + 1 > kMaxGroups) {
    set_error(h, "invalid arguments to group_increments_cells_device (S < 2, G outside 1..%d -- the cell is one more channel -- "
                 "or a null pointer)", kMaxGroups - 1);
    return RN_ERR_INVALID_ARGUMENT;
  }
  return guarded(h, [&]() {
    h->groups.set(h, "group_increments_cells_device", labels, h->g.N, G, nullptr);
    const size_t limit = workspace_limit ? workspace_limit : kTapeBudget;
    with_precision(h, use_float64, [&](auto t) {
      group_increments<decltype(t)>(h, d_positions, S, G, limit, d_out, (hipStream_t)stream, d_lattices);
    });
  });
}

int rn_potgnn_mode_contract_device(const double *d_jac, int64_t frames, const double *d_positions, int32_t N,
                                   const double *d_disp, const double *d_proj, int32_t M, const double *sigma, int rest,
                                   int out_channels, double *d_out, void *stream) {
  if (!d_jac || !d_positions || !d_disp || !d_proj || !sigma || !d_out) return RN_ERR_INVALID_ARGUMENT;
  if (frames < 2 || N < 1 || M < 1 || M > kMaxModes || (rest != 0 && rest != 1)) return RN_ERR_INVALID_ARGUMENT;
  if ((int64_t)out_channels < (int64_t)M + rest) return RN_ERR_INVALID_ARGUMENT;
  return guarded<rn_potgnn>(nullptr, [&]() {
    hipStream_t st = (hipStream_t)stream;
    DeviceBuf d_sigma;
    d_sigma.ensure(9 * sizeof(double));
    HIP_TRY(hipMemcpyAsync(d_sigma.p, sigma, 9 * sizeof(double), hipMemcpyHostToDevice, st));
    mode_contract(d_jac, frames, d_positions, N, d_disp, d_proj, M, d_sigma.as<double>(), rest != 0, out_channels, d_out, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));  // (sigma's copy is freed on return)
  });
}

int rn_potgnn_mode_increments_device(rn_potgnn *h, const double *d_positions, const double *d_lattices, int64_t S,
                                     const double *disp, const double *proj, int32_t M, int rest, int use_float64,
                                     size_t workspace_limit, double *d_out, void *stream) {
  if (const int rc = check_mode_entry(h, S, d_positions, disp, proj, d_out, M, rest)) return rc;
  if (const int rc = check_mode_vectors(h, disp, proj, M, h->g.N)) return rc;
  return guarded(h, [&]() {
    const size_t limit = workspace_limit ? workspace_limit : kTapeBudget;
    with_precision(h, use_float64, [&](auto t) {
      mode_increments<decltype(t)>(h, d_positions, S, disp, proj, M, rest != 0, limit, d_out, (hipStream_t)stream, d_lattices);
    });
  });
}

int rn_potgnn_partial_raman_tensors(rn_potgnn *h, const double *ref_positions, const double *displacements, int64_t M,
                                    const int32_t *labels, int G, double *raman) {
  if (const int rc = check_partial_raman_entry(h, ref_positions, displacements, M, labels, G, raman)) return rc;
  return guarded(h, [&]() {
    h->groups.set(h, "partial_raman_tensors", labels, h->g.N, G, nullptr);
    if (M == 0) return;
    sync_host(h);  // (device-resident training may have moved the weights ahead of the float64 copy)
    ensure_precision<double>(h);
    h->train_S = 0;  // the tape and lane 0 are reused: a pending train_forward is void
    const int N = h->g.N;
    const size_t n3 = (size_t)N * 3;
    hipStream_t st = h->f64.lanes[0].stream;
    HIP_TRY(hipStreamSynchronize(st));  // (io_pos and the staging below are filled from the null stream)
    h->grp_out.ensure((size_t)M * G * 9 * sizeof(double));
    h->grp_jac.ensure(6 * n3 * sizeof(double));
    const double *d_ref = stage<double>(h->io_pos, ref_positions, n3 * sizeof(double));
    stage<double>(h->grp_disp, displacements, (size_t)M * n3 * sizeof(double));
    jacobian_rows<double>(h, d_ref, 1, h->grp_jac.as<double>());
    // R[m][g] = 2 sigma (.) sum_{i in g} J_i . d_{m,i}: the kernel's 1/2 (J + J) . (2 d)
    const int *perm = h->groups.perm();
    launch_group_increments(h->grp_jac.as<double>(), 0, nullptr, h->grp_disp.as<double>(), 2.0, M, N, perm, perm + N, G,
                            h->d_mean_std.as<double>() + 9, h->grp_out.as<double>(), st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    check_ps_fail(h);
    HIP_TRY(hipMemcpy(raman, h->grp_out.p, (size_t)M * G * 9 * sizeof(double), hipMemcpyDeviceToHost));
  });
}

int rn_potgnn_train_backward_inputs(rn_potgnn *h, const float *dvec6, float *grads, double *dpos, double *dlat) {
  const Checked c = check_pending(h, dvec6 && (dpos || dlat), "train_backward_inputs", kHostF32,
                                  "train_backward_inputs needs a preceding train_forward (an evaluation or Jacobian call in "
                                  "between discards its tape)");
  if (c.rc != kGo) return c.rc;
  return guarded(h, [&]() { train_backward<float>(h, dvec6, grads, dpos, dlat); });
}

int rn_potgnn_train_backward_inputs_device(rn_potgnn *h, const float *d_dvec6, double *d_dpos, double *d_dlat,
                                           void *stream) {
  const Checked c = check_pending(h, d_dvec6 && (d_dpos || d_dlat), "train_backward_inputs_device", kDeviceF32,
                                  "train_backward_inputs_device needs device-resident training and a preceding float32 train_forward");
  if (c.rc != kGo) return c.rc;
  return guarded(h, [&]() { train_backward_device(h, d_dvec6, (hipStream_t)stream, d_dpos, d_dlat); });
}

int rn_potgnn_train_forward_f64(rn_potgnn *h, const double *positions, int64_t S, double *vec6,
                                double *batch_mean, double *batch_var) {
  const Checked c = check_train_batch(h, S, {positions, vec6, batch_mean, batch_var}, "train_forward_f64", kHostF64);
  if (c.rc != kGo) return c.rc;
  return guarded(h, [&]() {
    sync_host(h);
    train_forward<double>(h, positions, (int)S, vec6, batch_mean, batch_var);
  });
}

int rn_potgnn_train_backward_f64(rn_potgnn *h, const double *dvec6, double *grads) {
  const Checked c = check_pending(h, dvec6 && grads, "train_backward_f64", kHostF64,
                                  "train_backward_f64 needs a preceding train_forward_f64");
  if (c.rc != kGo) return c.rc;
  return guarded(h, [&]() { train_backward<double>(h, dvec6, grads); });
}

int rn_potgnn_set_device_training(rn_potgnn *h, int enabled) {
  if (!h) return RN_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::recursive_mutex> hold(h->lock);  // (the checks below read handle state)
  h->device_training = enabled != 0;
  return RN_OK;
}

int rn_potgnn_train_backward_device(rn_potgnn *h, const float *dvec6) {
  const Checked c = check_pending(h, dvec6, "train_backward_device", kHostF32,
                                  "train_backward_device needs a preceding train_forward (an evaluation or Jacobian call "
                                  "in between discards its tape)");
  if (c.rc != kGo) return c.rc;
  return guarded(h, [&]() { train_backward<float>(h, dvec6, nullptr); });
}

int rn_potgnn_gradient_buffer(rn_potgnn *h, void **device_ptr, size_t *count) {
  if (!h || !device_ptr || !count || !h->grads_on_device) {
    set_error(h, "no gradients on the device (call rn_potgnn_train_backward_device first)");
    return RN_ERR_INVALID_ARGUMENT;
  }
  *device_ptr = h->f32.grad.p;
  *count = h->lay.total;
  return RN_OK;
}

int rn_potgnn_adam_step(rn_potgnn *h, double lr, double beta1, double beta2, double eps, double weight_decay,
                        int64_t step) {
  if (!h || step < 1 || !(lr >= 0) || !(eps >= 0)) {
    set_error(h, "invalid arguments to adam_step");
    return RN_ERR_INVALID_ARGUMENT;
  }
  std::lock_guard<std::recursive_mutex> hold(h->lock);  // (the checks below read handle state)
  if (!h->grads_on_device) {
    set_error(h, "adam_step needs the gradients of a preceding train_backward_device");
    return RN_ERR_INVALID_ARGUMENT;
  }
  return guarded(h, [&]() {
    Precision<float> &P = h->f32;
    const PackedLayout &L = h->lay;
    const size_t n = L.total;
    hipStream_t st = P.lanes[0].stream;
    if (!h->trainable_mask.p) {  // first step: moments, mask and the table of derived ranges
      h->adam_m.ensure(n * sizeof(float));
      h->adam_v.ensure(n * sizeof(float));
      HIP_TRY(hipMemset(h->adam_m.p, 0, n * sizeof(float)));
      HIP_TRY(hipMemset(h->adam_v.p, 0, n * sizeof(float)));
      const std::vector<unsigned char> mask = trainable_mask(L);
      h->trainable_mask.ensure(mask.size());
      HIP_TRY(hipMemcpy(h->trainable_mask.p, mask.data(), mask.size(), hipMemcpyHostToDevice));
      const std::vector<DerivedOp> ops = derived_ops(L, &h->derived_first_stage);
      h->derived_ops.ensure(ops.size() * sizeof(DerivedOp));
      HIP_TRY(hipMemcpy(h->derived_ops.p, ops.data(), ops.size() * sizeof(DerivedOp), hipMemcpyHostToDevice));
      h->num_derived_ops = (int)ops.size();
    }
    float *w = P.weights.as<float>();
    after_other_lanes(h, st);
    launch_adam(w, P.grad.as<float>(), h->adam_m.as<float>(), h->adam_v.as<float>(),
                h->trainable_mask.as<unsigned char>(), n, lr, beta1, beta2, eps, weight_decay, step, st,
                (h->plan.use_ps && h->ps_fail.p) ? h->ps_fail.as<int>() : nullptr);
    launch_refresh_derived(w, h->derived_ops.as<DerivedOp>(), h->derived_first_stage, st);
    launch_refresh_derived(w, h->derived_ops.as<DerivedOp>() + h->derived_first_stage, h->num_derived_ops - h->derived_first_stage, st);
    device_setup<float>(h, w, st);
    HIP_TRY(hipGetLastError());
    // The host looks at three kinds of entries after a step: c3_norm_1's folded constants (the triplet loop's folded-scale
    // variant is chosen from them), the prescale pairs (which double as the finiteness flags of the weight blocks,
    // mfma_f16_range_ok) and the readout block of the split-f16 range guard.  One gather kernel + ONE download into pinned
    // memory (2 P + 1 separate small downloads cost a round trip each: 0.2 ms of a 0.3 ms step).
    {
      std::vector<long long> seg;
      long long total = 0;
      auto add = [&](Span s) {
        seg.push_back((long long)s.begin);
        seg.push_back(total);
        seg.push_back((long long)s.count);
        total += (long long)s.count;
      };
      for (int p = 0; p < L.P; ++p) {
        add(L.c3_norm_1(p));    // the folded-gate criterion reads gamma and beta
        add(L.mfma_scales(p));  // the prescale pairs double as finiteness flags
      }
      add(L.readout());
      if (h->step_seg.bytes < seg.size() * sizeof(long long)) {
        h->step_seg.ensure(seg.size() * sizeof(long long));
        HIP_TRY(hipMemcpy(h->step_seg.p, seg.data(), seg.size() * sizeof(long long), hipMemcpyHostToDevice));
        h->step_stage.ensure((size_t)total * sizeof(float));
        if (h->step_host) (void)hipHostFree(h->step_host);
        h->step_host = nullptr;
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&h->step_host), (size_t)total * sizeof(float), hipHostMallocDefault));
      }
      launch_gather_segments(w, h->step_seg.as<long long>(), (int)(seg.size() / 3), h->step_stage.as<float>(), st);
      HIP_TRY(hipMemcpyAsync(h->step_host, h->step_stage.p, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      for (size_t i = 0; i < seg.size(); i += 3)
        std::memcpy(h->packed.data() + seg[i], h->step_host + seg[i + 1], (size_t)seg[i + 2] * sizeof(float));
    }
    HIP_TRY(hipStreamSynchronize(st));
    // The taped forward of this step ran the role-specialised EdgeBlock and nothing has looked at its time-out word since.  If it
    // is set the Adam kernel has applied nothing (it reads the same word), so weights, moments and the host mirror are those of
    // before the step; the gradients are void either way and the handle says so before the error leaves.
    h->grads_on_device = false;
    h->train_S = 0;
    h->host_stale = true;
    refresh_pass_flags<float>(h);
    refresh_mfma_mode(h);
    check_ps_fail(h);
  });
}

int rn_potgnn_get_weights(rn_potgnn *h, float *weights, size_t num_weights) {
  if (!h || !weights || num_weights != h->lay.weight_count()) {
    set_error(h, "invalid arguments to get_weights");
    return RN_ERR_INVALID_ARGUMENT;
  }
  return guarded(h, [&]() {
    sync_host(h);
    unpack_weights<float>(h->lay, h->packed.data(), weights, true);
  });
}

int rn_potgnn_set_stat_reducer(rn_potgnn *h, rn_potgnn_reduce_fn fn, void *ctx) {
  if (!h) return RN_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::recursive_mutex> hold(h->lock);
  h->reducer = fn;
  h->reducer_ctx = ctx;
  return RN_OK;
}

double rn_potgnn_train_row_count(const rn_potgnn *h) {
  if (!h) return 0.0;
  std::lock_guard<std::recursive_mutex> hold(h->lock);
  return h->bn_count;
}

int rn_potgnn_train_backward(rn_potgnn *h, const float *dvec6, float *grads) {
  const Checked c = check_pending(h, dvec6 && grads, "train_backward", kHostF32,
                                  "train_backward needs a preceding train_forward (an evaluation or Jacobian call in "
                                  "between discards its tape)");
  if (c.rc != kGo) return c.rc;
  return guarded(h, [&]() { train_backward<float>(h, dvec6, grads); });
}

int rn_potgnn_radius_graph(const double *lattice, const double *positions, int32_t num_atoms,
                           double cutoff, int device, uint8_t *adjacency) {
  if (!lattice || !positions || !adjacency || num_atoms <= 0 || !(cutoff > 0)) {
    set_error<rn_potgnn>(nullptr, "invalid arguments to radius_graph");
    return RN_ERR_INVALID_ARGUMENT;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    set_error<rn_potgnn>(nullptr, "no usable HIP device (count=%d, requested=%d)", ndev, device);
    return RN_ERR_NO_DEVICE;
  }
  return guarded<rn_potgnn>(nullptr, [&]() {
    HIP_TRY(hipSetDevice(device));
    const size_t n = (size_t)num_atoms;
    DeviceBuf lat, pos, adj;
    lat.ensure(9 * sizeof(double));
    pos.ensure(n * 3 * sizeof(double));
    adj.ensure(n * n);
    HIP_TRY(hipMemcpy(lat.p, lattice, 9 * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(pos.p, positions, n * 3 * sizeof(double), hipMemcpyHostToDevice));
    launch_radius_graph(lat.as<double>(), pos.as<double>(), num_atoms, (float)cutoff,
                        adj.as<unsigned char>(), nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(adjacency, adj.p, n * n, hipMemcpyDeviceToHost));
  });
}

int rn_potgnn_config_flags(const rn_potgnn *h) {
  if (!h) return -1;
  std::lock_guard<std::recursive_mutex> hold(h->lock);  // (the pass flags are rewritten when weights change)
  int flags = (h->plan.use_fused ? 1 : 0) | ((h->plan.use_fused && h->mfma_f16) ? 4 : 0) | (h->plan.use_narrow ? 8 : 0) |
              ((h->plan.use_fused && h->mfma_range_fallback) ? 16 : 0);
  {  // bit 8: every pass of a float32 evaluation takes the role-specialised EdgeBlock (kernels_edge_ps.hip)
    bool ps = h->plan.use_fused && h->plan.use_ps && !h->f32.pass.empty();  // (split-f16 or exact-f32 products: the same kernel)
    for (const auto &p : h->f32.pass) ps = ps && (p.c3_fast & 1);
    flags |= ps ? 256 : 0;
  }
  {  // bit 9: float32 evaluations take the atom-owning fused NodeBlock (kernels_node_atom.hip)
    static const bool centred = !(getenv("RN_POTGNN_NODE_CENTRED") && atoi(getenv("RN_POTGNN_NODE_CENTRED")) == 0);
    const bool atom = h->plan.use_fused && h->plan.use_node_fused && h->mfma_f16 && centred && h->g.na_num > 0;
    flags |= atom ? 512 : 0;
    // bit 10: float32 evaluations keep their edge rows as split-f16 pairs (bits 8 and 9 and the fused readout)
    flags |= (atom && (flags & 256) && h->plan.use_readout_fused && h->want_pair_rows && !h->keep_stages) ? 1024 : 0;
    // bit 11: such evaluations compute the EdgeBlock's c2 branch once per atom pair (kernels_c2_pairs.hip)
    flags |= ((flags & 1024) && h->want_c2_pairs && c2_rows_fit(h)) ? 2048 : 0;
  }
  bool fast = !h->f32.pass.empty();
  for (const auto &p : h->f32.pass) fast = fast && !h->plan.use_narrow && (p.c3_fast & (h->plan.use_fused ? 1 : 2));
  return flags | (fast ? 2 : 0);
}

int rn_potgnn_debug_ps_schedule(const int32_t *rb, const int32_t *re, int32_t num_destinations, int32_t back, int32_t ring_tiles,
                                int32_t *window) {
  if (!rb || !re || num_destinations < 0 || back < 1 || back > 8 || ring_tiles < 1 || ring_tiles > 64) return RN_ERR_INVALID_ARGUMENT;
  int w = 0;
  const bool ok = edge_ps_tile_ok(rb, re, num_destinations, back, ring_tiles, &w);
  if (window) *window = w;
  return ok ? 1 : 0;
}

int64_t rn_potgnn_num_triplets(const rn_potgnn *h) { return h ? h->g.T : -1; }

int rn_potgnn_debug_triplets(rn_potgnn *h, int32_t *idx_i, int32_t *idx_j, int32_t *idx_k,
                             int32_t *slot5, int32_t *slot6) {
  if (!h || !idx_i || !idx_j || !idx_k || !slot5 || !slot6) return RN_ERR_INVALID_ARGUMENT;
  return guarded(h, [&]() {
    const size_t T = (size_t)h->g.T;
    if (T == 0) return;
    DeviceBuf buf;
    buf.ensure(5 * T * sizeof(int));
    int *p = buf.as<int>();
    launch_enum_triplets(h->g, p, p + T, p + 2 * T, p + 3 * T, p + 4 * T, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    int32_t *outs[5] = {idx_i, idx_j, idx_k, slot5, slot6};
    for (int k = 0; k < 5; ++k)
      HIP_TRY(hipMemcpy(outs[k], p + k * T, T * sizeof(int), hipMemcpyDeviceToHost));
  });
}

int rn_potgnn_debug_stage(rn_potgnn *h, int stage, int index, float *out, size_t out_capacity,
                          int64_t *rows, int64_t *cols) {
  if (!h || !out || !rows || !cols) return RN_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::recursive_mutex> hold(h->lock);  // (the checks below read handle state)
  if (h->last_was_f64) {
    set_error(h, "debug_stage only reads the float32 path");
    return RN_ERR_UNSUPPORTED;
  }
  const int S = h->last_chunk_structs;
  Precision<float> &P = h->f32;  // (debug use: evaluate <= one chunk so lane 0 holds it)
  return guarded(h, [&]() {
    HIP_TRY(hipDeviceSynchronize());
    const float *src = nullptr;
    int64_t r = 0, c = 0, ld = 0;
    const int64_t ME = (int64_t)S * h->g.E, MN = (int64_t)S * h->g.N;
    if (stage == 0) {
      src = P.lanes[0].unit4.as<float>(); r = ME; c = 4; ld = 4;
    } else if (stage == 1 || stage == 2) {
      if ((!h->keep_stages && !h->snap_pairs) || index < 0 || index > h->cfg.num_message_passes)
        throw HipError{hipErrorInvalidValue, "stage snapshots need RN_POTGNN_KEEP_STAGES=1 or 2"};
      if (stage == 1) { src = P.snap_node[index].as<float>(); r = MN; c = h->d.Fn; ld = h->d.FnP; }
      else { src = P.snap_edge[index].as<float>(); r = ME; c = h->d.Fe; ld = h->d.FeP; }
    } else if (stage == 3) {
      src = P.lanes[0].bufA.as<float>(); r = ME; c = 12; ld = 32;
    } else if (stage == 4) {  // stage 2's snapshot as it lies in memory: padded columns included, pair rows not decoded
      if ((!h->keep_stages && !h->snap_pairs) || index < 0 || index > h->cfg.num_message_passes)
        throw HipError{hipErrorInvalidValue, "stage snapshots need RN_POTGNN_KEEP_STAGES=1 or 2"};
      src = P.snap_edge[index].as<float>(); r = ME; c = h->d.FeP; ld = h->d.FeP;
    } else {
      throw HipError{hipErrorInvalidValue, "unknown stage"};
    }
    if ((size_t)(r * c) > out_capacity) throw HipError{hipErrorInvalidValue, "out_capacity too small"};
    if (stage == 2 && h->snap_pairs && h->last_pair_rows) {  // split-f16 pair rows (kernels.hpp: launch_geom_rbf_pairs): x = hi + lo
      std::vector<_Float16> raw((size_t)r * 128);
      HIP_TRY(hipMemcpy(raw.data(), src, raw.size() * sizeof(_Float16), hipMemcpyDeviceToHost));
      for (int64_t i = 0; i < r; ++i)
        for (int64_t k = 0; k < c; ++k) {
          const _Float16 *grp = raw.data() + i * 128 + (k >> 3) * 16;  // [hi x8][lo x8] of columns 8 m .. 8 m + 7
          out[i * c + k] = (float)grp[k & 7] + (float)grp[8 + (k & 7)];
        }
      *rows = r;
      *cols = c;
      return;
    }
    HIP_TRY(hipMemcpy2D(out, c * sizeof(float), src, ld * sizeof(float), c * sizeof(float), r,
                        hipMemcpyDeviceToHost));
    if (h->last_in_order && r == ME && stage != 1 && stage != 4) {  // per-edge rows of a narrow run: back to edge-id order
      std::vector<float> tmp(out, out + r * c);
      const int E = h->g.E;
      for (int64_t s = 0; s < S; ++s)
        for (int e = 0; e < E; ++e)
          std::memcpy(out + (s * E + e) * c, tmp.data() + (s * E + h->plan.in_pos[e]) * c, (size_t)c * sizeof(float));
    }
    *rows = r;
    *cols = c;
  });
}

int rn_potgnn_set_profiling(rn_potgnn *h, int enabled) {
  if (!h) return RN_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::recursive_mutex> hold(h->lock);
  resolve_timers(h);
  h->profiling = enabled;
  for (int k = 0; k < K_COUNT; ++k) {
    h->k_ms[k] = 0;
    h->k_launches[k] = 0;
  }
  return RN_OK;
}

int rn_potgnn_kernel_times(rn_potgnn *h, const char **names, double *millis, int64_t *launches,
                           int cap) {
  if (!h || !names || !millis || !launches) return RN_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::recursive_mutex> hold(h->lock);
  (void)hipSetDevice(h->cfg.device);
  resolve_timers(h);
  int n = 0;
  for (int k = 0; k < K_COUNT && n < cap; ++k, ++n) {
    names[n] = kKernelNames[k];
    millis[n] = h->k_ms[k];
    launches[n] = h->k_launches[k];
  }
  return n;
}

}  // extern "C"
