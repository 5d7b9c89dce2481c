// The evaluator's handle (struct rn_potgnn) and what every host unit of the evaluator needs with it: the per-precision
// state, the kernel timers and the run policy.  Host only.
//
// A handle owns: the frozen graph (CSR both ways, node tiles, triplet offsets), the weights re-laid-out for the kernels
// (weight_layout.hpp), and per-"lane" device workspaces (a lane = a HIP stream).  Every stream, event and page-locked
// buffer is a member that releases itself (host_runtime.hpp), so deleting the handle frees all of it.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "graph_plan.hpp"
#include "host_runtime.hpp"
#include "increments.hpp"
#include "kernels.hpp"
#include "weight_layout.hpp"

namespace rn {

enum KernelId {
  K_GEOM = 0, K_NODE_INIT, K_PROJ_NODE, K_PROJ_EDGE_C1, K_NODE_AGG, K_PROJ_EDGE_C3, K_PROJ_C2,
  K_EDGE_AGG, K_READOUT_MLP, K_READOUT_REDUCE, K_C2_PAIRS, K_COUNT
};
extern const char *const kKernelNames[K_COUNT];  // (api.hip, next to rn_potgnn_kernel_times)

template <typename T>
struct Lane {
  Stream stream;
  Event done;
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
  Stream side;  // weight-gradient products of the reverse pass run here, beside the cotangent chain
  Event ev_side[3];
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

}  // namespace rn

struct rn_potgnn {
  mutable std::recursive_mutex lock;  // serialises the calls on this handle (guarded(), the small getters / setters, set_error)
  rn_potgnn_config cfg{};
  rn::Dims d{};
  int chunk = 1;
  size_t f64_budget = 0;  // workspace bytes the float64 lanes may take (0: what the float32 lanes were given)
  bool keep_stages = false;
  bool snap_pairs = false;      // RN_POTGNN_KEEP_STAGES=2: the same snapshots of a run that keeps its kernels (edge rows stay split-f16
                                // pairs where they would be; rn_potgnn_debug_stage decodes them); stage 3 is not kept
  bool last_pair_rows = false;  // the last float32 run's edge rows were split-f16 pairs
  bool debug_sync = false;  // RN_POTGNN_DEBUG_SYNC=1: synchronise + check after every kernel
  rn::GraphPlan plan;  // the graph's host arrays, its atom tiles, the kernel family and the lanes (graph_plan.hpp); `g` is its device image
  bool split_projections = true;  // RN_POTGNN_SPLIT_PROJ=0: the forward's stand-alone projections on the exact-f32 MFMA kernel
  bool want_pair_rows = true;   // RN_POTGNN_PAIR_ROWS at create time (rn::choose decides per run)
  bool want_c2_pairs = true;    // RN_POTGNN_C2_PAIRS at create time (rn::choose decides per run)
  rn::DeviceBuf step_seg, step_stage;  // segments / staging of the one download after a device-resident Adam step
  rn::PinnedBuf step_host;             // its pinned host image
  bool tape_ps = true;          // RN_POTGNN_TAPE_PS: taped float32 runs on the role-specialised EdgeBlock / atom-owning NodeBlock
  bool mfma_f16 = true;  // fused kernels: split-f16 MFMA products are in use (requested and inside the safe range)
  bool mfma_f16_requested = true;   // RN_POTGNN_MFMA=f32 at create time: exact-f32 MFMA everywhere
  bool mfma_range_fallback = false; // split-f16 was requested but the range guard (mfma_f16_range_ok) refused it
  rn::Graph g{};
  rn::DeviceBuf g_ints;
  rn::DeviceBuf ps_fail;  // [1] int: set by edge_block_ps_kernel when one of its bounded waits ran out
  double lattice[9], mean[9], stdv[9];
  rn::DeviceBuf d_mean_std;  // [18] double
  std::vector<float> packed;  // host packed weights (float master copy)
  rn::PackedLayout lay;
  rn::Precision<float> f32;
  rn::Precision<double> f64;
  // cached I/O staging for the host entry points
  rn::DeviceBuf io_pos, io_alpha, io_vec6, io_lat, io_types, io_desc;
  // pipelined host entry (rn_potgnn_calc_polarizabilities_async): two staging slots
  struct Slot {
    rn::DeviceBuf pos, alpha;
    rn::Event copied, done;
    bool busy = false;
  } slots[2];
  rn::Stream copy_stream, exec_stream;
  int next_slot = 0;
  // host entry rn_potgnn_calc_polarizabilities: two page-locked buffers the caller's float64 positions are cast into
  // (float32) piece by piece, each with the event of its host-to-device copy
  struct HostStage {
    rn::PinnedBuf pin[2];  // (grown together: equal sizes)
    rn::Event copied[2];
    rn::Event done;
    // The float32 positions on the device.  Only staged_forward writes them (behind `done`): a to-device call returns
    // with kernels that still read them, and the other host entries fill io_pos from the null stream, which does not
    // wait for the handle's non-blocking streams.
    rn::DeviceBuf pos;
    rn::DeviceBuf lat;  // the float32 lattices of a variable-cell call [S][9], under the same rules
    rn::Event caller;   // the to-device entry: the caller's stream up to the call
    rn::PinnedBuf out;  // the result (+ the EdgeBlock's time-out word) of the synchronous host entry
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
  rn::DeviceBuf adam_m, adam_v, trainable_mask, derived_ops;
  int num_derived_ops = 0, derived_first_stage = 0;  // (ops after the first stage read what it wrote: second launch)
  double bn_count = 0;  // rows the pending step's BatchNorm statistics cover (all ranks)
  rn_potgnn_reduce_fn reducer = nullptr;  // data-parallel training: sums doubles over ranks
  void *reducer_ctx = nullptr;
  bool last_was_f64 = false;
  bool last_in_order = false;  // the last run kept its edge rows in (b, a) order (narrow kernels)
  // profiling
  int profiling = 0;
  std::vector<rn::TimedLaunch> timed;
  double k_ms[rn::K_COUNT] = {0};
  int64_t k_launches[rn::K_COUNT] = {0};
  std::string error;
  rn::Event ev_start;
  rn::Event ev_g[2];  // "projection stage done" per lane (run_pair)
  bool interleave = true;
  // atom-group contractions: the CSR permutation of the last labels (perm [N] | gptr [G+1]), Jacobian rows, staging
  rn::GroupTable groups;
  rn::DeviceBuf grp_jac, grp_disp, grp_out;
  rn::DeviceBuf mode_vectors;  // rn_potgnn_mode_increments_device: D [M][N][3] | P [M][N][3]
  // variable-cell calls: the lattice rows of the Jacobian [frames][6][9], a trajectory's lattices in the arithmetic of a
  // float32 run (group increments), the float32 lattices of rn_potgnn_forward_cells_device
  rn::DeviceBuf grp_jl, grp_lat, cells_lat;
  int device_index() const { return cfg.device; }
  static std::string &create_error();  // (api.hip)
};

namespace rn {

template <typename T>
Precision<T> &prec(rn_potgnn *h);
template <>
inline Precision<float> &prec<float>(rn_potgnn *h) { return h->f32; }
template <>
inline Precision<double> &prec<double>(rn_potgnn *h) { return h->f64; }

// Which kernels a run takes: decided HERE for the run (ChunkRun reads it, once per chunk) and for what the handle
// reports (rn_potgnn_config_flags), from the plan, the create-time knobs, the weights' flags and whether the run is taped.
struct RunChoices {
  bool fused = false;         // the fused kernels (the fused EdgeBlock also serves taped float32 runs: RN_POTGNN_TAPE_FUSED)
  bool narrow = false;        // the narrow kernels (kernels_narrow.hip): evaluation runs only
  bool node_centred = false;  // the fused NodeBlock on the centred copy of c1_linear (split-f16 products)
  bool node_atom = false;     // ... in its atom-owning form (kernels_node_atom.hip)
  bool pair_rows = false;     // edge rows as split-f16 pairs: every kernel of the run speaks the format, nothing else looks
  bool split_f16 = false, range_fallback = false;  // the fused kernels' products: split-f16 in use / refused by the range guard
  bool folded_gate = false;   // every pass folds c3_norm_1's scale into the triplet loop's operands
  bool edge_ps = false;       // the role-specialised EdgeBlock (kernels_edge_ps.hip) serves this run ...
  bool role_split(int c3_fast) const { return edge_ps && (c3_fast & 1) != 0; }  // ... in a pass with the folded gate scale
  bool every_pass_role_split = false;
  bool c2_pairs = false;  // the EdgeBlock's c2 branch once per atom pair, in a kernel of its own (kernels_c2_pairs.hip):
                          // runs on pair rows only, which take the role-specialised EdgeBlock in every pass
};
RunChoices choose(const rn_potgnn *h, bool f32, bool taped);  // (forward.hip)

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

inline void resolve_timers(rn_potgnn *h) {
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

}  // namespace rn
