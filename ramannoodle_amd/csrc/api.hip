// The C ABI (include/rn_potgnn.h) of the gfx950 PotGNN evaluator: the extern "C" entries with their argument checks,
// create / destroy and the debug entries.  Host only.  The host layer by file:
//   handle.hpp        struct rn_potgnn and its per-precision state, the kernel timers, the run policy's value type
//   forward.hip       workspace sizing, weight upload, the run policy (choose), ChunkRun, forward_device, the staged host path
//   reverse.hip       the reverse pass and its users: Jacobian, input gradients, group and mode increments
//   training.hip      one training step: taped forward, BatchNorm statistics, backward, running statistics, Adam
//   forward.hpp       what those three give each other and this file
//   host_runtime.hpp  error types, the owners (DeviceBuf, Stream, Event, PinnedBuf), set_error and guarded()
//   increments.hpp    the group table, the mode upload, the chunk walk and the checks of the increment entries,
//                     shared with the interpolation model (api_interp.hip)
// Planning is host-only code in graph_plan.hip (rn_potgnn_debug_plan runs it without a device), the packed weight layout
// in weight_layout.hip (rn_potgnn_debug_pack_weights); this file uploads the plan, forward.hip the blob.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "forward.hpp"

using namespace rn;

static std::string g_create_error;
std::string &rn_potgnn::create_error() { return g_create_error; }

namespace rn {
const char *const kKernelNames[K_COUNT] = {
    "geom_rbf", "node_init", "proj_node", "proj_edge_c1", "node_agg", "proj_edge_c3",
    "proj_c2", "edge_agg", "readout_mlp", "readout_reduce", "c2_pairs"};
}

namespace {

// ---- what the entries share: argument checks (each returns kGo, or the status the entry returns at once)

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

// What a device entry evaluates: float64 positions, optional lattices (in T) and atom types, and the outputs asked for.
template <typename T>
ForwardIO<T> device_io(const double *pos, const T *lat, const int *types, double *alpha, float *vec6) {
  ForwardIO<T> io;
  io.pos = pos, io.lat = lat, io.types = types, io.alpha = alpha, io.vec6 = vec6;
  return io;
}

// RN_OK when `device` is one of the HIP devices of this process, else RN_ERR_NO_DEVICE with the text of a failed create.
int check_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev) return RN_OK;
  set_error<rn_potgnn>(nullptr, "no usable HIP device (count=%d, requested=%d)", ndev, device);
  return RN_ERR_NO_DEVICE;
}

// One table of the plan of a graph (the debug_plan entries; no device): `table(plan)` into out[capacity], its size into
// *count; `what` names it in the text of a capacity that is too small.
template <typename V, class Table>
int debug_plan_table(const rn_potgnn_config *cfg, const int32_t *edge_a, const int32_t *edge_b, const int32_t *atom_types,
                     int32_t num_cus, V *out, size_t capacity, size_t *count, const char *what, Table table) {
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
    const std::vector<V> flat = table(plan_graph(*cfg, plan_dims(*cfg, knobs), edge_a, edge_b, atom_types, num_cus, knobs));
    *count = flat.size();
    if (!out || capacity < flat.size()) {
      set_error<rn_potgnn>(nullptr, "out holds %zu values, the %s has %zu", out ? capacity : (size_t)0, what, flat.size());
      return RN_ERR_INVALID_ARGUMENT;
    }
    std::memcpy(out, flat.data(), flat.size() * sizeof(V));
    return RN_OK;
  } catch (const std::bad_alloc &) {
    set_error<rn_potgnn>(nullptr, "host allocation failed");
    return RN_ERR_OUT_OF_MEMORY;
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
// `arrays` pairs each host array with the Graph field that points at its device copy, in packing order.
static Graph upload(const GraphPlan &plan, DeviceBuf &buf) {
  const struct {
    const std::vector<int> &host;
    const int *Graph::*field;
  } arrays[] = {{plan.edge_a, &Graph::edge_a},     {plan.edge_b, &Graph::edge_b},     {plan.out_ptr, &Graph::out_ptr},
                {plan.in_ptr, &Graph::in_ptr},     {plan.in_edge, &Graph::in_edge},   {plan.atom_type, &Graph::atom_type},
                {plan.tile.begin, &Graph::tile_begin}, {plan.trip_off, &Graph::trip_off}, {plan.rev_edge, &Graph::rev_edge},
                {plan.nt.begin, &Graph::nt_begin}, {plan.bt.begin, &Graph::bt_begin}, {plan.pt.begin, &Graph::pt_begin},
                {plan.in_pos, &Graph::in_pos},     {plan.pair_of_edge, &Graph::pair_of_edge},
                {plan.pair_a, &Graph::pair_a},     {plan.pair_b, &Graph::pair_b}};
  std::vector<int> ints;
  std::vector<size_t> at;
  for (const auto &a : arrays) {
    at.push_back(ints.size());
    ints.insert(ints.end(), a.host.begin(), a.host.end());
    while (ints.size() % 4) ints.push_back(0);
  }
  buf.upload(ints.data(), ints.size() * sizeof(int));
  Graph g = plan.scalars();
  for (size_t k = 0; k < at.size(); ++k) g.*arrays[k].field = buf.as<int>() + at[k];
  return g;
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

  if (const int no = check_device(cfg->device)) return no;
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
  return debug_plan_table(cfg, edge_a, edge_b, atom_types, num_cus, out, capacity, count, "plan",
                          [](const GraphPlan &p) { return p.flat(); });
}

int rn_potgnn_debug_plan_pairs(const rn_potgnn_config *cfg, const int32_t *edge_a, const int32_t *edge_b,
                               const int32_t *atom_types, int32_t num_cus, int32_t *out, size_t capacity, size_t *count) {
  return debug_plan_table(cfg, edge_a, edge_b, atom_types, num_cus, out, capacity, count, "pair table",
                          [](const GraphPlan &p) { return p.flat_pairs(); });
}

int rn_potgnn_debug_plan_lds(const rn_potgnn_config *cfg, const int32_t *edge_a, const int32_t *edge_b,
                             const int32_t *atom_types, int32_t num_cus, int64_t *out, size_t capacity, size_t *count) {
  return debug_plan_table(cfg, edge_a, edge_b, atom_types, num_cus, out, capacity, count, "table",
                          [](const GraphPlan &p) { return p.lds_requests(); });
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
  delete h;
}

int rn_potgnn_forward_device(rn_potgnn *h, const double *d_positions, int64_t S, double *d_alpha,
                             float *d_vec6, void *stream, int synchronize) {
  if (const int rc = check_batch(h, S, {d_positions}, "invalid positions / S"); rc != kGo) return rc;
  return guarded(h, [&]() {
    forward_device<float>(h, device_io<float>(d_positions, nullptr, nullptr, d_alpha, d_vec6), S, (hipStream_t)stream, synchronize != 0);
  });
}

int rn_potgnn_forward_device_f64(rn_potgnn *h, const double *d_positions, int64_t S, double *d_alpha,
                                 void *stream, int synchronize) {
  if (const int rc = check_batch(h, S, {d_positions, d_alpha}, "invalid positions / alpha / S"); rc != kGo) return rc;
  return guarded(h, [&]() {
    sync_host(h);  // the float64 copy of the weights is made from the host master copy
    forward_device<double>(h, device_io<double>(d_positions, nullptr, nullptr, d_alpha, nullptr), S, (hipStream_t)stream, synchronize != 0);
  });
}

int rn_potgnn_calc_polarizabilities(rn_potgnn *h, const double *positions, int64_t S,
                                    double *alpha) {
  if (const int rc = check_batch(h, S, {positions, alpha}, "invalid positions / alpha / S"); rc != kGo) return rc;
  return guarded(h, [&]() { host_polarizabilities(h, positions, nullptr, S, alpha); });
}

static int host_polarizabilities_f64(rn_potgnn *h, const double *positions, const double *lattices, int64_t S, double *alpha) {
  return guarded(h, [&]() {
    sync_host(h);  // the float64 copy of the weights is made from the host master copy
    host_forward<double>(h, lattices, nullptr, positions, S, alpha, nullptr);
  });
}

int rn_potgnn_calc_polarizabilities_cells(rn_potgnn *h, const double *positions, const double *lattices, int64_t S,
                                          int use_float64, double *alpha) {
  if (const int rc = check_batch(h, S, {positions, alpha}, "invalid positions / alpha / S"); rc != kGo) return rc;
  if (const int rc = check_lattices(h, lattices, S); rc != kGo) return rc;
  if (use_float64) return host_polarizabilities_f64(h, positions, lattices, S, alpha);
  return guarded(h, [&]() { host_polarizabilities(h, positions, lattices, S, alpha); });
}

static int host_polarizabilities_to_device(rn_potgnn *h, const double *positions, const double *lattices, int64_t S,
                                           double *d_alpha, void *stream) {
  return guarded(h, [&]() {
    // The evaluation starts behind what the caller queued on `stream` before the call: an earlier reader of d_alpha (the
    // previous all-gather on the same tensor, the last user of a block torch's caching allocator handed out again).
    auto &hs = h->hstage;
    HIP_TRY(hipEventRecord(hs.caller.get(), (hipStream_t)stream));
    HIP_TRY(hipStreamWaitEvent(h->exec_stream.get(), hs.caller.get(), 0));
    staged_forward(h, positions, lattices, S, d_alpha, false);
    // the caller's stream continues behind the evaluation (e.g. the RCCL all-gather of ramannoodle_amd.parallel)
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, hs.done.get(), 0));
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
      forward_device<double>(h, device_io<double>(d_positions, d_lattices, nullptr, d_alpha, nullptr), S, user, synchronize != 0);
      return;
    }
    // float32: the lattices are cast on the caller's stream into a buffer of the handle's, behind the kernels of an
    // earlier call that may still read it (every entry leaves its lanes' `done` recorded behind its last kernel)
    ensure_precision<float>(h);
    for (auto &ln : h->f32.lanes)
      if (ln.done.e) HIP_TRY(hipStreamWaitEvent(user, ln.done.e, 0));
    h->cells_lat.ensure((size_t)S * 9 * sizeof(float));
    launch_cast_from_f64<float>(d_lattices, h->cells_lat.as<float>(), S * 9, user);
    forward_device<float>(h, device_io<float>(d_positions, h->cells_lat.as<float>(), nullptr, d_alpha, nullptr), S, user, synchronize != 0);
  });
}

int rn_potgnn_descriptors(rn_potgnn *h, const double *positions, const double *lattices, int64_t S, int use_float64,
                          double *desc, double *alpha) {
  if (const int rc = check_batch(h, S, {positions, desc}, "invalid positions / desc / S"); rc != kGo) return rc;
  if (const int rc = check_lattices(h, lattices, S); rc != kGo) return rc;
  return guarded(h, [&]() {
    with_precision(h, use_float64 != 0, [&](auto t) {
      host_descriptors<decltype(t)>(h, lattices, positions, S, desc, alpha);
    });
  });
}

int rn_potgnn_device_descriptors(rn_potgnn *h, const double *d_positions, const double *d_lattices, int64_t S, int use_float64,
                                 double *d_desc, double *d_alpha, void *stream) {
  if (const int rc = check_batch(h, S, {d_positions, d_desc}, "invalid positions / desc / S"); rc != kGo) return rc;
  return guarded(h, [&]() {
    hipStream_t user = (hipStream_t)stream;
    if (use_float64) {
      sync_host(h);  // the float64 copy of the weights is made from the host master copy
      ForwardIO<double> io = device_io<double>(d_positions, d_lattices, nullptr, d_alpha, nullptr);
      io.desc = d_desc;
      forward_device<double>(h, io, S, user, false);
      return;
    }
    const float *lat32 = nullptr;
    if (d_lattices) {  // cast on the caller's stream into the handle's buffer, as rn_potgnn_forward_cells_device does
      ensure_precision<float>(h);
      for (auto &ln : h->f32.lanes)
        if (ln.done.e) HIP_TRY(hipStreamWaitEvent(user, ln.done.e, 0));
      h->cells_lat.ensure((size_t)S * 9 * sizeof(float));
      launch_cast_from_f64<float>(d_lattices, h->cells_lat.as<float>(), S * 9, user);
      lat32 = h->cells_lat.as<float>();
    }
    ForwardIO<float> io = device_io<float>(d_positions, lat32, nullptr, d_alpha, nullptr);
    io.desc = d_desc;
    forward_device<float>(h, io, S, user, false);
  });
}

int rn_potgnn_calc_polarizabilities_f64(rn_potgnn *h, const double *positions, int64_t S, double *alpha) {
  if (const int rc = check_batch(h, S, {positions, alpha}, "invalid positions / alpha / S"); rc != kGo) return rc;
  return host_polarizabilities_f64(h, positions, nullptr, S, alpha);
}

int rn_potgnn_calc_polarizabilities_async(rn_potgnn *h, const double *positions, int64_t S, double *alpha) {
  if (const int rc = check_batch(h, S, {positions, alpha}, "invalid positions / alpha / S"); rc != kGo) return rc;
  return guarded(h, [&]() {
    hipStream_t copy = h->copy_stream.get(), exec = h->exec_stream.get();  // (the synchronous host entry uses them too)
    auto &sl = h->slots[h->next_slot];
    h->next_slot ^= 1;
    if (sl.busy) HIP_TRY(hipEventSynchronize(sl.done.get()));  // its staging buffers are about to be reused
    const size_t pb = (size_t)S * h->cfg.num_atoms * 3 * sizeof(double);
    sl.pos.ensure(pb);
    sl.alpha.ensure((size_t)S * 9 * sizeof(double));
    HIP_TRY(hipMemcpyAsync(sl.pos.p, positions, pb, hipMemcpyHostToDevice, copy));
    HIP_TRY(hipEventRecord(sl.copied.get(), copy));
    HIP_TRY(hipStreamWaitEvent(exec, sl.copied.get(), 0));
    forward_device<float>(h, device_io<float>(sl.pos.as<double>(), nullptr, nullptr, sl.alpha.as<double>(), nullptr), S, exec, false);
    HIP_TRY(hipMemcpyAsync(alpha, sl.alpha.p, (size_t)S * 9 * sizeof(double), hipMemcpyDeviceToHost, exec));
    HIP_TRY(hipEventRecord(sl.done.get(), exec));
    sl.busy = true;
  });
}

int rn_potgnn_wait(rn_potgnn *h) {
  if (!h) return RN_ERR_INVALID_ARGUMENT;
  return guarded(h, [&]() {
    for (auto &sl : h->slots)
      if (sl.busy) {
        HIP_TRY(hipEventSynchronize(sl.done.get()));
        sl.busy = false;
      }
    resolve_timers(h);
    check_ps_fail(h);
  });
}

int rn_host_buffer_alloc(size_t bytes, int device, void **out) {
  if (!out || bytes == 0) return RN_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (const int no = check_device(device)) return no;
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
  // (the reference's forward computes in float32: the lattices are cast to it)
  return guarded(h, [&]() { host_forward<float>(h, lattices, atom_types, positions, S, nullptr, vec6); });
}

int rn_potgnn_forward_samples_f64(rn_potgnn *h, const double *lattices, const int32_t *atom_types,
                                  const double *positions, int64_t S, double *vec6) {
  if (const int rc = check_batch(h, S, {positions, vec6}, "invalid positions / vec6 / S"); rc != kGo) return rc;
  if (const int rc = check_types(h, atom_types, S); rc != kGo) return rc;
  return guarded(h, [&]() {
    sync_host(h);  // the float64 copy of the weights is made from the host master copy
    host_forward<double>(h, lattices, atom_types, positions, S, nullptr, vec6);
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
    std::vector<double> a((size_t)2 * M * 9);
    host_forward<double>(h, nullptr, nullptr, pos.data(), 2 * M, a.data(), nullptr);
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
    forward_device<float>(h, device_io<float>(d_positions, d_lattices, d_atom_types, nullptr, d_vec6), S, (hipStream_t)stream, synchronize != 0);
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
    partial_raman(h, ref_positions, displacements, M, G, raman);
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
  return guarded(h, [&]() { adam_step(h, lr, beta1, beta2, eps, weight_decay, step); });
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
  if (const int no = check_device(device)) return no;
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
  // what a float32 evaluation takes (forward.hip: choose, the policy the run itself reads) -- bit 8: every pass the
  // role-specialised EdgeBlock; 9: the atom-owning fused NodeBlock; 10: edge rows as split-f16 pairs; 11: c2 once per atom pair
  const RunChoices c = choose(h, true, false);
  return (c.fused ? 1 : 0) | (c.folded_gate ? 2 : 0) | (c.split_f16 ? 4 : 0) | (c.narrow ? 8 : 0) | (c.range_fallback ? 16 : 0) |
         (c.every_pass_role_split ? 256 : 0) | (c.node_atom ? 512 : 0) | (c.pair_rows ? 1024 : 0) | (c.c2_pairs ? 2048 : 0);
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
  return guarded(h, [&]() { read_stage(h, stage, index, out, out_capacity, rows, cols); });
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
