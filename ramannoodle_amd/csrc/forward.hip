// The forward engine of the evaluator: workspace sizing, weight upload, the run policy (choose), one chunk's stages on one
// lane (ChunkRun), the evaluation (forward_device) and the staged host path.  Host only: the kernels are kernels_*.hip.
//
// An evaluation walks the frames in chunks (hundreds to thousands of frames: large launches amortise launch gaps and
// tails).  The fused pipeline (kernels_fused.hip) uses one lane; the unfused one alternates chunks between two lanes so
// that the HBM-bound projections of one chunk overlap the VALU-bound aggregation of the other (run_pair).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "forward.hpp"

namespace rn {

// Frames per device work chunk in precision T.  The workspace budget is counted in bytes, so
// the float64 lanes (created on first use, next to the float32 ones) take half the frames.
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
static bool c2_rows_fit(const rn_potgnn *h) {
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

template <typename T>
static T *upload_packed(rn_potgnn *h) {  // the host master copy, in T, into the precision's weight blob
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
  device_setup<T>(h, upload_packed<T>(h), P.lanes[0].stream.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(P.lanes[0].stream.get()));
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
    (void)ln.stream.get(), (void)ln.done.get();  // (created here: after_other_lanes looks for the lanes that exist)
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
  device_setup<T>(h, w, P.lanes[0].stream.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(P.lanes[0].stream.get()));
  P.ready = true;
}

// The run policy (handle.hpp: RunChoices) of a float32 (`f32`) or float64 run, taped (training, Jacobian, increments) or not.
//  - The fused kernels also serve taped float32 runs: the EdgeBlock kernel records the one extra array the reverse pass
//    needs; RN_POTGNN_TAPE_FUSED=0 keeps those runs on the unfused kernels.
//  - The role-specialised EdgeBlock takes a pass with the folded gate scale, with split-f16 or exact-f32 products.  Taped
//    runs take it too (it records the pre-LayerNorm sums, and the reverse pass recomputes every projection from the taped
//    rows, so it never sees the centred copies); RN_POTGNN_TAPE_PS=0 keeps them on the per-frame kernel and the row-ordered
//    NodeBlock.
//  - Pair rows (kernels.hpp: launch_geom_rbf_pairs): when EVERY kernel that touches the edge rows in this run speaks the
//    format -- the role-specialised EdgeBlock in every pass, the atom-owning NodeBlock, the fused readout -- and nothing
//    else looks at them (no tape, no stage snapshots).  RN_POTGNN_PAIR_ROWS=0 keeps plain float32 rows.
//  - The pair kernel: runs on pair rows, on a graph whose pair rows fit the readout's buffer (c2_rows_fit); every other
//    run keeps c2 inside the EdgeBlock.  RN_POTGNN_C2_PAIRS=0 at create time: always.
RunChoices choose(const rn_potgnn *h, bool f32, bool taped) {
  // (the one knob read once per process; the others are handle state, read when the handle was created)
  static const bool centred_on = !(getenv("RN_POTGNN_NODE_CENTRED") && atoi(getenv("RN_POTGNN_NODE_CENTRED")) == 0);
  const GraphPlan &pl = h->plan;
  const auto &pass = h->f32.pass;  // (only float32 runs read the per-pass flag)
  const bool ps_ok = !taped || h->tape_ps;
  RunChoices c;
  c.fused = f32 && pl.use_fused && (!taped || h->tape_fused);
  c.narrow = f32 && pl.use_narrow && !taped;
  c.split_f16 = pl.use_fused && h->mfma_f16;
  c.range_fallback = pl.use_fused && h->mfma_range_fallback;
  c.node_centred = centred_on && c.fused && pl.use_node_fused && h->mfma_f16 && ps_ok;
  c.node_atom = c.node_centred && h->g.na_num > 0;
  c.edge_ps = c.fused && pl.use_ps && ps_ok;
  c.every_pass_role_split = c.folded_gate = !pass.empty();
  for (size_t p = 0; p < pass.size(); ++p) {
    c.every_pass_role_split = c.every_pass_role_split && c.role_split(pass[p].c3_fast);
    c.folded_gate = c.folded_gate && !pl.use_narrow && (pass[p].c3_fast & (pl.use_fused ? 1 : 2)) != 0;
  }
  c.pair_rows = h->want_pair_rows && !h->keep_stages && !taped && c.node_atom && pl.use_readout_fused && c.every_pass_role_split;
  c.c2_pairs = h->want_c2_pairs && c.pair_rows && c2_rows_fit(h);
  return c;
}

// ---- ChunkRun (forward.hpp): one chunk's stages on one lane
template <typename T>
ChunkRun<T>::ChunkRun(rn_potgnn *h_, Lane<T> &l, const ForwardIO<T> &io_, int S_)
    : h(h_), ln(&l), io(io_), S(S_), ch(choose(h_, sizeof(T) == 4, prec<T>(h_).tape_on)) {
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
// With the tape on, the embeddings after pass p are written straight into tape slot p+1 (the
// ping-pong pair is re-pointed pass by pass), so recording costs no copies.
template <typename T>
void ChunkRun<T>::target_tape(int slot, int which) {
  Precision<T> &P = prec<T>(h);
  if (!P.tape_on) return;
  node[which] = P.tape_node[slot].template as<T>();
  edge[which] = P.tape_edge[slot].template as<T>();
}
template <typename T>
void ChunkRun<T>::snapshot(int p) {
  Precision<T> &P = prec<T>(h);
  if (!h->keep_stages && !h->snap_pairs) return;
  HIP_TRY(hipMemcpyAsync(P.snap_node[p].p, node[cur], (size_t)MN * h->d.FnP * sizeof(T),
                         hipMemcpyDeviceToDevice, st()));
  HIP_TRY(hipMemcpyAsync(P.snap_edge[p].p, edge[cur], (size_t)ME * h->d.FeP * sizeof(T),
                         hipMemcpyDeviceToDevice, st()));
}

// geometry + radial basis, initial node embedding
template <typename T>
void ChunkRun<T>::begin() {
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
        if (ch.pair_rows) launch_geom_rbf_pairs_pos32(io.pos32, S, h->g, lat, lat_stride, P.offsets, gauss, h->d, unit4, edge[0], st());
        else launch_geom_rbf_pos32(io.pos32, S, h->g, lat, lat_stride, P.offsets, gauss, h->d, unit4, edge[0], st(), ch.narrow);
        done = true;
      } else if (ch.pair_rows) {
        launch_geom_rbf_pairs(io.pos, S, h->g, lat, lat_stride, P.offsets, gauss, h->d, unit4, edge[0], st());
        done = true;
      }
    }
    if (!done) launch_geom_rbf<T>(io.pos, S, h->g, lat, lat_stride, P.offsets, gauss, h->d, unit4, edge[0], st(), ch.narrow);
    h->last_in_order = ch.narrow;  // (kernels_narrow.hip: edge rows in (b, a) order; rn_potgnn_debug_stage undoes it)
    h->last_pair_rows = ch.pair_rows;
  }
  {
    Timer t(h, st(), K_NODE_INIT);
    launch_node_init<T>(P.node_table, S, h->g, h->d, node[0], io.types, st());
  }
  cur = 0;
  snapshot(0);
}

// begin + every pass: what is left is finish(), or the reverse pass over the tape
template <typename T>
void ChunkRun<T>::run_stages() {
  begin();
  for (int p = 0; p < h->cfg.num_message_passes; ++p) {
    stage_project(p);
    stage_aggregate(p);
  }
}

// Y[R rows] = X W (+ bias): float32 with the split-f16 products enabled -> rowgemm_split_kernel where it serves the shape
// (K a multiple of 64), else the exact-f32 MFMA projection kernel
template <typename T>
void ChunkRun<T>::project(const T *X, int64_t R, int K, const T *WT, int NOUT, T *Y, const T *bias, int amode, const T *nd) {
  if constexpr (sizeof(T) == 4) {
    if (h->mfma_f16 && h->split_projections &&
        launch_rowgemm_split(X, K, K, R, WT, NOUT, Y, false, bias, amode, nd, h->g, st()))
      return;
  }
  launch_rowgemm<T>(X, R, K, WT, NOUT, Y, nullptr, bias, false, amode, nd, h->g, st());
}

// "G" stage of pass p: NodeBlock + every dense projection the EdgeBlock needs
// (matrix pipe / HBM bound)
template <typename T>
void ChunkRun<T>::stage_project(int p) {
  const PassW<T> &w = prec<T>(h).pass[p];
  const Graph &g = h->g;
  const Dims d = h->d;
  const int nxt = cur ^ 1;
  target_tape(p + 1, nxt);
  if constexpr (sizeof(T) == 4) {
    if (ch.narrow) {  // the whole NodeBlock, projections included, in one launch
      Timer t(h, st(), K_NODE_AGG);
      launch_node_narrow(edge[cur], node[cur], node[nxt], S, g, d, w, st());
      return;
    }
  }
  {
    Timer t(h, st(), K_PROJ_NODE);
    if (ch.node_centred) project(node[cur], MN, d.FnP, w.c1_WnT_c, 2 * d.FnP, npc1, w.c1_bias_c, 0, nullptr);  // zero row mean
    else project(node[cur], MN, d.FnP, w.c1_WnT, 2 * d.FnP, npc1, w.c1_bias, 0, nullptr);
  }
  bool node_fused = false;
  if constexpr (sizeof(T) == 4) {
    if (ch.fused && h->plan.use_node_fused) {  // c1 edge projection + aggregation in one launch
      Timer t(h, st(), K_NODE_AGG);
      if (ch.node_atom) launch_node_atom(edge[cur], node[cur], npc1, node[nxt], S, g, d, w, st(), ch.pair_rows);
      else launch_node_fused(edge[cur], node[cur], npc1, node[nxt], S, g, d, w, h->mfma_f16, ch.node_centred, st());
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
    if (ch.role_split(w.c3_fast)) project(node[nxt], MN, d.FnP, w.c3_WnT_c, 6 * d.FeP, np3, w.c3_nshift_c, 0, nullptr);  // zero row mean
    else project(node[nxt], MN, d.FnP, w.c3_WnT, 6 * d.FeP, np3, w.c3_nshift, 0, nullptr);
  }
  if (!ch.fused) {
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
template <typename T>
void ChunkRun<T>::stage_aggregate(int p) {
  const PassW<T> &w = prec<T>(h).pass[p];
  const int nxt = cur ^ 1;
  const float *c2_rows = nullptr;
  if constexpr (sizeof(T) == 4) {
    if (ch.c2_pairs) {  // the c2 branch once per atom pair, into the readout's buffer (idle until finish())
      Timer t(h, st(), K_C2_PAIRS);
      launch_c2_pairs(node[nxt], bufA, S, h->g, h->d, w, st());
      c2_rows = bufA;
    }
  }
  {
    Timer t(h, st(), K_EDGE_AGG);
    if constexpr (sizeof(T) == 4) {
      if (ch.narrow) launch_edge_narrow(edge[cur], edge[nxt], node[nxt], S, h->g, h->d, w, st());
      else if (ch.role_split(w.c3_fast)) launch_edge_ps(edge[cur], edge[nxt], node[nxt], np3, tape_agg(p), S, h->g, h->d, w, h->ps_fail.as<int>(), st(), ch.pair_rows, h->mfma_f16, c2_rows);
      else if (ch.fused) edge_unfused_in_blocks(p);
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
template <typename T>
void ChunkRun<T>::edge_unfused_in_blocks(int p) {
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
template <typename T>
void ChunkRun<T>::finish() {
  Precision<T> &P = prec<T>(h);
  const Graph &g = h->g;
  const Dims d = h->d;
  if (io.desc) {  // the descriptors, from the rows the readout is about to read (nothing has written edge[cur] since the last pass)
    const EdgeRows rows = sizeof(T) == 8 ? EdgeRows::kFloat64 : ch.pair_rows ? EdgeRows::kPairs : EdgeRows::kFloat32;
    if (!edge_pool_supported(rows, d.FeP)) throw HipError{hipErrorInvalidValue, "descriptors: unsupported edge row width"};
    launch_edge_pool(edge[cur], rows, S, g.E, d.Fe, d.FeP, io.desc, st());
    HIP_TRY(hipGetLastError());
  }
  if constexpr (sizeof(T) == 4) {
    if (ch.narrow) {  // readout MLP + edge tensors + per-frame mean in one launch
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
      if (ch.fused && h->plan.use_readout_fused) {  // the three layers in one launch; whole 64-byte rows of the 16 columns it writes
        pol_stride = h->keep_stages ? 32 : 16;  // (the stage snapshots read the unfused chain's 32-column layout)
        launch_readout_fused(edge[cur], ME, P.ro, bufA, h->mfma_f16, st(), ch.pair_rows, pol_stride);
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

template <typename T>
T *ChunkRun<T>::tape_agg(int p) {  // where the EdgeBlock's pre-LayerNorm sums are recorded (taped runs only)
  Precision<T> &P = prec<T>(h);
  return P.tape_on ? P.tape_agg[p].template as<T>() : nullptr;
}

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
  hipEvent_t g_a = h->ev_g[0].get(), g_b = h->ev_g[1].get();
  a.begin();
  b.begin();
  for (int p = 0; p < P; ++p) {
    if (p > 0) HIP_TRY(hipStreamWaitEvent(a.st(), g_b, 0));  // after G_B(p-1)
    a.stage_project(p);
    HIP_TRY(hipEventRecord(g_a, a.st()));
    a.stage_aggregate(p);
    HIP_TRY(hipStreamWaitEvent(b.st(), g_a, 0));             // after G_A(p)
    b.stage_project(p);
    HIP_TRY(hipEventRecord(g_b, b.st()));
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
  hipEvent_t start = h->ev_start.get();
  HIP_TRY(hipEventRecord(start, user));
  for (int l = 0; l < n; ++l) HIP_TRY(hipStreamWaitEvent(lanes[l].stream.get(), start, 0));
}
template <typename T>
void hand_back(rn_potgnn *h, hipStream_t user, Lane<T> *lanes, int n, bool sync, bool timers) {
  for (int l = 0; l < n; ++l) {
    HIP_TRY(hipEventRecord(lanes[l].done.get(), lanes[l].stream.get()));
    HIP_TRY(hipStreamWaitEvent(user, lanes[l].done.get(), 0));
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
  auto make = [&](int lane, int64_t first, int s) { return ChunkRun<T>(h, P.lanes[lane], io.at(first, N, h->d.Fe), s); };
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

template <typename T>
void host_forward(rn_potgnn *h, const double *lattices, const int32_t *types, const double *positions, int64_t S,
                  double *alpha, T *vec6) {
  ForwardIO<T> io;
  io.pos = stage<double>(h->io_pos, positions, (size_t)S * h->cfg.num_atoms * 3 * sizeof(double));
  io.lat = stage_lattices<T>(h, lattices, S);
  io.types = stage_types(h, types, S);
  // float64 6-vectors: the standardised tensor (what PotGNN.forward returns as a 6-vector) is the reduction's value
  // before alpha * sigma + mu
  constexpr bool kernel_vec6 = sizeof(T) == 4;
  if (alpha || !kernel_vec6) {
    h->io_alpha.ensure((size_t)S * 9 * sizeof(double));
    (alpha ? io.alpha : io.alpha_raw) = h->io_alpha.as<double>();
  } else {
    h->io_vec6.ensure((size_t)S * 6 * sizeof(float));
    io.vec6 = h->io_vec6.as<float>();
  }
  forward_device<T>(h, io, S, nullptr, true);
  if (alpha) {
    HIP_TRY(hipMemcpy(alpha, h->io_alpha.p, (size_t)S * 9 * sizeof(double), hipMemcpyDeviceToHost));
  } else if constexpr (kernel_vec6) {
    HIP_TRY(hipMemcpy(vec6, h->io_vec6.p, (size_t)S * 6 * sizeof(float), hipMemcpyDeviceToHost));
  } else {
    std::vector<double> raw((size_t)S * 9);
    HIP_TRY(hipMemcpy(raw.data(), h->io_alpha.p, raw.size() * sizeof(double), hipMemcpyDeviceToHost));
    pick_vec6(raw.data(), S, vec6);
  }
}

// rn_potgnn_descriptors: host_forward's staging with the descriptors [S][Fe] as the result, and the polarizabilities [S][9]
// of the same evaluation when `alpha` is given.
template <typename T>
void host_descriptors(rn_potgnn *h, const double *lattices, const double *positions, int64_t S, double *desc, double *alpha) {
  const size_t desc_bytes = (size_t)S * h->d.Fe * sizeof(double), alpha_bytes = (size_t)S * 9 * sizeof(double);
  ForwardIO<T> io;
  io.pos = stage<double>(h->io_pos, positions, (size_t)S * h->cfg.num_atoms * 3 * sizeof(double));
  io.lat = stage_lattices<T>(h, lattices, S);
  h->io_desc.ensure(desc_bytes);
  io.desc = h->io_desc.as<double>();
  if (alpha) {
    h->io_alpha.ensure(alpha_bytes);
    io.alpha = h->io_alpha.as<double>();
  }
  forward_device<T>(h, io, S, nullptr, true);
  HIP_TRY(hipMemcpy(desc, h->io_desc.p, desc_bytes, hipMemcpyDeviceToHost));
  if (alpha) HIP_TRY(hipMemcpy(alpha, h->io_alpha.p, alpha_bytes, hipMemcpyDeviceToHost));
}

// Chunk size.  Throughput rises monotonically with the frames per launch
// (profiles/r01_chunk_sweep.txt, profiles/r01/overlap_experiments.txt section 7) and the
// Infinity Cache does not reward small chunks.  The fused kernels take a whole CU each, so a
// second lane has nothing to overlap with: ONE lane with an 8 GiB workspace (of 288 GB HBM)
// beats two lanes of 1.5 GiB (63.7 k vs 62.1 k structures/s at 4000 frames).  The unfused
// pipeline keeps two alternating lanes of 1.5 GiB (GraphPlan::num_lanes).
void size_chunk(rn_potgnn *h) {
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
void staged_forward(rn_potgnn *h, const double *positions, const double *lattices, int64_t S, double *d_alpha, bool sync) {
  const size_t per_frame = (size_t)h->cfg.num_atoms * 3;
  const size_t pin_frame = per_frame + (lattices ? 9 : 0);  // floats of a frame in a page-locked piece
  const int64_t chunk = std::max<int64_t>(1, h->chunk);
  hipStream_t exec = h->exec_stream.get(), copy = h->copy_stream.get();
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
    if (hs.copied[b].e) HIP_TRY(hipEventSynchronize(hs.copied[b].e));
  if (hs.done.e) HIP_TRY(hipStreamWaitEvent(copy, hs.done.e, 0));
  for (auto &pin : hs.pin) pin.ensure((size_t)piece * pin_frame * sizeof(float));
  const size_t pos_bytes = (size_t)S * per_frame * sizeof(float);
  if (hs.pos.bytes < pos_bytes && hs.done.e) HIP_TRY(hipEventSynchronize(hs.done.e));  // (growing frees what it may still read)
  hs.pos.ensure(pos_bytes);
  float *d_pos32 = hs.pos.as<float>();
  float *d_lat32 = nullptr;
  if (lattices) {
    const size_t lat_bytes = (size_t)S * 9 * sizeof(float);
    if (hs.lat.bytes < lat_bytes && hs.done.e) HIP_TRY(hipEventSynchronize(hs.done.e));
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
    float *pin = hs.pin[b].as<float>();
    if (k >= 2) HIP_TRY(hipEventSynchronize(hs.copied[b].get()));  // this buffer's previous copy has left it
    const double t1 = now();
    cast_to_float(positions + first * per_frame, pin, (size_t)n * per_frame);
    t_wait += t1 - t0;
    t_cast += now() - t1;
    HIP_TRY(hipMemcpyAsync(d_pos32 + first * per_frame, pin, (size_t)n * per_frame * sizeof(float), hipMemcpyHostToDevice, copy));
    if (lattices) {
      float *pin_lat = pin + (size_t)n * per_frame;
      for (int64_t i = 0; i < n * 9; ++i) pin_lat[i] = (float)lattices[first * 9 + i];
      HIP_TRY(hipMemcpyAsync(d_lat32 + first * 9, pin_lat, (size_t)n * 9 * sizeof(float), hipMemcpyHostToDevice, copy));
    }
    HIP_TRY(hipEventRecord(hs.copied[b].get(), copy));
    HIP_TRY(hipStreamWaitEvent(exec, hs.copied[b].get(), 0));
    ForwardIO<float> io;
    io.pos32 = d_pos32 + first * per_frame;
    io.lat = lattices ? d_lat32 + first * 9 : nullptr;
    io.alpha = d_alpha + first * 9;
    forward_device<float>(h, io, n, exec, sync && first + n >= S);
  }
  HIP_TRY(hipEventRecord(hs.done.get(), exec));  // (everything this call enqueued, on every lane, precedes it)
  if (timing)
    fprintf(stderr, "[host timing] S=%lld pieces=%zu total %.0f us: cast %.0f, buffer waits %.0f, rest (enqueue%s) %.0f\n", (long long)S,
            pieces.size(), now() - t_begin, t_cast, t_wait, sync ? " + final sync" : "", now() - t_begin - t_cast - t_wait);
}

// The float32 host-to-host evaluation behind rn_potgnn_calc_polarizabilities and, with lattices, its _cells form.
void host_polarizabilities(rn_potgnn *h, const double *positions, const double *lattices, int64_t S, double *alpha) {
  const size_t per_frame = (size_t)h->cfg.num_atoms * 3;
  h->io_alpha.ensure((size_t)S * 9 * sizeof(double));
  hipStream_t exec = h->exec_stream.get();
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
      forward_device<float>(h, io, n, exec, first + n >= S);
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
  hs.out.ensure(out_bytes + 16);
  int *fail_pin = reinterpret_cast<int *>(hs.out.as<char>() + out_bytes);
  *fail_pin = 0;
  HIP_TRY(hipMemcpyAsync(hs.out.p, h->io_alpha.p, out_bytes, hipMemcpyDeviceToHost, exec));
  const bool watch = h->plan.use_ps && h->ps_fail.p;
  if (watch) HIP_TRY(hipMemcpyAsync(fail_pin, h->ps_fail.p, sizeof(int), hipMemcpyDeviceToHost, exec));
  HIP_TRY(hipStreamSynchronize(exec));
  resolve_timers(h);
  if (watch && *fail_pin != 0) check_ps_fail(h);  // (reads the word again, clears it and throws)
  std::memcpy(alpha, hs.out.p, out_bytes);
}

// rn_potgnn_debug_stage: what the last float32 evaluation left on lane 0 (evaluate <= one chunk so lane 0 holds it) -- 0 the
// unit vectors, 1 / 2 the node / edge snapshot `index`, 3 the readout's rows, 4 the edge snapshot as it lies in memory.
void read_stage(rn_potgnn *h, int stage, int index, float *out, size_t out_capacity, int64_t *rows, int64_t *cols) {
  const int S = h->last_chunk_structs;
  Precision<float> &P = h->f32;
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
}

#define RN_FORWARD_INSTANCES(T)                                                                              \
  template struct ChunkRun<T>;                                                                               \
  template int chunk_frames<T>(const rn_potgnn *);                                                           \
  template void refresh_pass_flags<T>(rn_potgnn *);                                                          \
  template void device_setup<T>(rn_potgnn *, T *, hipStream_t);                                              \
  template void upload_weights<T>(rn_potgnn *);                                                              \
  template void ensure_precision<T>(rn_potgnn *);                                                            \
  template const T *stage_lattices<T>(rn_potgnn *, const double *, int64_t);                                 \
  template void behind_caller<T>(rn_potgnn *, hipStream_t, Lane<T> *, int);                                  \
  template void hand_back<T>(rn_potgnn *, hipStream_t, Lane<T> *, int, bool, bool);                          \
  template void forward_device<T>(rn_potgnn *, const ForwardIO<T> &, int64_t, hipStream_t, bool);            \
  template void host_forward<T>(rn_potgnn *, const double *, const int32_t *, const double *, int64_t, double *, T *); \
  template void host_descriptors<T>(rn_potgnn *, const double *, const double *, int64_t, double *, double *);
RN_FORWARD_INSTANCES(float)
RN_FORWARD_INSTANCES(double)

}  // namespace rn
