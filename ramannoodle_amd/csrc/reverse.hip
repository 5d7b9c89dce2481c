// The reverse pass over a taped forward and its users: the Jacobian, the input gradients of forward, the atom-group and
// phonon-mode increments.  Training (training.hip) runs the same pass for its parameter gradients.  Host only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "forward.hpp"

namespace rn {

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
  hipStream_t sd = overlap ? P.side.get() : st;
  auto side_after_chain = [&](int which) {  // what the chain has enqueued so far precedes what the side stream gets next
    if (!overlap) return;
    HIP_TRY(hipEventRecord(P.ev_side[which].get(), st));
    HIP_TRY(hipStreamWaitEvent(sd, P.ev_side[which].get(), 0));
  };
  auto chain_after_side = [&]() {  // ... and the other way round
    if (!overlap) return;
    HIP_TRY(hipEventRecord(P.ev_side[2].get(), sd));
    HIP_TRY(hipStreamWaitEvent(st, P.ev_side[2].get(), 0));
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
static size_t tape_elems(const rn_potgnn *h) {  // the tape of one frame (ensure_tape)
  const size_t N = h->cfg.num_atoms, E = h->cfg.num_edges, NP = h->cfg.num_message_passes;
  return (NP + 1) * (N * h->d.FnP + 2 * E * h->d.FeP);
}
static size_t reverse_elems(const rn_potgnn *h) {  // the reverse pass's workspace for one cotangent row of one frame (reverse_pass: sizes)
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
  hipStream_t st = P.lanes[0].stream.get();
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
    HIP_TRY(hipStreamSynchronize(P.lanes[0].stream.get()));  // (an earlier chunk may still read the old seeds)
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
  hipStream_t st = P.lanes[0].stream.get();
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
                      hipStream_t user, const double *d_lat) {
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
  const ModeVectors modes = upload_modes(h->mode_vectors, disp, proj, M, N, limit, prec<T>(h).lanes[0].stream.get());
  const double *sigma = h->d_mean_std.as<double>() + 9;
  const int channels = M + (rest ? 1 : 0);
  const int out_channels = channels + (d_lat ? 1 : 0);
  chunked_increments<T>(h, d_pos, S, limit - modes.bytes, out_channels, channels, d_out, user, d_lat,
                        "mode_increments: one step does not fit the workspace limit",
                        [&](const double *jac, const double *pos, int f, double *out, hipStream_t st2) {
                          mode_contract(jac, (int64_t)f + 1, pos, N, modes.disp, modes.proj, M, sigma, rest, out_channels, out, st2);
                        });
}

// Raman tensors per atom group [M][G][9] from the float64 Jacobian rows at the reference structure (the group table is set).
void partial_raman(rn_potgnn *h, const double *ref_positions, const double *displacements, int64_t M, int G, double *raman) {
  ensure_precision<double>(h);
  h->train_S = 0;  // the tape and lane 0 are reused: a pending train_forward is void
  const int N = h->g.N;
  const size_t n3 = (size_t)N * 3;
  hipStream_t st = h->f64.lanes[0].stream.get();
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
}

#define RN_REVERSE_INSTANCES(T)                                                                                       \
  template void reverse_pass<T>(rn_potgnn *, ChunkRun<T> &, const Reverse<T> &);                                      \
  template ChunkRun<T> taped_forward<T>(rn_potgnn *, const ForwardIO<T> &, int);                                      \
  template void jacobian<T>(rn_potgnn *, const double *, double *);                                                   \
  template void forward_vjp<T>(rn_potgnn *, const double *, const int32_t *, const double *, int64_t, const double *, \
                               double *, double *, hipStream_t);                                                      \
  template void group_increments<T>(rn_potgnn *, const double *, int64_t, int, size_t, double *, hipStream_t,         \
                                    const double *);                                                                  \
  template void mode_increments<T>(rn_potgnn *, const double *, int64_t, const double *, const double *, int, bool,   \
                                   size_t, double *, hipStream_t, const double *);
RN_REVERSE_INSTANCES(float)
RN_REVERSE_INSTANCES(double)

}  // namespace rn
