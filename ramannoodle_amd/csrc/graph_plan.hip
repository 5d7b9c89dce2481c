// Host-only graph planner (graph_plan.hpp).  A .hip file only because the *_lds_bytes / *_supported host functions it
// calls are declared in kernels.hpp next to their kernels; it holds no kernel and calls nothing of the HIP runtime.
#include "graph_plan.hpp"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

namespace rn {

namespace {

std::string format(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return buf;
}

const char *knob(const char *name) { return getenv(name); }
bool knob_flag(const char *name, bool otherwise) { return knob(name) ? atoi(knob(name)) != 0 : otherwise; }

// Fe padded to 64 with a narrower Fn (e.g. Fn = 32 / Fe = 64, Fn = 20 / Fe = 48): padding
// Fn to 64 as well puts the model on the fused MFMA kernels (their masked LayerNorms handle F < FP) instead of the unfused
// per-stage chain (round 3: 15.4 -> 12.4 us per 128-atom structure).  Since round 5 the same holds for Fe in 17..32 (below).
// RN_POTGNN_WIDEN=0: minimal power-of-two padding everywhere; =1: round 4's policy; =3: experiment.
void widen_for_fused(Dims &d, int widen) {
  if (widen == 0) return;
  if (d.FeP == 64 && d.FnP < 64) d.FnP = 64;
  // round 5: with the role-specialised EdgeBlock at 3.2 us per structure and pass the 64-wide fused kernels (7.8 us per
  // 128-atom structure whatever the real widths) are level with or ahead of the unfused chain for every Fe in 17..32 (7.5-7.9 us
  // at Fn <= 32, 9.1 at Fn in 33..64: profiles/r05/width_sweep.txt), so those pad to 64 x 64 as well: one kernel family
  // for every edge width in 17..64.  Fe <= 16 with a wide Fn stays unfused (6.0 us).  RN_POTGNN_WIDEN=1 keeps round 4's
  // policy (only Fe in 33..64 widens Fn).
  if (widen >= 2 && d.FeP == 32 && d.FnP >= 32 && d.FnP <= 64) d.FnP = d.FeP = 64;  // Fe in 17..32, Fn in 17..64 (Fn <= 16: 6.8 unfused against 7.7)
  if (widen >= 3 && d.FeP <= 16 && d.FnP >= 32 && d.FnP <= 64) d.FnP = d.FeP = 64;  // (experiment) Fe <= 16 with Fn in 17..64
}

// The three maxima of a partition, from the CSRs.
void fill_maxima(Partition &p, const GraphPlan &g) {
  p.max_out_rows = p.max_in_rows = p.max_nodes = 0;
  for (size_t t = 0; t + 1 < p.begin.size(); ++t) {
    p.max_out_rows = std::max(p.max_out_rows, g.out_ptr[p.begin[t + 1]] - g.out_ptr[p.begin[t]]);
    p.max_in_rows = std::max(p.max_in_rows, g.in_ptr[p.begin[t + 1]] - g.in_ptr[p.begin[t]]);
    p.max_nodes = std::max(p.max_nodes, p.begin[t + 1] - p.begin[t]);
  }
}

// What a greedy walk counts against its budget.  The out-row walk calls a tile open once it holds a row, the in-row
// walk once it holds an atom: an atom without edges in front of one over the budget stays with it in the first and
// gets a tile of its own in the second.
enum class Rows { Out, In };

// Consecutive atoms, a tile closed when the next atom would exceed `budget` rows (or, with `cap`, that many atoms).
// (a single atom with more rows than the budget still gets its tile: the LDS checks of the callers decide)
Partition greedy_tiles(const GraphPlan &g, Rows what, size_t budget, int cap = 0) {
  const std::vector<int> &ptr = what == Rows::Out ? g.out_ptr : g.in_ptr;
  Partition p;
  p.begin.assign(1, 0);
  int rows = 0, first = 0;
  for (int n = 0; n < g.N; ++n) {
    const int deg = ptr[n + 1] - ptr[n];
    const bool open = what == Rows::Out ? rows > 0 : n > first;
    if (open && ((size_t)(rows + deg) > budget || (cap > 0 && n - first >= cap))) {
      p.begin.push_back(n);
      first = n;
      rows = 0;
    }
    rows += deg;
  }
  p.begin.push_back(g.N);
  fill_maxima(p, g);
  return p;
}

// what edge_agg_kernel asks of LDS on a partition, in float64 (the float64 chain has no other EdgeBlock)
size_t edge_agg_f64_lds_bytes(Dims d, int max_out_rows, int max_in_rows, int max_nodes) {
  Graph s{};
  s.max_tile_out_rows = max_out_rows, s.max_tile_in_rows = max_in_rows, s.max_tile_nodes = max_nodes;
  return edge_agg_lds_bytes(s, d, sizeof(double));
}

// every atom a tile of its own: the partition with the smallest footprint there is (validate_create_args admits a graph
// when this one fits the CU in float64)
Partition one_atom_tiles(const GraphPlan &g) {
  Partition p;
  p.begin.resize(g.N + 1);
  for (int n = 0; n <= g.N; ++n) p.begin[n] = n;
  fill_maxima(p, g);
  return p;
}

// node tiles: consecutive atoms whose outgoing-edge rows fit an LDS budget (counted in
// float32 rows; the float64 path uses twice the bytes for the same tiles).  A workgroup
// serves its tile's destination edges G at a time (G lane groups), so the budget is chosen
// to waste as few lane groups in the last round as possible (18 in-edges per atom and
// G = 16: 4 atoms per tile idle 10 % of the groups, 6 atoms 4 %).
Partition edge_tiles(const GraphPlan &g, const PlanKnobs &k, bool fused_mode, bool narrow_mode) {
  const Dims d = g.d;
  const int N = g.N, E = g.E;
  const size_t row_bytes = (size_t)2 * d.FeP * sizeof(float);  // (the out-degree cap was checked by validate_create_args)
  if (narrow_mode && !k.tile_kb_set) {
    // narrow-width kernels (kernels_narrow.hip): one lane per destination edge, so a tile should bring
    // about one workgroup's worth (256) of destination edges and keep its LDS rows within ~40 KiB
    const size_t per_row = edge_narrow_lds_bytes(d.Fn, d.Fe, 1024, 1024) / 1024 + 1;
    // 128 rows = one two-wave workgroup per tile (kernels_narrow.hip launch_edge_cfg); an atom with more out-edges gets a
    // tile of its own and the four-wave form
    size_t budget = std::min<size_t>(128, (size_t)40 * 1024 / per_row);
    if (k.narrow_tile_rows > 0) budget = (size_t)k.narrow_tile_rows;
    Partition greedy = greedy_tiles(g, Rows::Out, std::max<size_t>(1, budget));
    // The greedy partition fills every tile but the last (256 atoms of degree 18: eighteen tiles of 14 atoms and one
    // of 4).  The same NUMBER of tiles with boundaries at equal shares of the edge list (14, 13, 14, 13, ...) costs
    // the same lane slots and keeps the workgroups of a frame in step, as long as no tile exceeds the budget.
    if (greedy.num() > 1) {
      const int T = greedy.num();
      Partition even;
      even.begin.assign(1, 0);
      for (int t = 1; t < T; ++t) {
        const int64_t want = ((int64_t)E * t + T - 1) / T;
        int n = even.begin.back();
        while (n < N && g.out_ptr[n] < want) ++n;
        even.begin.push_back(std::max(n, even.begin.back()));
      }
      even.begin.push_back(N);
      bool ok = true;
      for (int t = 0; t < T; ++t) ok = ok && even.begin[t + 1] > even.begin[t];
      fill_maxima(even, g);
      if (ok && (size_t)even.max_out_rows <= budget && even.max_in_rows <= std::max(greedy.max_in_rows, (int)budget)) return even;
    }
    return greedy;
  }
  if (k.tile_kb_set || k.vpl8) return greedy_tiles(g, Rows::Out, std::max<size_t>(1, (size_t)k.tile_kb * 1024 / row_bytes));
  // relative cost of one frame = (rounds of the slowest tile) x (tiles sharing the chip),
  // among budgets whose whole LDS footprint stays within 64 KiB (measured: beyond that
  // only one workgroup per CU runs)
  const int G = 256 / std::max(1, d.FeP / 4);
  double best = 0;
  Partition chosen;
  for (size_t kb = 8; kb <= 62; kb += 2) {
    const Partition p = greedy_tiles(g, Rows::Out, std::max<size_t>(1, kb * 1024 / row_bytes));
    const int mr = p.max_out_rows, max_in = p.max_in_rows, max_nodes = p.max_nodes;
    const int rounds = std::max(1, (max_in + G - 1) / G);
    // (fused: the footprint of the retired per-frame kernel still sizes these tiles -- kernels_fused.hip says why)
    const size_t lds = fused_mode ? edge_fused_lds_bytes(mr, max_in, max_nodes)
                                  : (size_t)mr * (row_bytes + 4) + (size_t)max_nodes * row_bytes +
                                        (size_t)12 * d.FeP * 4 + (size_t)mr * 4 + (size_t)max_in * 24 + 96;
    // unfused: two aggregation workgroups + one projection workgroup (34 KiB) share a CU
    const size_t lds_cap = fused_mode ? kFusedLdsBudget : (size_t)63 * 1024;
    if (lds > lds_cap && !chosen.begin.empty()) break;
    const double cost = (double)rounds * (double)p.num();
    if (chosen.begin.empty() || cost < best * 0.995) {
      best = cost;
      chosen = p;
    }
  }
  return chosen;
}

// node tiles of the EdgeBlock reverse kernel: the largest whose float32 LDS footprint leaves room for two workgroups
// per CU (RN_POTGNN_BWD_TILES=0: the forward kernel's tiles, one 512-thread workgroup per CU)
Partition reverse_tiles(const GraphPlan &g) {
  Partition chosen;
  for (size_t budget = 1; budget <= 512; ++budget) {
    const Partition p = greedy_tiles(g, Rows::Out, budget);
    if (edge_bwd_tile2_lds_bytes(p.max_out_rows, p.max_in_rows, p.max_nodes, g.d.FeP, sizeof(float)) > (size_t)78 * 1024) {
      if (!chosen.begin.empty()) break;
      continue;
    }
    if (chosen.begin.empty() || p.max_out_rows > chosen.max_out_rows) chosen = p;
  }
  return chosen;
}

// node_tiled_kernel (kernels_narrow.hip): ONE WAVE per tile -- at most 64 atoms (one lane each in its last pass)
// whose in-edge rows are streamed 64 at a time: the partition that fills those chunks best, within 12 KiB of LDS
// (thirteen waves per CU and more); among equals the larger tiles (fewer frame starts per row)
Partition node_tiles_narrow(const GraphPlan &g, const PlanKnobs &k) {
  double best = -1;
  Partition chosen;
  const int max_budget = k.node_tile_rows_set ? std::max(1, k.node_tile_rows) : 256;
  for (int budget = 32; budget <= std::max(max_budget, 32); budget += 2) {
    const Partition p = greedy_tiles(g, Rows::In, (size_t)budget, 64);
    double work = 0;  // chunk slots the partition pays for
    for (int t = 0; t < p.num(); ++t)
      work += (double)std::max((g.in_ptr[p.begin[t + 1]] - g.in_ptr[p.begin[t]] + 63) / 64, 1) * 64.0;
    if (node_tiled_lds_bytes(g.d.Fn, g.d.Fe, p.max_in_rows, p.max_nodes) > (size_t)(chosen.begin.empty() ? 64 : k.node_tile_kb) * 1024) {
      if (!chosen.begin.empty()) break;
      continue;
    }
    const double fill = (double)g.E / std::max(work, 1.0);
    if (fill >= best * 0.999) {
      best = std::max(best, fill);
      chosen = p;
    }
  }
  return chosen;
}

// node tiles of the fused NodeBlock kernel: consecutive atoms by IN-edges; four workgroups per CU
// (40 KiB of LDS each), as few rounds x tiles as possible
Partition node_tiles_wide(const GraphPlan &g, const PlanKnobs &k) {
  double best = 0;
  Partition chosen;
  const int forced = k.node_tile_rows_set ? k.node_tile_rows : 0;  // experiment knob
  for (int budget = forced > 0 ? forced : 16; budget <= (forced > 0 ? forced : 256); budget += 8) {
    const Partition p = greedy_tiles(g, Rows::In, (size_t)budget);
    if (node_fused_lds_bytes(p.max_in_rows, p.max_nodes) > (size_t)40 * 1024 && !chosen.begin.empty()) break;
    const double cost = (double)((p.max_in_rows + 15) / 16) * (double)p.num();
    if (chosen.begin.empty() || cost < best * 0.995) {
      best = cost;
      chosen = p;
    }
  }
  return chosen;
}

// node tiles of the role-specialised EdgeBlock (kernels_edge_ps.hip): ONE twelve-wave workgroup per CU, 16 destinations
// per round.  A launch runs floor(CUs / tiles) frame groups side by side, so the cost of a partition is (rounds of its
// slowest tile) / (frame groups); a partition is admissible when every tile passes the producers' schedule check and
// the kernel's LDS footprint fits the CU.
Partition ps_tiles(const GraphPlan &g, const PlanKnobs &k, int cus, int *pt_back, int *pt_gram) {
  double best = 0;
  Partition chosen;
  std::vector<int> rb, re;
  const int forced = k.ps_tile_rows;  // experiment knob
  const bool want_back3 = k.ps_back != 2;
  // GRAM is opt-in (RN_POTGNN_PS_GRAM=1): parity-green, but the producers' Gram phase costs them more than the consumers' loop
  // gains while the producers are the slower role with it (profiles/r05/edge_ps_experiments.txt: 7.38 against 7.01 ms per launch)
  // One variant of the kernel for a partition: {gram, back}.  GRAM (the LayerNorm cross terms on the matrix pipe) has a ring
  // of 7 tiles and needs every round's window to span <= 3 of them, every destination <= 32 source rows, and its tables
  // inside the CU's LDS; back = 3 (the producers three rounds ahead of the slower consumer set) needs the room in the ring.
  // (back = 4: with eight destinations per consumer wave four rounds are in flight at a time -- the eight-lane form of
  //  the kernel --, and a step that may only rewrite the ring behind round g - 4 would stall the producers)
  struct Variant { bool gram; int back; double factor; };
  const Variant variants[6] = {{true, 3, 0.88}, {true, 2, 0.94}, {false, 5, 0.94}, {false, 4, 0.96}, {false, 3, 1.0}, {false, 2, 1.07}};
  for (size_t budget = forced > 0 ? forced : 8; budget <= (size_t)(forced > 0 ? forced : 1024); budget += 2) {
    const Partition p = greedy_tiles(g, Rows::Out, budget);
    const int ntiles = p.num();
    for (const Variant &v : variants) {
      if ((v.gram && !k.want_gram) || (v.back == 3 && !want_back3) || v.back > k.ps_back) continue;
      bool ok = true;
      for (int t = 0; t < ntiles && ok; ++t) {
        const int eo0 = g.out_ptr[p.begin[t]];
        rb.clear();
        re.clear();
        int longest = 0;
        for (int i = g.in_ptr[p.begin[t]]; i < g.in_ptr[p.begin[t + 1]]; ++i) {
          const int bd = g.edge_b[g.in_edge[i]];
          rb.push_back(g.out_ptr[bd] - eo0);
          re.push_back(g.out_ptr[bd + 1] - eo0);
          longest = std::max(longest, re.back() - rb.back());
        }
        int window = 0;
        ok = edge_ps_tile_ok(rb.data(), re.data(), (int)rb.size(), v.back, edge_ps_ring_tiles(v.gram), &window);
        if (v.gram) ok = ok && window <= edge_ps_gram_window() && longest <= 32;
      }
      if (!ok || edge_ps_lds_bytes(p.max_out_rows, p.max_in_rows, v.gram) > (size_t)160 * 1024) continue;
      const int max_rounds = std::max(1, (p.max_in_rows + 15) / 16);
      const double groups = ntiles <= cus ? (double)(cus / ntiles) : 1.0 / (double)((ntiles + cus - 1) / cus);
      const double cost = (double)max_rounds / groups * v.factor;
      if (chosen.begin.empty() || cost < best * 0.999) {
        best = cost;
        chosen = p;
        *pt_back = v.back;
        *pt_gram = v.gram ? 1 : 0;
      }
      break;  // (the variants are ordered by their factor: the first admissible one is this partition's)
    }
    if (p.max_out_rows >= g.E) break;  // one tile holds everything: larger budgets change nothing
  }
  return chosen;
}

// the atom-owning NodeBlock pays max-in-degree rounds per 16-atom tile; the row-ordered one ceil(rows / 16) per tile of
// its own partition.  A round of the former is ~25 % cheaper (one barrier, no LDS pass per row): take it unless the
// in-degrees are so uneven that it runs > 1.2x the rounds.  RN_POTGNN_NODE_ATOM=0 / 1 forces.
void choose_node_atom(GraphPlan &g, const PlanKnobs &k) {
  const int N = g.N;
  int max_deg = 0;
  long rounds_atom = 0, rounds_row = 0;
  for (int n0 = 0; n0 < N; n0 += 16) {
    int m = 0;
    for (int n = n0; n < std::min(N, n0 + 16); ++n) m = std::max(m, g.in_ptr[n + 1] - g.in_ptr[n]);
    rounds_atom += m;
    max_deg = std::max(max_deg, m);
  }
  for (int t = 0; t < g.nt.num(); ++t) rounds_row += (g.in_ptr[g.nt.begin[t + 1]] - g.in_ptr[g.nt.begin[t]] + 15) / 16;
  bool ok = !g.nt_narrow && g.d.FnP == 64 && g.d.FeP == 64 && node_atom_lds_bytes(max_deg) <= (size_t)40 * 1024 &&
            (double)rounds_atom <= 1.2 * (double)rounds_row;
  if (k.node_atom >= 0) ok = k.node_atom != 0 && g.d.FnP == 64 && g.d.FeP == 64 && node_atom_lds_bytes(max_deg) <= (size_t)64 * 1024;
  g.na_num = ok ? (N + 15) / 16 : 0;
  g.na_max_deg = max_deg;
}

// CSR over a (edges are already grouped), CSR over b, triplet offsets, reverse edges
void build_index_arrays(GraphPlan &g) {
  const int N = g.N, E = g.E;
  const int *edge_a = g.edge_a.data(), *edge_b = g.edge_b.data();
  g.out_ptr.assign(N + 1, 0);
  g.in_ptr.assign(N + 1, 0);
  for (int e = 0; e < E; ++e) {
    g.out_ptr[edge_a[e] + 1]++;
    g.in_ptr[edge_b[e] + 1]++;
  }
  for (int n = 0; n < N; ++n) {
    g.out_ptr[n + 1] += g.out_ptr[n];
    g.in_ptr[n + 1] += g.in_ptr[n];
  }
  g.in_edge.assign(E, 0);
  {
    std::vector<int> fill(g.in_ptr.begin(), g.in_ptr.end() - 1);
    for (int e = 0; e < E; ++e) g.in_edge[fill[edge_b[e]]++] = e;  // ascending edge id per b
  }
  g.in_pos.assign(E, 0);
  for (int i = 0; i < E; ++i) g.in_pos[g.in_edge[i]] = i;  // position of edge e in the (b, a) order
  g.trip_off.assign(E + 1, 0);
  g.rev_edge.assign(E, -1);
  for (int e = 0; e < E; ++e) {
    const int bd = edge_b[e], ad = edge_a[e];
    int cnt = 0;
    for (int o = g.out_ptr[bd]; o < g.out_ptr[bd + 1]; ++o) cnt += edge_b[o] != ad;
    g.trip_off[e + 1] = g.trip_off[e] + cnt;
    // reverse edge (b -> a): binary search in b's sorted out-list
    const int *lo = edge_b + g.out_ptr[bd], *hi = edge_b + g.out_ptr[bd + 1];
    const int *it = std::lower_bound(lo, hi, ad);
    if (it != hi && *it == ad) g.rev_edge[e] = (int)(it - edge_b);
  }
  g.T = g.trip_off[E];
  // atom pairs: the reverse of an edge with a lower id has its pair already
  g.pair_of_edge.assign(E, -1);
  g.pair_a.clear();
  g.pair_b.clear();
  for (int e = 0; e < E; ++e) {
    const int r = g.rev_edge[e];
    if (r >= 0 && r < e) {
      g.pair_of_edge[e] = g.pair_of_edge[r];
    } else {
      g.pair_of_edge[e] = (int)g.pair_a.size();
      g.pair_a.push_back(edge_a[e]);
      g.pair_b.push_back(edge_b[e]);
    }
  }
}

}  // namespace

PlanKnobs read_plan_knobs() {
  PlanKnobs k;
  static const int widen = knob("RN_POTGNN_WIDEN") ? atoi(knob("RN_POTGNN_WIDEN")) : 2;
  k.widen = widen;
  k.vpl8 = knob("RN_POTGNN_VPL") && atoi(knob("RN_POTGNN_VPL")) == 8;
  k.want_fused = knob_flag("RN_POTGNN_FUSED", true);
  k.want_narrow = knob_flag("RN_POTGNN_NARROW", true);
  if (const char *e = knob("RN_POTGNN_TILE_KB")) k.tile_kb_set = true, k.tile_kb = atoi(e);
  if (const char *e = knob("RN_POTGNN_NARROW_TILE_ROWS")) k.narrow_tile_rows = std::max(1, atoi(e));
  k.bwd_tiles = knob_flag("RN_POTGNN_BWD_TILES", true);
  if (const char *e = knob("RN_POTGNN_NODE_TILE_ROWS")) k.node_tile_rows_set = true, k.node_tile_rows = atoi(e);
  if (const char *e = knob("RN_POTGNN_NODE_TILE_KB")) k.node_tile_kb = std::max(1, atoi(e));
  k.want_ps = knob_flag("RN_POTGNN_EDGE_PS", true);
  if (const char *e = knob("RN_POTGNN_PS_TILE_ROWS")) k.ps_tile_rows = atoi(e);
  if (const char *e = knob("RN_POTGNN_PS_BACK")) k.ps_back = atoi(e);
  k.want_gram = knob_flag("RN_POTGNN_PS_GRAM", false);
  if (const char *e = knob("RN_POTGNN_NODE_ATOM")) k.node_atom = atoi(e) != 0;
  k.want_node_fused = knob_flag("RN_POTGNN_NODE_FUSED", true);
  k.want_readout_fused = knob_flag("RN_POTGNN_READOUT_FUSED", true);
  if (const char *e = knob("RN_POTGNN_LANES")) k.lanes = std::max(1, std::min(2, atoi(e)));
  return k;
}

int pad_pow2(int f) {
  int p = 16;
  while (p < f) p *= 2;
  return p;
}

Dims plan_dims(const rn_potgnn_config &cfg, const PlanKnobs &knobs) {
  Dims d = {cfg.size_node_embedding, cfg.size_edge_embedding, pad_pow2(cfg.size_node_embedding),
            pad_pow2(cfg.size_edge_embedding)};
  widen_for_fused(d, knobs.widen);
  return d;
}

// The float64 EdgeBlock (edge_agg_kernel) keeps a tile's source rows, their scalars, the tile's node rows, the pass's
// LayerNorm weights and two index tables in LDS.  The smallest tile there is holds one atom: the cap is the largest degree
// D at which such a tile, with D out-edges and D in-edges (a radius graph has b -> a beside a -> b), still fits the CU --
// 554 / 292 / 147 / 71 at FeP = 16 / 32 / 64 / 128.
size_t max_out_degree(Dims d) {
  size_t deg = 0;
  while (edge_agg_f64_lds_bytes(d, (int)deg + 1, (int)deg + 1, 1) <= kCuLdsBytes) ++deg;
  return deg;
}

int validate_config(const rn_potgnn_config *cfg_in, bool others_null, const size_t *num_weights, std::string &error) {
  if (!cfg_in || others_null) {
    error = "null argument";
    return RN_ERR_INVALID_ARGUMENT;
  }
  const rn_potgnn_config &cfg = *cfg_in;
  const int N = cfg.num_atoms, E = cfg.num_edges;
  if (N <= 0 || E < 0 || cfg.num_atom_types <= 0 || cfg.size_node_embedding <= 0 ||
      cfg.size_edge_embedding <= 0 || cfg.num_message_passes <= 0) {
    error = "invalid configuration (non-positive size)";
    return RN_ERR_INVALID_ARGUMENT;
  }
  if (E == 0) {
    error = "reference graph has no edges: the per-structure mean over edges "
            "(_gnn.py:662-664) is undefined";
    return RN_ERR_INVALID_ARGUMENT;
  }
  if (cfg.size_node_embedding > 128 || cfg.size_edge_embedding > 128) {
    error = format("embedding sizes above 128 are not supported (Fn=%d, Fe=%d)", cfg.size_node_embedding,
                   cfg.size_edge_embedding);
    return RN_ERR_UNSUPPORTED;
  }
  if (num_weights && *num_weights != rn_potgnn_weight_count(&cfg)) {
    error = format("weights has %zu floats, expected %zu", *num_weights, rn_potgnn_weight_count(&cfg));
    return RN_ERR_INVALID_ARGUMENT;
  }
  return RN_OK;
}

int validate_create_args(const rn_potgnn_config *cfg_in, const int32_t *edge_a, const int32_t *edge_b, const int32_t *atom_types,
                         bool others_null, const size_t *num_weights, std::string &error) {
  const bool graph_null = !atom_types || (cfg_in && cfg_in->num_edges > 0 && (!edge_a || !edge_b));
  if (const int rc = validate_config(cfg_in, others_null || graph_null, num_weights, error); rc != RN_OK) return rc;
  const rn_potgnn_config &cfg = *cfg_in;
  const int N = cfg.num_atoms, E = cfg.num_edges;
  for (int e = 0; e < E; ++e) {
    if (edge_a[e] < 0 || edge_a[e] >= N || edge_b[e] < 0 || edge_b[e] >= N || edge_a[e] == edge_b[e]) {
      error = format("edge %d = (%d,%d) is out of range or a self loop", e, edge_a[e], edge_b[e]);
      return RN_ERR_INVALID_ARGUMENT;
    }
    if (e > 0 && (edge_a[e] < edge_a[e - 1] || (edge_a[e] == edge_a[e - 1] && edge_b[e] <= edge_b[e - 1]))) {
      error = format("edges must be strictly sorted by (a, b); violated at edge %d", e);
      return RN_ERR_INVALID_ARGUMENT;
    }
  }
  for (int n = 0; n < N; ++n)
    if (atom_types[n] < 0 || atom_types[n] >= cfg.num_atom_types) {
      error = format("atom %d has type %d outside [0,%d)", n, atom_types[n], cfg.num_atom_types);
      return RN_ERR_INVALID_ARGUMENT;
    }
  // a one-atom tile of the float64 EdgeBlock must fit the CU's LDS at the widths the model is PLANNED at (24 / 20 runs
  // 64 wide); plan_graph falls back to one-atom tiles where its own choice does not fit, so accepted => every request fits
  const Dims d = plan_dims(cfg, read_plan_knobs());
  const size_t cap = max_out_degree(d);
  std::vector<int> deg(N, 0), deg_in(N, 0);
  for (int e = 0; e < E; ++e) deg[edge_a[e]]++, deg_in[edge_b[e]]++;
  for (int n = 0; n < N; ++n)
    if ((size_t)deg[n] > cap) {
      error = format("atom %d has %d outgoing edges; more than %zu per atom is unsupported "
                     "for size_edge_embedding=%d", n, deg[n], cap, cfg.size_edge_embedding);
      return RN_ERR_UNSUPPORTED;
    }
  // (a directed graph whose in-degrees exceed its out-degrees: the tables of the destination edges count as well)
  const int max_out = *std::max_element(deg.begin(), deg.end()), max_in = *std::max_element(deg_in.begin(), deg_in.end());
  const size_t need = edge_agg_f64_lds_bytes(d, max_out, max_in, 1);
  if (need > kCuLdsBytes) {
    error = format("an atom with %d outgoing edges beside one with %d incoming edges needs %zu bytes of LDS per tile in "
                   "float64 (%zu available) for size_edge_embedding=%d", max_out, max_in, need, kCuLdsBytes, cfg.size_edge_embedding);
    return RN_ERR_UNSUPPORTED;
  }
  return RN_OK;
}

GraphPlan plan_graph(const rn_potgnn_config &cfg, Dims d, const int32_t *edge_a, const int32_t *edge_b,
                     const int32_t *atom_types, int num_cus, const PlanKnobs &k) {
  GraphPlan g;
  g.N = cfg.num_atoms;
  g.E = cfg.num_edges;
  g.d = d;
  g.edge_a.assign(edge_a, edge_a + g.E);
  g.edge_b.assign(edge_b, edge_b + g.E);
  g.atom_type.assign(atom_types, atom_types + g.N);
  build_index_arrays(g);

  // fused EdgeBlock (kernels_fused.hip): its LDS footprint bounds the tile instead
  const bool fused_mode = k.want_fused && d.FnP == 64 && d.FeP == 64;
  const bool narrow_mode = k.want_narrow && narrow_supported(d);
  g.tile = edge_tiles(g, k, fused_mode, narrow_mode);
  // The searches above size tiles in float32 and always keep their first candidate; the maxima of a partition also mix
  // tiles (the rows of a hub's tile with the atoms of a tile of low-degree atoms).  Where the float64 EdgeBlock could not
  // hold the result, every atom gets its own tile: that fits whenever validate_create_args accepted the graph.  The
  // float32 kernels share Graph::tile_begin, so they run on the one-atom tiles too (slower for such a graph, never wrong:
  // every kernel that reads this partition -- edge_agg, the narrow EdgeBlock, the reverse kernels without bt_ -- takes any
  // partition of consecutive atoms and sizes its LDS from the maxima; use_fused / use_narrow below are decided on it).
  if (edge_agg_f64_lds_bytes(d, g.tile.max_out_rows, g.tile.max_in_rows, g.tile.max_nodes) > kCuLdsBytes) g.tile = one_atom_tiles(g);
  if (k.bwd_tiles) g.bt = reverse_tiles(g);
  if (narrow_mode) g.nt = node_tiles_narrow(g, k);
  g.nt_narrow = g.nt.num() > 0;
  if (!g.nt_narrow) g.nt = node_tiles_wide(g, k);
  if (fused_mode && k.want_ps) g.pt = ps_tiles(g, k, num_cus, &g.pt_back, &g.pt_gram);
  choose_node_atom(g, k);

  // The fused kernels (kernels_fused.hip) are the default where they apply (float32, Fn and
  // Fe padded to 64); RN_POTGNN_FUSED=0 selects projections + edge_agg_kernel.
  const Graph s = g.scalars();
  g.use_fused = k.want_fused && edge_fused_supported(s, d);
  g.use_ps = g.use_fused && g.pt.num() > 0;
  g.use_narrow = narrow_mode && edge_narrow_lds_bytes(d.Fn, d.Fe, g.tile.max_out_rows, g.tile.max_in_rows) <= (size_t)64 * 1024;
  g.use_node_fused = g.use_fused && k.want_node_fused && node_fused_lds_bytes(s) <= 64 * 1024;
  g.use_readout_fused = g.use_fused && k.want_readout_fused;
  // Lanes.  The fused kernels take a whole CU each, so a second lane has nothing to overlap with; the unfused
  // pipeline keeps two alternating lanes.  Round 4: the role-specialised EdgeBlock is bound by SIMD issue and
  // leaves HBM idle and ~10 KiB of LDS per CU free, so the small HBM-bound kernels of a second lane (geometry, per-atom
  // projections, readout reduction) do run under it: RN_POTGNN_LANES=2 gives 48.9 -> 49.2 k structures/s on config 3.
  // Not the default: kernels of two lanes wait for each other's LDS, and HIP events around a launch then time the wait
  // too (the NodeBlock's HBM figure of the bench line reads 6 % instead of 46 %).
  g.num_lanes = k.lanes > 0 ? k.lanes : ((g.use_fused || g.use_narrow) ? 1 : 2);
  return g;
}

Graph GraphPlan::scalars() const {
  Graph s{};
  s.N = N, s.E = E, s.T = T;
  s.NP = (int)pair_a.size();
  s.num_tiles = tile.num(), s.max_tile_out_rows = tile.max_out_rows, s.max_tile_in_rows = tile.max_in_rows, s.max_tile_nodes = tile.max_nodes;
  s.nt_num = nt.num(), s.nt_max_in_rows = nt.max_in_rows, s.nt_max_nodes = nt.max_nodes, s.nt_narrow = nt_narrow ? 1 : 0;
  s.na_num = na_num, s.na_max_deg = na_max_deg;
  s.pt_num = pt.num(), s.pt_max_out_rows = pt.max_out_rows, s.pt_max_in_rows = pt.max_in_rows, s.pt_back = pt_back, s.pt_gram = pt_gram;
  s.bt_num = bt.num(), s.bt_max_out_rows = bt.max_out_rows, s.bt_max_in_rows = bt.max_in_rows, s.bt_max_nodes = bt.max_nodes;
  return s;
}

std::vector<int64_t> GraphPlan::lds_requests() const {
  const Graph s = scalars();
  const bool node_fused = use_fused && use_node_fused;
  std::vector<int64_t> o;
  auto add = [&o](size_t f32, size_t f64) { o.insert(o.end(), {(int64_t)f32, (int64_t)f64}); };
  add(edge_agg_lds_bytes(s, d, sizeof(float)), edge_agg_lds_bytes(s, d, sizeof(double)));
  add(edge_bwd_lds_bytes(s, d.FeP, sizeof(float)), edge_bwd_lds_bytes(s, d.FeP, sizeof(double)));
  add(use_narrow ? edge_narrow_lds_bytes(d.Fn, d.Fe, tile.max_out_rows, tile.max_in_rows) : 0, 0);
  add(use_narrow && nt_narrow ? node_tiled_lds_bytes(d.Fn, d.Fe, nt.max_in_rows, nt.max_nodes) : 0, 0);
  add(use_ps ? edge_ps_lds_bytes(pt.max_out_rows, pt.max_in_rows, pt_gram != 0) : 0, 0);
  add(node_fused && na_num > 0 ? node_atom_lds_bytes(na_max_deg) : 0, 0);
  add(node_fused ? node_fused_lds_bytes(s) : 0, 0);
  return o;
}

std::vector<int32_t> GraphPlan::flat() const {
  std::vector<int32_t> o = {d.FnP, d.FeP};
  const Partition reserved;  // the third slot held a retired kernel's partition: written empty, so the layout keeps its positions
  for (const Partition *p : {&tile, &nt, &reserved, &bt, &pt}) {
    o.push_back((int32_t)p->begin.size());
    o.insert(o.end(), p->begin.begin(), p->begin.end());
    o.insert(o.end(), {p->max_out_rows, p->max_in_rows, p->max_nodes});
  }
  o.insert(o.end(), {nt_narrow ? 1 : 0, na_num, na_max_deg, pt_back, pt_gram, (int32_t)T});
  o.insert(o.end(), {use_fused, 0 /* reserved */, 0 /* reserved */, use_ps, use_narrow, use_node_fused, use_readout_fused, num_lanes});
  for (const std::vector<int> *v : {&out_ptr, &in_ptr, &in_edge, &in_pos, &rev_edge, &trip_off}) o.insert(o.end(), v->begin(), v->end());
  return o;
}

std::vector<int32_t> GraphPlan::flat_pairs() const {
  std::vector<int32_t> o = {(int32_t)pair_a.size()};
  for (const std::vector<int> *v : {&pair_of_edge, &pair_a, &pair_b}) o.insert(o.end(), v->begin(), v->end());
  return o;
}

}  // namespace rn
