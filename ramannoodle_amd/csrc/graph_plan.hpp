// Host-only planning of a frozen graph: validation of the create arguments, the CSRs and derived index arrays, the atom
// tiles of every kernel family and the choice of the family itself.  Nothing here calls the HIP runtime or needs a device
// (the LDS footprints and "supported" predicates come from kernels.hpp, where they sit next to their kernels), so every
// decision is reachable on a machine without a GPU through rn_potgnn_debug_plan.  api.hip uploads the result.
#pragma once

#include <string>
#include <vector>

#include "../../include/rn_potgnn.h"
#include "kernels.hpp"

namespace rn {

// Every RN_POTGNN_* environment knob that steers the plan, read in one place at create time (read_plan_knobs);
// RN_POTGNN_WIDEN is read once per process.
struct PlanKnobs {
  int widen = 2;               // WIDEN: 0 minimal power-of-two padding, 1 round 4's policy, 3 experiment
  bool vpl8 = false;           // VPL=8
  bool want_fused = true;      // FUSED
  bool want_narrow = true;     // NARROW
  bool tile_kb_set = false;
  int tile_kb = 64;            // TILE_KB (set, or VPL=8: that budget for the EdgeBlock's tiles instead of a search)
  int narrow_tile_rows = 0;    // NARROW_TILE_ROWS (experiment knob; 0: not set)
  bool bwd_tiles = true;       // BWD_TILES=0: the reverse kernel runs on the forward kernel's tiles
  bool node_tile_rows_set = false;
  int node_tile_rows = 0;      // NODE_TILE_ROWS (experiment knob)
  int node_tile_kb = 12;       // NODE_TILE_KB
  bool want_ps = true;         // EDGE_PS
  int ps_tile_rows = 0;        // PS_TILE_ROWS (experiment knob)
  int ps_back = 5;             // PS_BACK: the largest lookahead a partition may take (2 also rules out 3)
  bool want_gram = false;      // PS_GRAM
  int node_atom = -1;          // NODE_ATOM: 0 / 1 forces
  bool want_node_fused = true;     // NODE_FUSED
  bool want_readout_fused = true;  // READOUT_FUSED
  int lanes = 0;               // LANES (1 or 2; 0: by kernel family)
};
PlanKnobs read_plan_knobs();

int pad_pow2(int f);
// Which padded widths a model runs at (widen_for_fused decides where a narrower Fn / Fe pads up to the fused kernels' 64).
Dims plan_dims(const rn_potgnn_config &cfg, const PlanKnobs &knobs);
// Largest out-degree the tiled kernels take at the planned widths (554 / 292 / 147 / 71 for FeP = 16 / 32 / 64 / 128): what
// validate_create_args refuses above, from the float64 footprint of edge_agg_kernel (edge_agg_lds_bytes) on a one-atom tile.
size_t max_out_degree(Dims d);

// The checks of rn_potgnn_create that need no device, in its order (null arguments, the configuration, the weight count
// unless `num_weights` is null, the edge list, the atom types, the out-degrees).  RN_OK, or the status with its text in `error`.
// Its first part, which needs no graph: a null configuration (or `others_null`), the sizes, the widths, the weight count.
int validate_config(const rn_potgnn_config *cfg, bool others_null, const size_t *num_weights, std::string &error);
int validate_create_args(const rn_potgnn_config *cfg, const int32_t *edge_a, const int32_t *edge_b, const int32_t *atom_types,
                         bool others_null, const size_t *num_weights, std::string &error);

// Consecutive atoms grouped into tiles: tile t holds atoms begin[t] .. begin[t+1].  Empty = no such partition.
struct Partition {
  std::vector<int> begin;
  int max_out_rows = 0, max_in_rows = 0, max_nodes = 0;  // over its tiles: most out-edges, in-edges, atoms
  int num() const { return begin.empty() ? 0 : (int)begin.size() - 1; }
};

struct GraphPlan {
  int N = 0, E = 0;
  Dims d{};
  std::vector<int> edge_a, edge_b, atom_type;
  std::vector<int> out_ptr, in_ptr;  // [N+1] CSR over a / over b
  std::vector<int> in_edge, in_pos;  // [E] edge ids entering b, ascending; its inverse
  std::vector<int> rev_edge;         // [E] id of (b -> a) or -1
  std::vector<int> trip_off;         // [E+1] exclusive prefix of triplets per destination edge
  // Atom pairs: edge d and rev_edge[d] share one (what depends on {a_d, b_d} alone -- the EdgeBlock's c2 branch -- need be
  // computed once per pair).  Pairs are numbered in ascending order of their lower edge id and take
  // its atoms; an edge without a reverse, or that is its own reverse, is a pair of its own.
  std::vector<int> pair_of_edge;     // [E] compact pair index
  std::vector<int> pair_a, pair_b;   // [NP] the two atoms of each pair
  int64_t T = 0;
  Partition tile, nt, bt, pt;        // Graph::tile_begin / nt_ / bt_ / pt_ (kernels.hpp says which kernel each serves)
  bool nt_narrow = false;
  int na_num = 0, na_max_deg = 0;
  int pt_back = 2, pt_gram = 0;
  // kernel family (rn_potgnn_config_flags reports it)
  bool use_fused = false;
  bool use_ps = false;     // role-specialised fused EdgeBlock (kernels_edge_ps.hip) on its own atom tiles (Graph::pt_*)
  bool use_narrow = false;  // narrow-width kernels (kernels_narrow.hip): Fn, Fe <= 16, one lane per row
  bool use_node_fused = false;  // fused NodeBlock (only together with the fused EdgeBlock)
  bool use_readout_fused = false;  // readout MLP in one launch (same condition)
  int num_lanes = 2;

  // The scalar fields of Graph; every pointer null (api.hip's upload fills them).
  Graph scalars() const;
  // Dynamic LDS bytes (float32, float64) each kernel family would ask for on this plan, in the order documented at
  // rn_potgnn_debug_plan_lds (include/rn_potgnn.h); 0 where the family does not run.  From the kernels' own *_lds_bytes.
  std::vector<int64_t> lds_requests() const;
  // The plan as rn_potgnn_debug_plan writes it (include/rn_potgnn.h documents the layout).
  std::vector<int32_t> flat() const;
  // The pair table as rn_potgnn_debug_plan_pairs writes it: NP, pair_of_edge[E], pair_a[NP], pair_b[NP].
  std::vector<int32_t> flat_pairs() const;
};

// The arguments must have passed validate_create_args.  num_cus: compute units of the device the handle will run on.
GraphPlan plan_graph(const rn_potgnn_config &cfg, Dims d, const int32_t *edge_a, const int32_t *edge_b,
                     const int32_t *atom_types, int num_cus, const PlanKnobs &knobs);

}  // namespace rn
