// Kernel launch interface between api.hip (host orchestration) and the kernel TUs.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rn {

// Frozen reference graph on the device (all int32).
struct Graph {
  int N, E;
  const int *edge_a;   // [E]  source atom a of edge (a -> b); edges sorted by (a, b)
  const int *edge_b;   // [E]  destination atom b
  const int *out_ptr;  // [N+1] CSR over a: edges out_ptr[a]..out_ptr[a+1] leave a
  const int *in_ptr;   // [N+1] CSR over b
  const int *in_edge;  // [E]  edge ids entering b, ascending
  const int *in_pos;   // [E]  inverse of in_edge: position of edge e in the (b, a) order
  const int *atom_type;  // [N]
  const int *rev_edge;   // [E]  id of the reverse edge (b -> a), or -1
  // atom pairs (GraphPlan::pair_of_edge): edge d and rev_edge[d] share pair_of_edge[d]; pair p joins atoms pair_a[p], pair_b[p]
  int NP;
  const int *pair_of_edge;  // [E]
  const int *pair_a, *pair_b;  // [NP]
  // node tiles for the edge-block kernel
  int num_tiles;
  const int *tile_begin;  // [num_tiles+1] node ranges
  int max_tile_out_rows;  // LDS rows needed by the largest tile
  int max_tile_in_rows;   // most destination edges entering one tile
  int max_tile_nodes;     // most atoms in one tile
  // node tiles of the fused NodeBlock kernel (its own partition: it holds no Q' rows, so its tiles can
  // be larger than the EdgeBlock's and fill their rounds better)
  int nt_num;
  const int *nt_begin;    // [nt_num+1] node ranges
  int nt_max_in_rows, nt_max_nodes;
  int nt_narrow;          // the partition was made for node_tiled_kernel (kernels_narrow.hip)
  // atom-owning fused NodeBlock (kernels_node_atom.hip): tiles of 16 consecutive atoms, round r = their r-th in-edges
  int na_num;             // ceil(N / 16), or 0 when that kernel does not serve the graph
  int na_max_deg;         // largest in-degree
  // node tiles of the role-specialised EdgeBlock (kernels_edge_ps.hip: one twelve-wave workgroup per CU, 16 destinations a round)
  int pt_num;
  const int *pt_begin;    // [pt_num+1] node ranges
  int pt_max_out_rows, pt_max_in_rows;
  int pt_back;            // rounds that may still read the ring when a step rewrites it (2 .. 5: edge_ps_tile_ok, the largest the ring has room for)
  int pt_gram;            // 1: the GRAM instantiation (LayerNorm cross terms on the matrix pipe; a 7-tile ring + the Gram tables)
  // node tiles of the EdgeBlock reverse kernel (edge_bwd_tile2_kernel): small enough for TWO workgroups per CU
  int bt_num;
  const int *bt_begin;    // [bt_num+1] node ranges
  int bt_max_out_rows, bt_max_in_rows, bt_max_nodes;
  // triplet enumeration
  const int *trip_off;  // [E+1] exclusive prefix of triplets per destination edge
  int64_t T;
};

// One LayerNorm's affine parameters (device pointers, padded with zeros).
template <typename T>
struct Ln {
  const T *g, *b;
};

template <typename T>
struct PassW {
  const T *c1_WnT;   // [FnP][2FnP]   node part of c1_linear, transposed, [filter|core]
  const T *c1_WeT;   // [FeP][2FnP]   edge part
  const T *c1_bias;  // [2FnP]
  Ln<T> c1_norm;     // [2FnP]
  Ln<T> final_norm;  // [FnP]
  const T *c2_WT;    // [FnP][2FeP]
  const T *c2_bias;  // [2FeP]
  Ln<T> c2_norm_1;   // [2FeP]
  Ln<T> c2_norm_2;   // [FeP]
  const T *c3_WnT;   // [FnP][6FeP]   (W_i | W_j | W_k) node parts of c3_linear
  const T *c3_nshift;  // [6FeP]      (0 | c3 bias | 0)
  const T *c3_WeT;   // [FeP][4FeP]   (W_4 | W_5) edge parts: dest-edge | source-edge
  Ln<T> c3_norm_1;   // [2FeP]
  Ln<T> c3_norm_2;   // [FeP]
  Ln<T> c3_norm_1s;  // [2FeP] c3_norm_1 times the gate's exp2 scales (-log2e on the filter half, 2 log2e on the core half)
  Ln<T> c2_norm_1s;  // [2FeP] c2_norm_1 and
  Ln<T> c1_norm_s;   // [2FnP] c1_norm in the same form (kernels_narrow.hip)
  const T *mfma_scale;  // [8] split-f16 prescales (s, 1/s) of c1_WeT | c3_WeT[:, W4] | c3_WeT[:, W5] | c2_WT (mfma_prescale)
  // c3_linear / c2_linear centred over their real output columns (LayerNorm(x) = LayerNorm(x - mean x), and the
  // mean is linear in the inputs): projections with these come out with zero row mean (kernels_edge_ps.hip)
  const T *c3_WeT_c;    // [FeP][4FeP]
  const T *c3_WnT_c;    // [FnP][6FeP]
  const T *c3_nshift_c; // [6FeP]
  const T *c2_WT_c;     // [FnP][2FeP]
  const T *c2_bias_c;   // [2FeP]
  // c1_linear centred the same way (the fused NodeBlock then needs no LayerNorm(2Fn) mean either)
  const T *c1_WnT_c;    // [FnP][2FnP]
  const T *c1_WeT_c;    // [FeP][2FnP]
  const T *c1_bias_c;   // [2FnP]
  const T *mfma_scale_c;  // [8] split-f16 prescales (s, 1/s) of c3_WeT_c[:, W4] | c3_WeT_c[:, W5] | c2_WT_c | c1_WeT_c
  int c3_fast;       // host-side decision: c3_norm_1 admits the folded-scale triplet loop
                     // (bit 0: in the fused EdgeBlock kernel, bit 1: in edge_agg_kernel)
};

template <typename T>
struct ReadoutW {
  // HP = max(FeP, 32): hidden width of the readout MLP as stored
  const T *W0T;  // [FeP][HP]
  const T *scale0, *shift0;  // [HP] BatchNorm(eval) folded with bias 0: ssp(acc*scale+shift)
  const T *W3T;  // [HP][HP]
  const T *b3;   // [HP]
  const T *W5T;  // [HP][32]  (12 real columns)
  const T *b5;   // [32]
  const T *mfma_scale;  // [8] split-f16 prescales (s, 1/s) of W0T | W3T | W5T (mfma_prescale)
};

// Power-of-two prescale of a weight matrix for the split-f16 matrix products (device_utils.hpp):
// s = 2^(12 - floor(log2 m)) for m = max |w|, so that s w lies in [2^12, 2^13) -- inside f16's
// normal range whatever the scale of the weights, with every entry down to 2^-15 of the largest
// one keeping its full 22 bits.  Exact (a power of two); the inverse is applied to the float32
// accumulator.  Same bit arithmetic on the host (pack_weights) and on the device (kernels_train.hip).
__host__ __device__ inline float mfma_prescale(float m) {
  union { float f; unsigned u; } b;
  b.f = m;
  const unsigned ex = (b.u >> 23) & 0xffu;
  if (!(m > 0.0f) || ex == 0xffu) return 1.0f;  // zero, negative, NaN, inf: leave unscaled
  int e = (int)ex - 127;
  if (e < -126) e = -126;
  int se = 12 - e;
  se = se < -126 ? -126 : (se > 126 ? 126 : se);
  b.u = (unsigned)(se + 127) << 23;
  return b.f;
}

struct Dims {
  int Fn, Fe, FnP, FeP;  // logical and padded (pow2 >= 16) embedding widths
};

// ---- launchers (all asynchronous on `st`) ----
template <typename T>
void launch_setup(const T *emb, const T *W2, const T *b2, const T *W4, const T *b4, int K,
                  Dims d, T *node_table, const T *b0, const T *bn_w, const T *bn_b,
                  const T *bn_rm, const T *bn_rv, T *scale0, T *shift0, hipStream_t st);

template <typename T>
void launch_geom_rbf(const double *pos, int S, const Graph &g, const T *lattice,
                     int lat_stride /* 0: one lattice for every frame; 9: lattice[S][9] */,
                     const T *offsets, T coef, Dims d, T *unit4, T *edge0, hipStream_t st,
                     bool in_order = false /* rows in (b, a) order: the narrow kernels' layout */);
// "Pair" edge rows (float32 evaluations on the role-specialised EdgeBlock + atom-owning NodeBlock + fused readout, FeP = 64):
// a row's 256 bytes hold, for each group m of eight columns, [f16 hi x8][f16 lo x8] with hi = f16(x), lo = f16(x - hi) --
// the split-f16 MFMA operand itself (device_utils.hpp), written once by the kernel that produces the row instead of being
// re-derived by each of its three consumers; x = hi + lo to 2^-25 absolute for |x| < 1 (tanh / Gaussian outputs).
void launch_geom_rbf_pairs(const double *pos, int S, const Graph &g, const float *lattice, int lat_stride, const float *offsets,
                           float coef, Dims d, float *unit4, float *edge0, hipStream_t st);
// The two float32 geometry kernels on positions that are float32 already (cast on the host while staging: bit-identical rows)
void launch_geom_rbf_pos32(const float *pos, int S, const Graph &g, const float *lattice, int lat_stride, const float *offsets,
                           float coef, Dims d, float *unit4, float *edge0, hipStream_t st, bool in_order);
void launch_geom_rbf_pairs_pos32(const float *pos, int S, const Graph &g, const float *lattice, int lat_stride,
                                 const float *offsets, float coef, Dims d, float *unit4, float *edge0, hipStream_t st);

template <typename T>
void launch_node_init(const T *table, int S, const Graph &g, Dims d, T *node,
                      const int *types /* [S*N] atom type per (sample, atom), or null: g.atom_type */, hipStream_t st);

// Y[M, NOUT] = act(X[M, KP] * WT[KP, NOUT] * scale + shift)
//   amode 0: X rows are read from `X` (row stride KP)
//   amode 1: X row r = node[s*N + b_e] * node[s*N + a_e]  (r = s*E + e)   -- c2 input
template <typename T>
void launch_rowgemm(const T *X, int64_t M, int KP, const T *WT, int NOUT, T *Y,
                    const T *scale, const T *shift, bool act, int amode, const T *node,
                    const Graph &g, hipStream_t st);

// float32 only: Y (+)= X[:, 0:N] * Wt[N, NOUT] on the MFMA kernel; false if the shape is unsupported
// LDS bytes of edge_bwd_tile2_kernel for a tile with these maxima (element size 4 or 8)
size_t edge_bwd_tile2_lds_bytes(int rows, int in_rows, int nodes, int FP, size_t elem);
// dynamic LDS bytes the reverse EdgeBlock asks for on this graph: the two-pass kernel on the bt_ tiles (or the forward
// tiles), else the one-pass tile kernel, else 0 -- the per-row kernel that takes what fits neither uses no dynamic LDS
size_t edge_bwd_lds_bytes(const Graph &g, int FP, size_t elem);
// split-f16 row product for the reverse pass (kernels_gemm.hip: rowgemm_split_kernel); false = shape not served
bool launch_rowgemm_split(const float *X, int ldx, int K, int64_t M, const float *Wt, int NOUT, float *Y,
                          bool accumulate, const float *bias, int amode, const float *node, const Graph &g,
                          hipStream_t st);
bool launch_rowgemm_blocks(const float *X, int ldx, int N, int64_t M, const float *Wt, int NOUT,
                           float *Y, bool accumulate, const Graph &g, hipStream_t st);

template <typename T>
void launch_node_agg(const T *npc1, const T *bc1, const T *node_in, T *node_out, int S,
                     const Graph &g, Dims d, const PassW<T> &w, hipStream_t st);

// (returns what hipFuncSetAttribute or the launch answered: a tile that asks for more LDS than the CU has is an error of
//  the call, never a silent no-op)
template <typename T>
hipError_t launch_edge_agg(const T *pq, const T *np3, const T *c2pre, const T *edge_in,
                           T *edge_out, int S, const Graph &g, Dims d, const PassW<T> &w,
                           T *agg_out /* optional tape of the pre-LayerNorm triplet sums */,
                           hipStream_t st);

template <typename T>
void launch_readout_reduce(const T *pol, const T *unit4, int S, const Graph &g,
                           const double *mean9, const double *std9, float *vec6,
                           double *alpha, double *alpha_raw, hipStream_t st, int pol_stride = 32 /* floats between rows of pol */);

void launch_radius_graph(const double *lattice, const double *pos, int N, float cutoff,
                         unsigned char *adjacency, hipStream_t st);

void launch_enum_triplets(const Graph &g, int *idx_i, int *idx_j, int *idx_k, int *slot5,
                          int *slot6, hipStream_t st);

// LDS of one CU (gfx950): no workgroup can ask for more
constexpr size_t kCuLdsBytes = 160 * 1024;
// dynamic LDS bytes edge_agg_kernel asks for on the tiles of `g` (max_tile_out_rows, max_tile_in_rows, max_tile_nodes)
size_t edge_agg_lds_bytes(const Graph &g, Dims d, size_t elem);

// ---- reverse mode w.r.t. activations / positions (kernels_bwd.hip).  C cotangent
// instances, B per forward frame.
template <typename T>
void launch_gemm_nt(const T *X, int64_t R, int N, const T *W, int ldw, int K, T *Y, bool accumulate,
                    hipStream_t st);
template <typename T>
void launch_readout_bwd(const T *dout6, const T *pol, const T *unit4, int C, int B, const Graph &g,
                        T *dpol, T *dunit, hipStream_t st);
template <typename T>
void launch_ssp_bwd(T *d, const T *h, const T *scale, int64_t rows_per_frame, int width, int C,
                    int B, hipStream_t st);
template <typename T>
hipError_t launch_edge_bwd(const T *pq, const T *np3, const T *c2pre, const T *edge_next,
                           const T *agg /* taped pre-LayerNorm triplet sums [S*E, FeP] */,
                           const T *dedge_next, T *dedge_prev, T *dpq, T *dnp3, T *dc2pre, int C, int B,
                           const Graph &g, Dims d, const PassW<T> &w, const PassW<T> *grad_w,
                           hipStream_t st);  // grad_w: same layout as w inside the gradient blob, or null
template <typename T>
void launch_prod_fwd(const T *node, T *prod, int64_t rows, const Graph &g, Dims d, hipStream_t st);
template <typename T>
void launch_prod_bwd(const T *dprod, const T *node, T *dnode, int C, int B, const Graph &g, Dims d,
                     hipStream_t st);
template <typename T>
void launch_node_bwd(const T *npc1, const T *bc1, const T *node_next, const T *dnode_next,
                     T *dnode_prev, T *dbc1, T *dnpc1, int C, int B, const Graph &g, Dims d,
                     const PassW<T> &w, const PassW<T> *grad_w, hipStream_t st);
// ---- training pieces (weight gradients, BatchNorm in training mode, embedding MLP)
// Deferred reduction of the weight-gradient products (float32 MFMA path): every product stores one
// [K+1][N] slice per workgroup into `arena`; launch_tn_reduce sums the slices of all products recorded
// in `table` with one launch (and resets the record).
struct TnReduceOp {
  const float *part;
  float *dst, *dbias;
  int nblk, K, N, ldw;
};
struct TnReduceTable {
  static constexpr int MAX_OPS = 32;
  TnReduceOp ops[MAX_OPS];
  int wg_begin[MAX_OPS + 1];
  int num;
};
struct TnDeferred {
  float *arena = nullptr;
  size_t capacity = 0, used = 0;  // in floats
  TnReduceTable table{};
};
size_t tn_partial_elems(int64_t R, int K, int N);
void launch_tn_reduce(TnDeferred &df, hipStream_t st);
template <typename T>
void launch_gemm_tn(const T *X, int ldx, const T *dY, int ldy, int64_t R, int K, int N, T *dWT,
                    int ldw, T *dbias, int amode, const T *node, const Graph &g, hipStream_t st,
                    TnDeferred *defer = nullptr);
template <typename T>
void launch_bn_col_sums(const T *z, int64_t R, int W, double *stats, hipStream_t st);
template <typename T>
void launch_bn_train_apply(const T *z, int64_t R, int W, int F, const double *stats, double count,
                           const T *gamma, const T *beta, T *h, T *mv, hipStream_t st);
template <typename T>
void launch_bn_bwd_sums(const T *d, const T *z, int64_t R, int W, int F, const double *stats, double count,
                        double *sums, hipStream_t st);
template <typename T>
void launch_bn_bwd_apply(T *d, const T *z, int64_t R, int W, int F, const double *stats, double count,
                         const double *sums, const double *own_sums, const T *gamma, T *dgamma, T *dbeta,
                         hipStream_t st);
template <typename T>
void launch_node_embed_bwd(const T *dnode0, int S, const Graph &g, Dims d, int K, const T *emb,
                           const T *W2, const T *b2, const T *W4, T *demb, T *dW2, T *db2, T *dW4,
                           T *db4, T *type_sums_scratch,
                           const int *types /* [S*N] atom type per (sample, atom), or null: g.atom_type */, hipStream_t st);
template <typename T>
void launch_geom_bwd(const T *dedge0, const T *dunit, const T *unit4, const T *lat, const T *offs,
                     T coef, int C, int B, const Graph &g, Dims d, double *dpos, hipStream_t st);
// Input gradients of the forward (kernels_bwd.hip: geom_input_bwd_kernel): d(edge0), d(unit) -> dpos float64 [C][N][3]
// (fractional positions) and / or dlat float64 [C][9] (the frame's lattice, row i = lattice vector i), each written
// once per entry; either may be null.  `pos` float64 [S][N][3] and `lat` ([9] with lat_stride 0, [S][9] with 9) are
// what the taped forward ran on; `dcart`: scratch of C * E * 3 doubles.
template <typename T>
void launch_geom_input_bwd(const T *dedge0, const T *dunit, const T *unit4, const double *pos, const T *lat,
                           int lat_stride, const T *offs, T coef, int C, int B, const Graph &g, Dims d, double *dcart,
                           double *dpos, double *dlat, hipStream_t st);
template <typename T>
void launch_cast_from_f64(const double *src, T *dst, int64_t n, hipStream_t st);
// The most atom groups a call may name (the group entries of api.hip and rn_md_raman_partial; MAX_GROUPS in spectrum.py).
constexpr int kMaxGroups = 16;

// Atom-group contraction (kernels_group.hip: group_increment_kernel): for steps t < `steps` and groups g < G,
// out[t][g][9] = sigma (.) sum_{i in g} 1/2 (J(t)_i + J(t+1)_i) . dx_{t,i}, J float64 [.][6][N][3] frames `jac_stride`
// doubles apart (0: one Jacobian for every t); dx = the minimum image of pos[t+1] - pos[t] (pos float64 [steps+1][N][3])
// or, with `disp` float64 [steps][N][3], disp_scale * disp[t].  perm [N] / gptr [G+1]: the atoms of group g are
// perm[gptr[g] .. gptr[g+1]).  Written once per entry, no atomics.  out_groups > G: the rows of `out` hold that many
// channels ([t][out_groups][9]) and the kernel fills the first G (0: G).
void launch_group_increments(const double *jac, int64_t jac_stride, const double *pos, const double *disp,
                             double disp_scale, int64_t steps, int N, const int *perm, const int *gptr, int G,
                             const double *sigma, double *out, hipStream_t st, int out_groups = 0);
// The cell's share of a variable-cell step (kernels_group.hip: cell_increment_kernel): for t < `steps`,
// out[t][channel][9] = sigma (.) 1/2 (J_L(t) + J_L(t+1)) : (lat[t+1] - lat[t]), jl float64 [steps+1][6][9] (the dlat rows of
// launch_geom_input_bwd for six one-hot cotangents per frame), lat float64 [steps+1][9]; `out` as above.
void launch_cell_increments(const double *jl, const double *lat, int64_t steps, int channel, int out_groups,
                            const double *sigma, double *out, hipStream_t st);
// Phonon-mode contraction (kernels_mode.hip: mode_increment_kernel, float64 MFMA): for steps t < `steps` and modes m < M,
// out[t][m][3r+s] = sigma[3r+s] a_{map(r,s)}[t][m] q[t][m], a_c = 1/2 (J_c(t) + J_c(t+1)) . disp[m], q = proj[m] . dx_t;
// jac float64 [steps+1][6][N][3], pos float64 [steps+1][N][3], disp / proj float64 [M][N][3], M <= kMaxModes, out
// float64 [steps][out_channels][9] with out_channels >= M.  Written once per entry, no atomics.
constexpr int kMaxModes = 64 * 65535;  // gridDim.y of mode_increment_kernel
void launch_mode_increments(const double *jac, const double *pos, int64_t steps, int N, const double *disp,
                            const double *proj, int M, const double *sigma, int out_channels, double *out,
                            hipStream_t st);
// The rest channel (kernels_mode.hip: mode_rest_kernel), after launch_mode_increments on the same stream:
// out[t][M] = the one-group increment of launch_group_increments - sum_{m<M} out[t][m] (ascending m); out_channels > M.
void launch_mode_rest(const double *jac, const double *pos, int64_t steps, int N, int M, const double *sigma,
                      int out_channels, double *out, hipStream_t st);

// Covariance moments of quasi-harmonic mode analysis (kernels_covariance.hip; include/rn_quasiharmonic.h states them):
// pos float64 [.][K]; chunks int64 [num_chunks][3] = (first frame, frames, steps) in ascending frames; block_chunks
// int64 [B + 1], the chunks of block b; ws float64 [covariance_workspace_doubles]; first_ws float64 [num_chunks][K];
// -> first float64 [B][K], second float64 [B][2][K][K].  All device pointers; B <= 65535 and num_chunks
// covariance_pairs(K) < 2^31 (the grid).
constexpr int kCovarianceChunkFrames = 512;  // the frames of a chunk: a multiple of the kernel's k-tile of 16
// pair p of the lower triangle of a matrix of tiles, row-major: (0,0) (1,0) (1,1) (2,0) ..  (also kernels_band.hip)
__device__ inline void lower_pair(int p, int &I, int &J) {
  I = 0;
  while ((I + 1) * (I + 2) / 2 <= p) ++I;
  J = p - I * (I + 1) / 2;
}
int covariance_pairs(int64_t K);
size_t covariance_workspace_doubles(int64_t K, int64_t num_chunks);
void launch_covariance_chunks(const double *pos, int64_t K, const double *anchor, const int64_t *chunks,
                              int64_t num_chunks, double *ws, double *first_ws, hipStream_t st);
void launch_covariance_reduce(const double *ws, const double *first_ws, int64_t K, const int64_t *block_chunks, int64_t B,
                              double *first, double *second, hipStream_t st);

// Structure descriptors (kernels_pool.hip): desc float64 [S][Fe] = the mean over a frame's E edge rows of the Fe real
// columns of `edge`, [S][E] rows of FeP columns in one of three layouts: float32, split-f16 pairs ([hi x 8][lo x 8] per
// group of eight columns, the bytes of a float32 row) or float64.  edge_pool_supported: FeP is a whole number of 16-byte
// (pairs: 32-byte) groups, at most 256 of them.
enum class EdgeRows { kFloat32, kPairs, kFloat64 };
bool edge_pool_supported(EdgeRows rows, int FeP);
void launch_edge_pool(const void *edge, EdgeRows rows, int S, int E, int Fe, int FeP, double *desc, hipStream_t st);

// Nearest reference row and farthest-point selection (kernels_select.hip;include/rn_select.h states them): X float64
// [S][D], R float64 [M][D], params float64 [2][D] = (center, scale).  All device pointers; the grids need S, M < 2^31.
constexpr int kSelectTile = 64;       // rows of X and of R per tile of the search
constexpr int kSelectSliceRows = 128; // rows of X a workgroup of the selection owns
struct SelectBest {                   // a candidate of a search (key ascending) or of a pick (value descending)
  double value;
  int64_t index;
};
// the ascending ranges of whole tiles a reference of M rows is split into for S rows of X, and the tiles of a range
void select_splits(int64_t S, int64_t M, int64_t *splits, int64_t *tiles_per_split);
// norms[j] = sum_c ((R[j][c] - center[c]) scale[c])^2, ascending c
void launch_select_norms(const double *R, int64_t M, int64_t D, const double *params, double *norms, hipStream_t st);
// partials [splits][S]: per row of X the lowest (|r'|^2 - 2 x'.r', j) of the range, (+inf, -1) when it has no candidate
void launch_select_search(const double *X, int64_t S, const double *R, int64_t M, int64_t D, const double *params,
                          const double *norms, int exclude_self, SelectBest *partials, hipStream_t st);
// index[s] = the lowest candidate over the ranges (ascending, the lowest index on equal keys); dist2[s] from differences
void launch_select_merge(const double *X, int64_t S, const double *R, int64_t M, int64_t D, const double *params,
                         const SelectBest *partials, double *dist2, int64_t *index, hipStream_t st);
// mean [D] = the column means of X, in a fixed order; mind[s] = d2(X_s, mean); mind[s] = value
void launch_select_column_mean(const double *X, int64_t S, int64_t D, double *mean, hipStream_t st);
void launch_select_distance_to(const double *X, int64_t S, int64_t D, const double *params, const double *point,
                               double *mind, hipStream_t st);
void launch_select_fill(double *mind, int64_t S, double value, hipStream_t st);
// partials [select_slices(S)]: per slice of rows the highest (mind, s), the lowest s on equal values
int64_t select_slices(int64_t S);
void launch_select_argmax(const double *mind, int64_t S, SelectBest *partials, hipStream_t st);
// One pick.  p = forced >= 0 ? forced : the highest of partials_in; picks[step] = p, pick_dist2[step] = first_of_none ?
// +inf : its value; then, unless `last`, mind[s] = first_of_none ? d2(X_s, X_p) : min(mind[s], d2(X_s, X_p)), mind[p] =
// -1 (picked: below every distance), and the slices' highest go to partials_out.
void launch_select_pick(const double *X, int64_t S, int64_t D, const double *params, double *mind,
                        const SelectBest *partials_in, SelectBest *partials_out, int64_t forced, int first_of_none, int last,
                        int64_t step, int64_t *picks, double *pick_dist2, hipStream_t st);

// Harmonic trajectories (kernels_harmonic.hip; include/rn_harmonic.h states them): ref float64 [K], D float64 [M][K],
// omega_dt float64 [M], amp / phase float64 [R][M] -> out float64 [R][T][K], frame t of a call being the absolute frame
// t0 + t.  All device pointers; harmonic_workgroups is the grid of the launch, -1 when it exceeds 2^31 - 1 workgroups.
int64_t harmonic_workgroups(int64_t K, int64_t R, int64_t T);
void launch_harmonic_synthesis(const double *ref, const double *D, const double *omega_dt, const double *amp,
                               const double *phase, int64_t K, int M, int64_t R, int64_t T, int64_t t0, double *out,
                               hipStream_t st);

// Band moments (kernels_band.hip; include/rn_bandmodes.h states them).  All device pointers but `lattice` (host, [9]).
// pos float64 [.][K], alpha float64 [.][9] or null (then Kc == K, else Kc == K + 6), sqrt_mass float64 [K / 3], starts
// int64, taper float64 [n], table float64 [n][2] (launch_band_phases), row_bins int32 [Rp]: the bin of row 2 i + part,
// -1 for the padding; Rp = band_padded(2 U).  V float64 [count][Rp][band_padded(Kc)]: the transforms of segments q0 ..
// q0 + count - 1.  launch_band_update: rows = count * Rp rows of V, weights float64 [B][Rp], ws float64
// [band_partial_doubles(Kc, B, rows)] -> moments float64 [B][Kc][Kc] (accumulate = 1: added to what is there).
// B <= 65535, band_chunks(rows) * band_pairs(Kc) and band_transform_workgroups (-1 when too many) < 2^31: the grids.
constexpr int kBandChunkRows = 512;  // the rows of V per chunk of the update: a multiple of its k-tile of 16
int64_t band_padded(int64_t count);
int band_pairs(int64_t Kc);
int64_t band_chunks(int64_t rows);
size_t band_partial_doubles(int64_t Kc, int64_t B, int64_t rows);
int64_t band_transform_workgroups(int64_t Kc, int64_t Rp, int64_t count);
void launch_band_phases(int64_t n, double *table, hipStream_t st);
void launch_band_transform(const double *pos, const double *alpha, const double *lattice, const double *sqrt_mass,
                           int64_t K, int64_t Kc, int64_t n, const int64_t *starts, int64_t q0, int64_t count,
                           const double *taper, const double *table, const int *row_bins, int64_t Rp, double *V,
                           hipStream_t st);
void launch_band_update(const double *V, int64_t rows, int64_t Rp, int64_t Kc, const double *weights, int64_t B,
                        int accumulate, double *ws, double *moments, hipStream_t st);

// The interpolation model on the device (kernels_interp.hip; api_interp.hip owns the arrays).  Everything float64:
// F [J][K3] the basis with the lattice folded in and FT [K3][J] its transpose, ref [K3] the reference positions,
// alpha_ref [9], poff [J+1] the piece offsets, xs the breakpoints (DOF j's P_j + 1 values start at poff[j] + j),
// coef [pieces][order+1][9] Taylor coefficients about each piece's left breakpoint (ascending power, zero-padded to the
// model's highest order `order` in 1..5), scale [J] = 1 - mask, Pmax the largest piece count of a DOF.
struct InterpModel {
  const double *F, *FT, *ref, *alpha_ref, *xs, *coef, *scale;
  const int *poff;
  int64_t K3;
  int J, order, Pmax;
};
// alpha float64 [S][9] of the frames pos float64 [S][K3] (interp_alpha_kernel): written once per entry, no atomics.
void launch_interp_alpha(const double *pos, int64_t S, const InterpModel &m, double *alpha, hipStream_t st);
// Jacobian rows jac float64 [S][6][K3] (component order of launch_group_increments) of the frames pos; g: workspace
// of S * 6 * J doubles (the scaled spline derivatives).  Two launches on `st`, no atomics.
void launch_interp_jacobian(const double *pos, int64_t S, const InterpModel &m, double *g, double *jac, hipStream_t st);

// Fused EdgeBlock (kernels_fused.hip): projections + triplet aggregation in one launch.
// Fused EdgeBlock (kernels_fused.hip): float32, FnP == FeP == 64.  Two workgroups per CU
// need their LDS footprint within this budget.
constexpr size_t kFusedLdsBudget = 80 * 1024;
// (edge_fused_lds_bytes: the footprint of the per-frame kernel retired in round 5 -- see profiles/r04/mfma_k32.txt and git
// history; the planner still sizes the EdgeBlock's atom tiles and decides use_fused with it, so it stays)
size_t edge_fused_lds_bytes(const Graph &g);
size_t edge_fused_lds_bytes(int tile_out_rows, int tile_in_rows, int tile_nodes);
bool edge_fused_supported(const Graph &g, Dims d);
size_t node_fused_lds_bytes(const Graph &g);
size_t node_fused_lds_bytes(int tile_in_rows, int tile_nodes);
// `f16`: matrix products as three split-f16 MFMAs (device_utils.hpp) instead of the exact-f32 MFMA
void launch_readout_fused(const float *edge, int64_t M, const ReadoutW<float> &w, float *pol, bool f16,
                          hipStream_t st, bool pair_rows = false, int pol_stride = 32 /* 16: rows of exactly the 16 columns written */);
// `centred`: npc1 was projected with c1_WnT_c / c1_bias_c and the kernel multiplies with c1_WeT_c: zero row mean, the
// LayerNorm(2Fn) in front of the gate needs the sum of squares only (split-f16 instantiations)
size_t node_atom_lds_bytes(int max_deg);
// (split-f16 products on the centred c1_linear only: PassW::c1_WeT_c, npc1 from c1_WnT_c / c1_bias_c)
void launch_node_atom(const float *edge, const float *node_in, const float *npc1, float *node_out, int S, const Graph &g,
                      Dims d, const PassW<float> &w, hipStream_t st, bool pair_rows = false);
void launch_node_fused(const float *edge, const float *node_in, const float *npc1, float *node_out, int S,
                       const Graph &g, Dims d, const PassW<float> &w, bool f16, bool centred, hipStream_t st);
// Role-specialised fused EdgeBlock (kernels_edge_ps.hip): float32, FnP == FeP == 64, split-f16 products, folded gate
// scale; needs the centred weight copies of PassW and np3 projected with c3_WnT_c / c3_nshift_c.
size_t edge_ps_lds_bytes(int tile_out_rows, int tile_in_rows, bool gram);
int edge_ps_ring_tiles(bool gram);  // ring capacity in 16-row tiles
int edge_ps_gram_window();          // source tiles a round's window may span in the GRAM instantiation
// one tile's destinations (first and end source row of each, sorted by atom): does the producers' schedule hold?
// `back`: rounds g - back .. g - 1 may still be reading the ring when the step of round g rewrites it (2 .. 5 in product handles); `ring`: its
// capacity in tiles; `window` (optional, out): the most source tiles one round's window spans
bool edge_ps_tile_ok(const int *rb, const int *re, int D, int back, int ring, int *window);
// `fail`: device int, set to a nonzero code if a bounded spin wait inside the kernel ran out (never in a correct run)
void launch_edge_ps(const float *edge_in, float *edge_out, const float *node, const float *np3, float *agg_out, int S,
                    const Graph &g, Dims d, const PassW<float> &w, int *fail, hipStream_t st, bool pair_rows = false,
                    bool f16 = true /* false: exact-f32 MFMA products (float32 rows, no Gram tables) */,
                    const float *c2_rows = nullptr /* [S, g.NP, 64] from launch_c2_pairs: the kernel computes no c2 branch of its
                                                      own (pair rows, split-f16 products, eight-lane form without Gram tables) */);
// may launch_edge_ps take c2 rows for this graph and these options?
bool edge_ps_takes_c2_rows(const Graph &g, bool pair_rows, bool f16);

// The EdgeBlock's c2 branch once per atom pair (kernels_c2_pairs.hip): out[S, g.NP, 64] float32 = LN(gate(LN(c2_linear(
// node[pair_b] * node[pair_a])))) on the centred, prescaled c2_linear -- the rows launch_edge_ps takes as `c2_rows`.
// float32, FnP == FeP == 64, split-f16 products.
void launch_c2_pairs(const float *node, float *out, int S, const Graph &g, Dims d, const PassW<float> &w, hipStream_t st);

// Device-resident optimisation step (kernels_train.hip); offsets index the packed weight blob.
struct DerivedOp {
  int kind;        // 0: transposed copy of a [K][N] block, 1: scaled copy of K values,
                   // 2: dst[0..1] = (s, 1/s), s = mfma_prescale(max |src[k * ld + n]|), ld = (int)scale
                   // 3: dst[k][n] = src[k][n] - mean over the REAL columns of n's [filter | core] block (2 FeP wide, the
                   //    first Fe of each half real; padded columns stay 0), rows of N = ld columns: the centred copies
                   //    of c3_linear / c2_linear (kernels_edge_ps.hip)
  int K, N;
  float scale;
  size_t src, dst;
  int Fe = 0, FeP = 0;  // kind 3
};
// (kind 2 entries that read a kind 3 result go into a second launch: blocks of one launch run concurrently)
void launch_adam(float *w, const float *g, float *m, float *v, const unsigned char *trainable, size_t n,
                 double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                 hipStream_t st, const int *poisoned = nullptr /* device word: non-zero = apply nothing */);
void launch_refresh_derived(float *w, const DerivedOp *ops, int num_ops, hipStream_t st);
// staging[dst .. dst + n) = w[src .. src + n) for every (src, dst, n) of `seg` (kernels_train.hip)
void launch_gather_segments(const float *w, const long long *seg, int nseg, float *staging, hipStream_t st);
void launch_bn_running(float *running_mean, float *running_var, const float *batch_mean, const float *batch_var,
                       int F, double momentum, double unbias, hipStream_t st);

// Narrow-width kernels (kernels_narrow.hip): one lane per row, compile-time (Fn, Fe) <= 16, float32.
bool narrow_supported(Dims d);
size_t edge_narrow_lds_bytes(int fn, int fe, int tile_out_rows, int tile_in_rows);
size_t node_tiled_lds_bytes(int fn, int fe, int tile_in_rows, int tile_nodes);
void launch_node_narrow(const float *edge, const float *node_in, float *node_out, int S, const Graph &g, Dims d,
                        const PassW<float> &w, hipStream_t st);
void launch_edge_narrow(const float *edge_in, float *edge_out, const float *node, int S, const Graph &g, Dims d,
                        const PassW<float> &w, hipStream_t st);
void launch_readout_narrow(const float *edge, const float *unit4, int S, const Graph &g, Dims d,
                           const ReadoutW<float> &w, const double *mean9, const double *std9, float *vec6,
                           double *alpha, double *alpha_raw, float *pol /* optional [S*E,32] */, hipStream_t st);

}  // namespace rn
