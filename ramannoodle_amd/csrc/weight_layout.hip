// Host-only packed weight layout (weight_layout.hpp).  A .hip file only because kernels.hpp, whose structs it fills, is a
// HIP header; it holds no kernel and calls nothing of the HIP runtime.
#include "weight_layout.hpp"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

namespace rn {

namespace {

// Column of the padded [filter | core] layout for original output row r of a Linear /
// LayerNorm of logical width 2F (first F rows = filter, last F = core; _gnn.py:143).
inline int gated_col(int r, int F, int FP) { return r < F ? r : FP + (r - F); }

// One tensor of the state dict, [rows][columns] row-major.  Its columns are cut into at most two pieces, a piece into
// `blocks` blocks of `width` columns; element (r, block b, column k of the block) lives at
//   dst + k * ld + b * block_stride + row(r),   row(r) = gated_col(r, F, FP) when F > 0, else r.
// A vector is `rows` rows of one column (ld = 0); a plain copy of a matrix is a vector of all its elements; a transposed
// Linear has ld = the packed leading dimension; c3_linear is 3 node-column blocks into c3_WnT and 2 edge-column blocks into c3_WeT.
struct Piece {
  int width, blocks;
  size_t dst;
  int ld, block_stride;
};
struct Tensor {
  int rows, F, FP;
  bool buffer;  // a buffer of the state dict, not a parameter
  int pieces;
  Piece piece[2];
};

std::vector<Tensor> state_dict_tensors(const PackedLayout &L) {
  const int K = L.K, Fn = L.d.Fn, Fe = L.d.Fe, FnP = L.d.FnP, FeP = L.d.FeP, HP = L.HP;
  std::vector<Tensor> t;
  auto vec = [&](size_t dst, int n, bool buffer = false) { t.push_back({n, 0, 0, buffer, 1, {{1, 1, dst, 0, 0}}}); };
  auto gated = [&](size_t dst, int F, int FP) { t.push_back({2 * F, F, FP, false, 1, {{1, 1, dst, 0, 0}}}); };
  auto transposed = [&](size_t dst, int rows, int cols, int ld) { t.push_back({rows, 0, 0, false, 1, {{cols, 1, dst, ld, 0}}}); };
  vec(L.emb, K * Fn);
  vec(L.W2, Fn * Fn);
  vec(L.b2, Fn);
  vec(L.W4, Fn * Fn);
  vec(L.b4, Fn);
  vec(L.offsets, Fe, true);  // "_edge_embedding.offset"
  // node blocks (all passes) come first in the state dict, then edge blocks
  for (const auto &q : L.pass) {
    t.push_back({2 * Fn, Fn, FnP, false, 2, {{Fn, 1, q.c1_WnT, 2 * FnP, 0}, {Fe, 1, q.c1_WeT, 2 * FnP, 0}}});  // c1_linear.weight [2Fn, Fn+Fe]
    gated(q.c1_bias, Fn, FnP);
    gated(q.c1n_g, Fn, FnP);
    gated(q.c1n_b, Fn, FnP);
    vec(q.fin_g, Fn);
    vec(q.fin_b, Fn);
  }
  for (const auto &q : L.pass) {
    t.push_back({2 * Fe, Fe, FeP, false, 1, {{Fn, 1, q.c2_WT, 2 * FeP, 0}}});  // c2_linear.weight [2Fe, Fn]
    gated(q.c2_bias, Fe, FeP);
    // c3_linear.weight [2Fe, 3Fn+2Fe]: [n_i | n_j | n_k | e_slot5 | e_slot6]
    t.push_back({2 * Fe, Fe, FeP, false, 2, {{Fn, 3, q.c3_WnT, 6 * FeP, 2 * FeP}, {Fe, 2, q.c3_WeT, 4 * FeP, 2 * FeP}}});
    gated(q.c3_nshift + 2 * FeP, Fe, FeP);  // c3 bias: the middle block of (0 | bias | 0)
    gated(q.c2n1_g, Fe, FeP);
    gated(q.c2n1_b, Fe, FeP);
    gated(q.c3n1_g, Fe, FeP);
    gated(q.c3n1_b, Fe, FeP);
    vec(q.c2n2_g, Fe);
    vec(q.c2n2_b, Fe);
    vec(q.c3n2_g, Fe);
    vec(q.c3n2_b, Fe);
  }
  transposed(L.W0T, Fe, Fe, HP);
  vec(L.b0p, Fe);  // the trained copy of readout bias 0; b0 is derived from it
  vec(L.bn_w, Fe);
  vec(L.bn_b, Fe);
  vec(L.bn_rm, Fe, true);  // running_mean
  vec(L.bn_rv, Fe, true);  // running_var
  transposed(L.W3T, Fe, Fe, HP);
  vec(L.b3, Fe);
  transposed(L.W5T, 12, Fe, 32);
  vec(L.b5, 12);
  return t;
}

size_t elements(const Tensor &t) {
  size_t cols = 0;
  for (int i = 0; i < t.pieces; ++i) cols += (size_t)t.piece[i].width * t.piece[i].blocks;
  return (size_t)t.rows * cols;
}

// The offsets alone (no index map): rn_potgnn_weight_count sums the table over them.
PackedLayout layout_offsets(const rn_potgnn_config &cfg, Dims d) {
  PackedLayout L;
  L.K = cfg.num_atom_types, L.P = cfg.num_message_passes, L.d = d, L.HP = std::max(d.FeP, 32);
  const size_t K = L.K, Fn = d.Fn, Fe = d.Fe, FnP = d.FnP, FeP = d.FeP, HP = L.HP;
  auto take = [&L](size_t n) {
    const size_t o = L.total;
    L.total += (n + 3) & ~size_t(3);  // keep 16-byte alignment for float4 loads
    return o;
  };
  L.emb = take(K * Fn);
  L.W2 = take(Fn * Fn);
  L.b2 = take(Fn);
  L.W4 = take(Fn * Fn);
  L.b4 = take(Fn);
  L.offsets = take(FeP);
  L.pass.resize(L.P);
  for (auto &p : L.pass) {
    p.c1_WnT = take(FnP * 2 * FnP);
    p.c1_WeT = take(FeP * 2 * FnP);
    p.c1_bias = take(2 * FnP);
    p.c1n_g = take(2 * FnP);
    p.c1n_b = take(2 * FnP);
    p.fin_g = take(FnP);
    p.fin_b = take(FnP);
    p.c2_WT = take(FnP * 2 * FeP);
    p.c2_bias = take(2 * FeP);
    p.c2n1_g = take(2 * FeP);
    p.c2n1_b = take(2 * FeP);
    p.c2n2_g = take(FeP);
    p.c2n2_b = take(FeP);
    p.c3_WnT = take(FnP * 6 * FeP);
    p.c3_nshift = take(6 * FeP);
    p.c3_WeT = take(FeP * 4 * FeP);
    p.c3n1_g = take(2 * FeP);
    p.c3n1_b = take(2 * FeP);
    p.c3n2_g = take(FeP);
    p.c3n2_b = take(FeP);
    p.c3n1_gs = take(2 * FeP);
    p.c3n1_bs = take(2 * FeP);
    p.c2n1_gs = take(2 * FeP);
    p.c2n1_bs = take(2 * FeP);
    p.c1n_gs = take(2 * FnP);
    p.c1n_bs = take(2 * FnP);
    p.mfma_scale = take(8);
    p.mfma_scale_c = take(8);  // (right behind mfma_scale: PackedLayout::mfma_scales)
    p.t_c3We = take(4 * FeP * FeP);
    p.t_c3Wn = take(6 * FeP * FnP);
    p.t_c2W = take(2 * FeP * FnP);
    p.t_c1We = take(2 * FnP * FeP);
    p.t_c1Wn = take(2 * FnP * FnP);
    p.c3_WeT_c = take(FeP * 4 * FeP);
    p.c3_WnT_c = take(FnP * 6 * FeP);
    p.c3_nshift_c = take(6 * FeP);
    p.c2_WT_c = take(FnP * 2 * FeP);
    p.c2_bias_c = take(2 * FeP);
    p.c1_WnT_c = take(FnP * 2 * FnP);
    p.c1_WeT_c = take(FeP * 2 * FnP);
    p.c1_bias_c = take(2 * FnP);
  }
  L.W0T = take(FeP * HP);
  L.b0 = take(Fe);
  L.bn_w = take(Fe);
  L.bn_b = take(Fe);
  L.bn_rm = take(Fe);
  L.bn_rv = take(Fe);
  L.W3T = take(HP * HP);
  L.b3 = take(HP);
  L.W5T = take(HP * 32);
  L.b5 = take(32);
  L.ones = take(HP);
  L.b0p = take(HP);  // bias of readout Linear 0, padded (training-mode forward)
  L.t_W0 = take(HP * FeP);
  L.t_W3 = take(HP * HP);
  L.t_W5 = take(32 * HP);
  L.ro_mfma_scale = take(8);
  L.node_table = take(K * FnP);
  L.scale0 = take(HP);
  L.shift0 = take(HP);
  return L;
}

}  // namespace

// (adjacent = the next block starts where this one, padded to four floats as `take` pads it, ends)
Span PackedLayout::c3_norm_1(int p) const {
  const Pass &q = pass[p];
  if (q.c3n1_b != q.c3n1_g + 2 * (size_t)d.FeP) throw std::logic_error("packed weight layout: c3_norm_1 gamma | beta is not contiguous");
  return {q.c3n1_g, 4 * (size_t)d.FeP};
}
Span PackedLayout::mfma_scales(int p) const {
  const Pass &q = pass[p];
  if (q.mfma_scale_c != q.mfma_scale + 8) throw std::logic_error("packed weight layout: mfma_scale | mfma_scale_c is not contiguous");
  return {q.mfma_scale, 16};
}
Span PackedLayout::readout() const {
  const size_t Fe4 = ((size_t)d.Fe + 3) & ~size_t(3), FeP = d.FeP;
  const size_t want[] = {W0T, W0T + FeP * HP, b0 + Fe4, bn_w + Fe4, bn_b + Fe4, bn_rm + Fe4, bn_rv + Fe4, W3T + (size_t)HP * HP, b3 + HP, W5T + (size_t)HP * 32};
  const size_t have[] = {W0T, b0, bn_w, bn_b, bn_rm, bn_rv, W3T, b3, W5T, b5};
  for (int i = 0; i < 10; ++i)
    if (want[i] != have[i]) throw std::logic_error("packed weight layout: W0T .. b5 is not contiguous");
  return {W0T, b5 + 32 - W0T};
}

PackedLayout layout_weights(const rn_potgnn_config &cfg, Dims d) {
  PackedLayout L = layout_offsets(cfg, d);
  if (L.total > UINT32_MAX) throw std::length_error("packed weight layout: more than 2^32 entries");
  for (const Tensor &t : state_dict_tensors(L)) {
    if (t.buffer) L.buffers.push_back({L.index.size(), elements(t)});
    for (int r = 0; r < t.rows; ++r) {
      const size_t row = t.F > 0 ? gated_col(r, t.F, t.FP) : r;
      for (int i = 0; i < t.pieces; ++i) {
        const Piece &p = t.piece[i];
        for (int b = 0; b < p.blocks; ++b)
          for (int k = 0; k < p.width; ++k) L.index.push_back((uint32_t)(p.dst + (size_t)k * p.ld + (size_t)b * p.block_stride + row));
      }
    }
  }
  return L;
}

size_t state_dict_count(const rn_potgnn_config *c) {
  if (!c || c->num_atom_types <= 0 || c->size_node_embedding <= 0 || c->size_edge_embedding <= 0 || c->num_message_passes <= 0) return 0;
  const int Fn = c->size_node_embedding, Fe = c->size_edge_embedding;
  size_t n = 0;
  for (const Tensor &t : state_dict_tensors(layout_offsets(*c, Dims{Fn, Fe, Fn, Fe}))) n += elements(t);  // (the count does not depend on the padding)
  return n;
}

std::vector<DerivedOp> derived_ops(const PackedLayout &L, int *first_stage) {
  const int Fn = L.d.Fn, Fe = L.d.Fe, FnP = L.d.FnP, FeP = L.d.FeP, HP = L.HP;
  const float filter = -1.4426950408889634f, core = 2.0f * 1.4426950408889634f;  // sigmoid(f) tanh(c) through exp2: exp2(-log2e f), exp2(2 log2e c)
  std::vector<DerivedOp> ops;
  auto transpose = [&](size_t src, int K, int N, size_t dst) { ops.push_back({0, K, N, 1.0f, src, dst}); };
  auto scaled = [&](size_t src, int n, float sc, size_t dst) { ops.push_back({1, n, 1, sc, src, dst}); };
  auto folded = [&](size_t g, size_t b, int FP, size_t gs, size_t bs) {  // a [filter | core] LayerNorm times the gate's exp2 scales
    scaled(g, FP, filter, gs);
    scaled(b, FP, filter, bs);
    scaled(g + FP, FP, core, gs + FP);
    scaled(b + FP, FP, core, bs + FP);
  };
  // (s, 1/s) of the [K][N] block at src (leading dimension ld) that enters a split-f16 matrix product
  auto prescale = [&](size_t src, int K, int N, int ld, size_t dst) { ops.push_back({2, K, N, (float)ld, src, dst}); };
  // The centred copies of a matrix / bias vector whose output columns feed a LayerNorm over a [filter | core] row.
  // LayerNorm(x) = LayerNorm(x - mean x), and the row mean of a Linear's output is itself linear in the input, so
  // subtracting from every weight row (and from the bias) its mean over the real output columns makes the projections
  // come out with zero row mean.  The [filter | core] blocks are 2 FP columns wide, the first F of each half real.
  auto centre = [&](size_t src, size_t dst, int K, int N, int F, int FP) { ops.push_back({3, K, N, 1.0f, src, dst, F, FP}); };
  for (const auto &q : L.pass) {
    transpose(q.c3_WeT, FeP, 4 * FeP, q.t_c3We);
    transpose(q.c3_WnT, FnP, 6 * FeP, q.t_c3Wn);
    transpose(q.c2_WT, FnP, 2 * FeP, q.t_c2W);
    transpose(q.c1_WeT, FeP, 2 * FnP, q.t_c1We);
    transpose(q.c1_WnT, FnP, 2 * FnP, q.t_c1Wn);
    folded(q.c3n1_g, q.c3n1_b, FeP, q.c3n1_gs, q.c3n1_bs);
    folded(q.c2n1_g, q.c2n1_b, FeP, q.c2n1_gs, q.c2n1_bs);
    folded(q.c1n_g, q.c1n_b, FnP, q.c1n_gs, q.c1n_bs);
  }
  transpose(L.W0T, FeP, HP, L.t_W0);
  transpose(L.W3T, HP, HP, L.t_W3);
  transpose(L.W5T, HP, 32, L.t_W5);
  scaled(L.b0p, Fe, 1.0f, L.b0);  // the bias of readout Linear 0 lives twice (eval fold / training forward)
  for (const auto &q : L.pass) {
    prescale(q.c1_WeT, FeP, 2 * FnP, 2 * FnP, q.mfma_scale);
    prescale(q.c3_WeT, FeP, 2 * FeP, 4 * FeP, q.mfma_scale + 2);            // W4: destination-edge part
    prescale(q.c3_WeT + 2 * FeP, FeP, 2 * FeP, 4 * FeP, q.mfma_scale + 4);  // W5: source-edge part
    prescale(q.c2_WT, FnP, 2 * FeP, 2 * FeP, q.mfma_scale + 6);
  }
  prescale(L.W0T, FeP, HP, HP, L.ro_mfma_scale);
  prescale(L.W3T, HP, HP, HP, L.ro_mfma_scale + 2);
  prescale(L.W5T, HP, 32, 32, L.ro_mfma_scale + 4);
  for (const auto &q : L.pass) {
    centre(q.c3_WeT, q.c3_WeT_c, FeP, 4 * FeP, Fe, FeP);
    centre(q.c3_WnT, q.c3_WnT_c, FnP, 6 * FeP, Fe, FeP);
    centre(q.c3_nshift, q.c3_nshift_c, 1, 6 * FeP, Fe, FeP);
    centre(q.c2_WT, q.c2_WT_c, FnP, 2 * FeP, Fe, FeP);
    centre(q.c2_bias, q.c2_bias_c, 1, 2 * FeP, Fe, FeP);
    centre(q.c1_WnT, q.c1_WnT_c, FnP, 2 * FnP, Fn, FnP);
    centre(q.c1_WeT, q.c1_WeT_c, FeP, 2 * FnP, Fn, FnP);
    centre(q.c1_bias, q.c1_bias_c, 1, 2 * FnP, Fn, FnP);
  }
  if (first_stage) *first_stage = (int)ops.size();
  // second stage: the prescales of the centred copies read what the first wrote
  for (const auto &q : L.pass) {
    prescale(q.c3_WeT_c, FeP, 2 * FeP, 4 * FeP, q.mfma_scale_c);
    prescale(q.c3_WeT_c + 2 * FeP, FeP, 2 * FeP, 4 * FeP, q.mfma_scale_c + 2);
    prescale(q.c2_WT_c, FnP, 2 * FeP, 2 * FeP, q.mfma_scale_c + 4);
    prescale(q.c1_WeT_c, FeP, 2 * FnP, 2 * FnP, q.mfma_scale_c + 6);
  }
  return ops;
}

void apply_derived(const std::vector<DerivedOp> &ops, float *o) {
  for (const DerivedOp &op : ops) {
    const float *src = o + op.src;
    float *dst = o + op.dst;
    if (op.kind == 0) {  // src [K][N] -> dst [N][K]
      for (int k = 0; k < op.K; ++k)
        for (int n = 0; n < op.N; ++n) dst[(size_t)n * op.K + k] = src[(size_t)k * op.N + n];
    } else if (op.kind == 1) {
      for (int k = 0; k < op.K; ++k) dst[k] = op.scale * src[k];
    } else if (op.kind == 2) {  // power-of-two prescale of a split-f16 product
      const int ld = (int)op.scale;
      float mx = 0.0f;
      for (int k = 0; k < op.K; ++k)
        for (int n = 0; n < op.N; ++n) mx = std::max(mx, std::fabs(src[(size_t)k * ld + n]));
      const float sc = mfma_prescale(mx);
      dst[0] = sc;
      dst[1] = 1.0f / sc;
    } else {  // row-centred copy (float64 means; padded columns stay zero)
      const int F = op.Fe, FP = op.FeP, bw = 2 * FP;
      for (int k = 0; k < op.K; ++k)
        for (int b = 0; b < op.N / bw; ++b) {
          const size_t base = (size_t)k * op.N + (size_t)b * bw;
          double sum = 0;
          for (int hh = 0; hh < 2; ++hh)
            for (int col = 0; col < F; ++col) sum += (double)src[base + hh * FP + col];
          const double mean = sum / (2.0 * F);
          for (int hh = 0; hh < 2; ++hh)
            for (int col = 0; col < FP; ++col)
              dst[base + hh * FP + col] = col < F ? (float)((double)src[base + hh * FP + col] - mean) : 0.0f;
        }
    }
  }
}

void pack_weights(const PackedLayout &L, const float *w, std::vector<float> &o) {
  o.assign(L.total, 0.0f);
  for (size_t i = 0; i < L.index.size(); ++i) o[L.index[i]] = w[i];
  std::fill_n(o.begin() + L.ones, L.HP, 1.0f);
  apply_derived(derived_ops(L), o.data());
}

template <typename T>
void unpack_weights(const PackedLayout &L, const T *packed, T *out, bool buffers) {
  for (size_t i = 0; i < L.index.size(); ++i) out[i] = packed[L.index[i]];
  if (!buffers)
    for (const Span &b : L.buffers) std::fill_n(out + b.begin, b.count, T(0));
}
template void unpack_weights<float>(const PackedLayout &, const float *, float *, bool);
template void unpack_weights<double>(const PackedLayout &, const double *, double *, bool);

std::vector<unsigned char> trainable_mask(const PackedLayout &L) {
  std::vector<unsigned char> mask(L.total, 0);
  for (uint32_t i : L.index) mask[i] = 1;
  for (const Span &b : L.buffers)
    for (size_t i = b.begin; i < b.begin + b.count; ++i) mask[L.index[i]] = 0;
  return mask;
}

std::vector<unsigned char> packed_writers(const PackedLayout &L) {
  std::vector<unsigned char> n(L.total, 0);
  for (uint32_t i : L.index) n[i] += (n[i] & 15) < 15;
  for (const DerivedOp &op : derived_ops(L)) {
    const size_t count = op.kind == 2 ? 2 : (size_t)op.K * ((op.kind == 0 || op.kind == 3) ? op.N : 1);
    for (size_t i = op.dst; i < op.dst + count; ++i) n[i] += n[i] < 240 ? 16 : 0;
  }
  return n;
}

// Weights: always -- each block is prescaled by a power of two into f16's normal range (mfma_prescale),
// so only a non-finite weight refuses.  Activations are split unscaled, which is exact to 22 bits while
// they stay well inside f16's range: edge rows (Gaussian basis, then tanh outputs), updated node rows
// and their products are bounded by 1 by construction; the two hidden layers of the readout MLP
// (shifted softplus, unbounded above) are bounded here from the weights, for |edge| <= 1:
//   |h1_n| <= |scale0_n| sum_k |W0[n][k]| + |shift0_n|,   |h2_n| <= B1 sum_k |W3[n][k]| + |b3_n|.
// Beyond 3e4 (f16 overflows at 65504) the handle falls back to the exact-f32 MFMA instantiations.
bool mfma_f16_range_ok(const PackedLayout &L, const float *o, bool host_stale) {
  const int Fe = L.d.Fe, HP = L.HP;
  // While the device weights are ahead of the host copy (device-resident training) only the readout block, c3_norm_1 and the
  // prescale pairs have been fetched: the finiteness of the weight blocks is then read off the pairs, which the device
  // refresh sets to NaN for a block with a non-finite entry (kernels_train.hip, kind 2)
  int first_stage = 0;
  const std::vector<DerivedOp> ops = derived_ops(L, &first_stage);
  for (size_t i = 0; i < ops.size(); ++i) {
    const DerivedOp &m = ops[i];
    if (m.kind != 2) continue;
    if (!std::isfinite(o[m.dst]) || !std::isfinite(o[m.dst + 1])) return false;
    if (host_stale || (int)i >= first_stage) continue;  // (the centred copies are finite when their sources are)
    const int ld = (int)m.scale;
    for (int k = 0; k < m.K; ++k)
      for (int n = 0; n < m.N; ++n)
        if (!std::isfinite(o[m.src + (size_t)k * ld + n])) return false;
  }
  const double ln2 = 0.6931471805599453;
  double b1 = ln2, b2 = ln2;
  for (int n = 0; n < Fe; ++n) {  // BatchNorm(eval) folded as setup_kernel does
    const double sc = (double)o[L.bn_w + n] / std::sqrt((double)o[L.bn_rv + n] + 1e-5);
    const double sh = ((double)o[L.b0 + n] - (double)o[L.bn_rm + n]) * sc + (double)o[L.bn_b + n];
    double sum = 0;
    for (int k = 0; k < Fe; ++k) sum += std::fabs((double)o[L.W0T + (size_t)k * HP + n]);
    b1 = std::max(b1, std::fabs(sc) * sum + std::fabs(sh));
  }
  for (int n = 0; n < Fe; ++n) {
    double sum = 0;
    for (int k = 0; k < Fe; ++k) sum += std::fabs((double)o[L.W3T + (size_t)k * HP + n]);
    b2 = std::max(b2, sum * b1 + std::fabs((double)o[L.b3 + n]));
  }
  return std::isfinite(b1) && std::isfinite(b2) && b1 <= 3.0e4 && b2 <= 3.0e4;
}

// Needs every gamma of a real column away from zero (the loop divides by it) and the gate arguments provably small:
// a LayerNorm output is at most sqrt(2Fe - 1) in magnitude.
bool folded_gate_ok(const PackedLayout &L, const float *packed, int p) {
  const int Fe = L.d.Fe, FeP = L.d.FeP;
  const float *gam = packed + L.pass[p].c3n1_g, *bet = packed + L.pass[p].c3n1_b;
  const double xmax = std::sqrt(2.0 * Fe) * 1.02;
  for (int half = 0; half < 2; ++half)
    for (int k = 0; k < Fe; ++k) {
      const double g = std::fabs((double)gam[half * FeP + k]), b = std::fabs((double)bet[half * FeP + k]);
      const double arg = (g * xmax + b) * 2.0 * 1.4426950408889634;
      if (!(std::isfinite(g) && std::isfinite(b) && g >= 1e-5 && arg < 60.0)) return false;
    }
  return true;
}

}  // namespace rn
