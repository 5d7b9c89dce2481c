// Host-only description of the packed weight blob: where every tensor of a model's state dict lands in the flat array the
// kernels read (transposed, [filter | core] halves padded to the planned widths), which entries are derived from others
// (transposed and centred copies, folded gate constants, split-f16 prescale pairs), and the decisions the host takes from the
// packed values.  Nothing here calls the HIP runtime or needs a device: rn_potgnn_debug_pack_weights /
// rn_potgnn_debug_unpack_weights run it on any machine.  forward.hip uploads the result.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/rn_potgnn.h"
#include "kernels.hpp"

namespace rn {

struct Span {
  size_t begin, count;
};

// Offsets into the packed array (layout_weights).  rn_potgnn_gradient_buffer exposes this layout to callers.
struct PackedLayout {
  int K = 0, P = 0;  // atom types, message passes
  Dims d{};
  int HP = 0;  // readout hidden width as stored: max(FeP, 32), projections emit 32-column tiles
  // setup inputs (unpadded)
  size_t emb, W2, b2, W4, b4, b0, bn_w, bn_b, bn_rm, bn_rv;
  size_t offsets;  // [FeP]
  struct Pass {
    size_t c1_WnT, c1_WeT, c1_bias, c1n_g, c1n_b, fin_g, fin_b;
    size_t c2_WT, c2_bias, c2n1_g, c2n1_b, c2n2_g, c2n2_b;
    size_t c3_WnT, c3_nshift, c3_WeT, c3n1_g, c3n1_b, c3n2_g, c3n2_b;
    size_t c3n1_gs, c3n1_bs;  // c3_norm_1 with the gate's exp2 scale folded in (-log2e | 2 log2e): narrow kernels
    size_t c2n1_gs, c2n1_bs, c1n_gs, c1n_bs;  // the same for c2_norm_1 and c1_norm (narrow kernels)
    size_t mfma_scale;        // [8] split-f16 prescales (s, 1/s): c1_WeT | W4 | W5 | c2_WT (kernels.hpp: mfma_prescale)
    size_t t_c3We, t_c3Wn, t_c2W, t_c1We, t_c1Wn;  // transposed copies [N][K] (reverse pass)
    // copies of c3_linear / c2_linear centred over their real output columns (kernels_edge_ps.hip) and the
    // split-f16 prescales (s, 1/s) of W4 | W5 | c2 | c1_WeT in that form
    size_t c3_WeT_c, c3_WnT_c, c3_nshift_c, c2_WT_c, c2_bias_c, mfma_scale_c;
    size_t c1_WnT_c, c1_WeT_c, c1_bias_c;  // c1_linear centred over its 2 Fn output columns (fused NodeBlock)
  };
  std::vector<Pass> pass;
  size_t W0T, W3T, b3, W5T, b5, ones, b0p, t_W0, t_W3, t_W5;
  size_t ro_mfma_scale;  // [8] split-f16 prescales (s, 1/s): W0T | W3T | W5T
  // device-computed
  size_t node_table, scale0, shift0;
  size_t total = 0;

  // State dict <-> packed: element i of the state-dict-ordered blob lives at packed[index[i]] (one walk over the table of
  // state-dict tensors, weight_layout.hip); `buffers` = the state-dict ranges that are no parameters (Gaussian offsets,
  // BatchNorm running statistics).
  std::vector<uint32_t> index;
  std::vector<Span> buffers;
  size_t weight_count() const { return index.size(); }

  // What rn_potgnn_adam_step fetches in one piece each; every accessor throws std::logic_error if the blocks it spans
  // are not adjacent in this layout.
  Span c3_norm_1(int p) const;    // gamma | beta of pass p's c3_norm_1: 4 FeP
  Span mfma_scales(int p) const;  // mfma_scale | mfma_scale_c of pass p: 16
  Span readout() const;           // W0T | b0 | BatchNorm | W3T | b3 | W5T | b5
};

PackedLayout layout_weights(const rn_potgnn_config &cfg, Dims d);
// Elements of the state dict of a model of this configuration (0 for a null configuration or a non-positive size).
size_t state_dict_count(const rn_potgnn_config *cfg);

// Every packed entry that is a function of other entries and how to recompute it, for the host (apply_derived, after the
// scatter) and for the device (refresh_derived_kernel, after an Adam step).  Ops from *first_stage on read what earlier
// ones wrote (the prescales of the centred copies): the device runs them in a second launch.
std::vector<DerivedOp> derived_ops(const PackedLayout &L, int *first_stage = nullptr);
void apply_derived(const std::vector<DerivedOp> &ops, float *packed);  // in list order; float64 row means for kind 3

// The state-dict-ordered blob `w` into the packed host master copy, derived entries included.
void pack_weights(const PackedLayout &L, const float *w, std::vector<float> &packed);
// The inverse, for packed weights (buffers = true) or a packed gradient (buffers = false: zeros where the state dict holds buffers).
template <typename T>
void unpack_weights(const PackedLayout &L, const T *packed, T *out, bool buffers);
// 1 where a packed entry is a trainable parameter.
std::vector<unsigned char> trainable_mask(const PackedLayout &L);

// Per packed entry, who writes it: low nibble = state-dict elements scattered there, high nibble = derived ops whose
// destination covers it (both saturate at 15).  A sound layout has at most one writer per entry.
std::vector<unsigned char> packed_writers(const PackedLayout &L);

// May the fused kernels run their matrix products as split-f16 MFMAs on these weights?  host_stale: only the spans above
// are current (the device is ahead of the host copy); the finiteness of the weight blocks is then read off the prescale pairs.
bool mfma_f16_range_ok(const PackedLayout &L, const float *packed, bool host_stale);
// May pass p's triplet loop fold c3_norm_1's scale into its operands and drop the gate's overflow clamp?
bool folded_gate_ok(const PackedLayout &L, const float *packed, int p);

// The kernels' views of a packed blob in precision T at `w` (c3_fast is left 0: forward.hip's refresh_pass_flags decides it).
template <typename T>
struct WeightViews {
  std::vector<PassW<T>> pass;
  ReadoutW<T> ro;
  const T *offsets, *node_table, *ones;
};
template <typename T>
WeightViews<T> bind_weights(const PackedLayout &L, const T *w) {
  WeightViews<T> v;
  for (const PackedLayout::Pass &q : L.pass) {
    PassW<T> o{};
    o.c1_WnT = w + q.c1_WnT;
    o.c1_WeT = w + q.c1_WeT;
    o.c1_bias = w + q.c1_bias;
    o.c1_norm = {w + q.c1n_g, w + q.c1n_b};
    o.final_norm = {w + q.fin_g, w + q.fin_b};
    o.c2_WT = w + q.c2_WT;
    o.c2_bias = w + q.c2_bias;
    o.c2_norm_1 = {w + q.c2n1_g, w + q.c2n1_b};
    o.c2_norm_2 = {w + q.c2n2_g, w + q.c2n2_b};
    o.c3_WnT = w + q.c3_WnT;
    o.c3_nshift = w + q.c3_nshift;
    o.c3_WeT = w + q.c3_WeT;
    o.c3_norm_1 = {w + q.c3n1_g, w + q.c3n1_b};
    o.c3_norm_2 = {w + q.c3n2_g, w + q.c3n2_b};
    o.c3_norm_1s = {w + q.c3n1_gs, w + q.c3n1_bs};
    o.c2_norm_1s = {w + q.c2n1_gs, w + q.c2n1_bs};
    o.c1_norm_s = {w + q.c1n_gs, w + q.c1n_bs};
    o.mfma_scale = w + q.mfma_scale;
    o.c3_WeT_c = w + q.c3_WeT_c;
    o.c3_WnT_c = w + q.c3_WnT_c;
    o.c3_nshift_c = w + q.c3_nshift_c;
    o.c2_WT_c = w + q.c2_WT_c;
    o.c2_bias_c = w + q.c2_bias_c;
    o.mfma_scale_c = w + q.mfma_scale_c;
    o.c1_WnT_c = w + q.c1_WnT_c;
    o.c1_WeT_c = w + q.c1_WeT_c;
    o.c1_bias_c = w + q.c1_bias_c;
    v.pass.push_back(o);
  }
  v.ro = {w + L.W0T, w + L.scale0, w + L.shift0, w + L.W3T, w + L.b3, w + L.W5T, w + L.b5, w + L.ro_mfma_scale};
  v.offsets = w + L.offsets;
  v.node_table = w + L.node_table;
  v.ones = w + L.ones;
  return v;
}

}  // namespace rn
