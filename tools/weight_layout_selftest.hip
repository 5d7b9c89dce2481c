// Stand-alone host program for sanitizer runs of csrc/weight_layout.hip (no device is touched):
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         tools/weight_layout_selftest.hip ramannoodle_amd/csrc/weight_layout.hip -o tools/weight_layout_selftest && tools/weight_layout_selftest
// Packs a seeded blob at every shape of tests/helpers.py WEIGHT_SHAPES (and the flag shape), runs the derived-entry
// interpreter, the mask, the writer counts, both host decisions and the three span accessors, unpacks both ways and
// checks the round trip.
#include <cstdio>
#include <random>

#include "../ramannoodle_amd/csrc/weight_layout.hpp"

using namespace rn;

static int pad(int f) {
  int p = 16;
  while (p < f) p *= 2;
  return p;
}

int main() {
  const int shapes[][4] = {{1, 1, 1, 1}, {3, 5, 14, 2}, {2, 16, 16, 1}, {2, 20, 40, 2}, {2, 8, 64, 1}, {3, 64, 64, 4}, {1, 100, 128, 1}, {2, 64, 64, 2}};
  for (const auto &s : shapes) {
    rn_potgnn_config cfg{};
    cfg.num_atoms = 4, cfg.num_edges = 2, cfg.num_atom_types = s[0], cfg.size_node_embedding = s[1], cfg.size_edge_embedding = s[2],
    cfg.num_message_passes = s[3];
    for (int widen = 0; widen < 2; ++widen) {  // minimal padding, and both widths at the wider one
      Dims d{s[1], s[2], pad(s[1]), pad(s[2])};
      if (widen) d.FnP = d.FeP = std::max(d.FnP, d.FeP);
      const PackedLayout L = layout_weights(cfg, d);
      if (L.weight_count() != state_dict_count(&cfg)) return std::printf("count mismatch\n"), 1;
      std::mt19937 rng(7);
      std::normal_distribution<float> normal;
      std::vector<float> w(L.weight_count()), packed, back(L.weight_count());
      for (float &x : w) x = normal(rng);
      pack_weights(L, w.data(), packed);
      unpack_weights<float>(L, packed.data(), back.data(), true);
      if (back != w) return std::printf("round trip failed\n"), 1;
      unpack_weights<float>(L, packed.data(), back.data(), false);
      size_t ones = 0, zeros = 0;
      for (unsigned char m : trainable_mask(L)) ones += m;
      for (size_t i = 0; i < w.size(); ++i) zeros += back[i] != w[i];
      for (unsigned char n : packed_writers(L))
        if ((n & 15) + (n >> 4) > 1) return std::printf("an entry with two writers\n"), 1;
      if (ones + zeros != w.size() || zeros > 3 * (size_t)s[2]) return std::printf("mask / buffers mismatch\n"), 1;
      int folds = 0;
      for (int p = 0; p < L.P; ++p) folds += folded_gate_ok(L, packed.data(), p), (void)L.c3_norm_1(p), (void)L.mfma_scales(p);
      std::printf("K=%d Fn=%d Fe=%d P=%d at %dx%d: %zu -> %zu entries, range ok %d / stale %d, folded passes %d, readout span %zu\n", s[0],
                  s[1], s[2], s[3], d.FnP, d.FeP, w.size(), L.total, (int)mfma_f16_range_ok(L, packed.data(), false),
                  (int)mfma_f16_range_ok(L, packed.data(), true), folds, L.readout().count);
    }
  }
  return 0;
}
