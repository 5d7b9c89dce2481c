// PotGNN evaluation kernels for gfx950: geometry + radial basis, segmented
// (atomic-free) neighbour aggregation for the node and edge blocks, and the readout
// reduction.  Reference semantics: ramannoodle/pmodel/torch/_gnn.py (cited per kernel).
//
// Row layout: every embedding row is padded to a power-of-two width FP >= 16 floats and
// is owned by an aligned "lane group" of FP/4 lanes, 4 consecutive columns per lane
// (16-byte loads/stores, LayerNorm statistics by DPP butterflies inside the group).
// Gated rows are [filter | core] of width 2*FP; a lane holds filter columns 4q..4q+3
// and the matching core columns FP+4q.., so sigmoid(filter)*tanh(core) is lane-local.
#include <algorithm>
#include <cstdlib>

#include "device_utils.hpp"
#include "kernels.hpp"

namespace rn {

#define RN_DISPATCH_LG(FP, PAD, CALL)                                   \
  do {                                                                  \
    switch ((FP) / 4) {                                                 \
      case 4:  if (PAD) { CALL(4, true); }  else { CALL(4, false); }  break;  \
      case 8:  if (PAD) { CALL(8, true); }  else { CALL(8, false); }  break;  \
      case 16: if (PAD) { CALL(16, true); } else { CALL(16, false); } break;  \
      case 32: if (PAD) { CALL(32, true); } else { CALL(32, false); } break;  \
    }                                                                   \
  } while (0)

// ============================================================================ setup
// Frame-independent pieces, computed once per model on the device:
//  * node table [K, FnP]: Embedding -> ssp -> Linear -> ssp -> Linear
//    (_gnn.py:508-514; depends only on the atom type, so K rows instead of S*N)
//  * BatchNorm1d(eval) of the readout folded with the preceding Linear's bias:
//    y = acc*scale + shift  (_gnn.py:533-534)
template <typename T>
__global__ void setup_kernel(const T *emb, const T *W2, const T *b2, const T *W4,
                             const T *b4, int K, Dims d, T *node_table, const T *b0,
                             const T *bn_w, const T *bn_b, const T *bn_rm, const T *bn_rv,
                             T *scale0, T *shift0) {
  extern __shared__ unsigned char smem_raw[];
  T *h = reinterpret_cast<T *>(smem_raw);  // [K*Fn] hidden
  const int Fn = d.Fn;
  for (int i = threadIdx.x; i < K * Fn; i += blockDim.x) {
    int k = i / Fn, o = i % Fn;
    T acc = b2[o];
    for (int c = 0; c < Fn; ++c) acc += ssp(emb[k * Fn + c]) * W2[o * Fn + c];
    h[i] = ssp(acc);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K * d.FnP; i += blockDim.x) {
    int k = i / d.FnP, o = i % d.FnP;
    T acc = 0;
    if (o < Fn) {
      acc = b4[o];
      for (int c = 0; c < Fn; ++c) acc += h[k * Fn + c] * W4[o * Fn + c];
    }
    node_table[i] = acc;
  }
  for (int o = threadIdx.x; o < d.FeP; o += blockDim.x) {
    T sc = 0, sh = 0;
    if (o < d.Fe) {
      T inv = (T)1 / sqrt(bn_rv[o] + (T)1e-5);
      sc = inv * bn_w[o];
      sh = (b0[o] - bn_rm[o]) * sc + bn_b[o];
    }
    scale0[o] = sc;
    shift0[o] = sh;
  }
}

template <typename T>
void launch_setup(const T *emb, const T *W2, const T *b2, const T *W4, const T *b4, int K,
                  Dims d, T *node_table, const T *b0, const T *bn_w, const T *bn_b,
                  const T *bn_rm, const T *bn_rv, T *scale0, T *shift0, hipStream_t st) {
  size_t lds = (size_t)K * d.Fn * sizeof(T);
  setup_kernel<T><<<1, 256, lds, st>>>(emb, W2, b2, W4, b4, K, d, node_table, b0, bn_w, bn_b,
                                       bn_rm, bn_rv, scale0, shift0);
}
template void launch_setup<float>(const float *, const float *, const float *, const float *,
                                  const float *, int, Dims, float *, const float *,
                                  const float *, const float *, const float *, const float *,
                                  float *, float *, hipStream_t);
template void launch_setup<double>(const double *, const double *, const double *,
                                   const double *, const double *, int, Dims, double *,
                                   const double *, const double *, const double *,
                                   const double *, const double *, double *, double *,
                                   hipStream_t);

// ============================================================================ geometry + RBF
// Per edge (a -> b) of every frame: minimum-image displacement
//   d = (x_b - x_a) mod 1;  d -= 1 if d > 0.5          (_gnn.py:603-606)
//   cart = d @ lattice;  dist = |cart|;  unit = cart/|cart|   (_gnn.py:610-611, _utils.py:78-84)
// computed from the edge list only (O(S*E), not the reference's O(S*N^2)), followed by the
// Gaussian radial basis exp(coef*(dist - mu_f)^2) (_gnn.py:81-82) written as padded rows.
// (wrap_min_image: device_utils.hpp, shared with the input-gradient reverse in kernels_bwd.hip)
// PT: the type the positions arrive in.  float32 evaluations cast them to float before any arithmetic (_gnn.py:709), so
// positions that were cast on the host while staging (rn_potgnn_calc_polarizabilities: half the PCIe bytes) give
// bit-identical rows.
template <typename T, typename PT>
__global__ __launch_bounds__(256) void geom_rbf_kernel(const PT *__restrict__ pos, int S,
                                                       Graph g, const T *__restrict__ lat_base,
                                                       int lat_stride,  // 0: one lattice; 9: one per frame
                                                       const T *__restrict__ offs, T coef,
                                                       Dims d, T *__restrict__ unit4,
                                                       T *__restrict__ edge0, int in_order) {
  __shared__ T sdist[256];
  const int64_t total = (int64_t)S * g.E;
  const int64_t r0 = (int64_t)blockIdx.x * 256;
  const int64_t row = r0 + threadIdx.x;
  T dist = 0;
  if (row < total) {
    const int s = (int)(row / g.E);
    // in_order: rows in the (b, a) order of the narrow kernels (kernels_narrow.hip) -- row i of a frame is edge in_edge[i]
    const int e = in_order ? g.in_edge[(int)(row % g.E)] : (int)(row % g.E);
    const int a = g.edge_a[e], b = g.edge_b[e];
    const T *lat = lat_base + (int64_t)s * lat_stride;  // _gnn.py:607-610: the sample's own lattice
    const PT *pa = pos + ((int64_t)s * g.N + a) * 3;
    const PT *pb = pos + ((int64_t)s * g.N + b) * 3;
    T f[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) f[k] = wrap_min_image((T)pb[k] - (T)pa[k]);
    T c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = f[0] * lat[k] + f[1] * lat[3 + k] + f[2] * lat[6 + k];
    dist = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    T *u = unit4 + row * 4;
    u[0] = c[0] / dist;
    u[1] = c[1] / dist;
    u[2] = c[2] / dist;
    u[3] = dist;
  }
  sdist[threadIdx.x] = dist;
  __syncthreads();
  const int c4n = d.FeP / 4;
  for (int i = threadIdx.x; i < 256 * c4n; i += 256) {
    const int r = i / c4n, q = i % c4n;
    if (r0 + r >= total) break;
    const T dd = sdist[r];
    Vec4<T> o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = 4 * q + j;
      T x = dd - offs[col];
      if constexpr (sizeof(T) == 4)  // hardware exp2 (1 ulp), as geom_rbf_pairs_kernel: libm's expf made this write-bound kernel VALU-heavy
        o.v[j] = (col < d.Fe) ? __builtin_amdgcn_exp2f((coef * 1.4426950408889634f) * (x * x)) : 0.0f;
      else
        o.v[j] = (col < d.Fe) ? exp(coef * (x * x)) : (T)0;
    }
    store4(edge0 + (r0 + r) * d.FeP + 4 * q, o);
  }
}

template <typename T>
void launch_geom_rbf(const double *pos, int S, const Graph &g, const T *lattice, int lat_stride,
                     const T *offsets, T coef, Dims d, T *unit4, T *edge0, hipStream_t st, bool in_order) {
  const int64_t total = (int64_t)S * g.E;
  if (total == 0) return;
  geom_rbf_kernel<T, double><<<(unsigned)((total + 255) / 256), 256, 0, st>>>(pos, S, g, lattice, lat_stride,
                                                                              offsets, coef, d, unit4, edge0, in_order ? 1 : 0);
}
void launch_geom_rbf_pos32(const float *pos, int S, const Graph &g, const float *lattice, int lat_stride,
                           const float *offsets, float coef, Dims d, float *unit4, float *edge0, hipStream_t st, bool in_order) {
  const int64_t total = (int64_t)S * g.E;
  if (total == 0) return;
  geom_rbf_kernel<float, float><<<(unsigned)((total + 255) / 256), 256, 0, st>>>(pos, S, g, lattice, lat_stride,
                                                                                 offsets, coef, d, unit4, edge0, in_order ? 1 : 0);
}
// The same with the rows written as split-f16 pairs (kernels.hpp: launch_geom_rbf_pairs), FeP = 64
template <typename PT>
__global__ __launch_bounds__(256) void geom_rbf_pairs_kernel(const PT *__restrict__ pos, int S, Graph g,
                                                             const float *__restrict__ lat_base, int lat_stride,
                                                             const float *__restrict__ offs, float coef, Dims d,
                                                             float *__restrict__ unit4, float *__restrict__ edge0) {
  typedef _Float16 h8 __attribute__((ext_vector_type(8)));
  __shared__ float sdist[256];
  const int64_t total = (int64_t)S * g.E;
  const int64_t r0 = (int64_t)blockIdx.x * 256;
  const int64_t row = r0 + threadIdx.x;
  // This lane's eight Gaussian centres, read once: its column group m is the same in every step of the second phase (read
  // at their use, the compiler left eight dependent loads, each behind a full wait that covers the stores too, in every step)
  const int lane = threadIdx.x & 63, m = lane & 7;
  float mu[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) mu[j] = offs[8 * m + j];
  float dist = 0;
  if (row < total) {
    const int s = (int)(row / g.E), e = (int)(row % g.E);
    const int a = g.edge_a[e], b = g.edge_b[e];
    const float *lat = lat_base + (int64_t)s * lat_stride;
    const PT *pa = pos + ((int64_t)s * g.N + a) * 3;
    const PT *pb = pos + ((int64_t)s * g.N + b) * 3;
    // (all fifteen loads requested before the first wrap: fmod is a loop, and behind it each coordinate's pair of loads
    //  and then the lattice's would wait out a memory latency of their own)
    float xa[3], xb[3], lt[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) xa[k] = (float)pa[k], xb[k] = (float)pb[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) lt[k] = lat[k];
    float f[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) f[k] = wrap_min_image(xb[k] - xa[k]);
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = f[0] * lt[k] + f[1] * lt[3 + k] + f[2] * lt[6 + k];
    dist = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    float *u = unit4 + row * 4;
    u[0] = c[0] / dist;
    u[1] = c[1] / dist;
    u[2] = c[2] / dist;
    u[3] = dist;
  }
  sdist[threadIdx.x] = dist;
  __syncthreads();
  for (int i = threadIdx.x; i < 256 * 8; i += 256) {  // (row, group m of eight columns)
    const int r = i >> 3;
    if (r0 + r >= total) break;
    const float dd = sdist[r];
    h8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = 8 * m + j;
      const float x = dd - mu[j];
      // (hardware exp2: 1 ulp, and the value is rounded to hi + lo = 2^-25 absolute right below anyway)
      const float v = (col < d.Fe) ? __builtin_amdgcn_exp2f((coef * 1.4426950408889634f) * (x * x)) : 0.0f;
      hi[j] = (_Float16)v;
      lo[j] = (_Float16)(v - (float)hi[j]);
    }
    h8 *o = reinterpret_cast<h8 *>(edge0 + (r0 + r) * 64 + 8 * m);
    o[0] = hi;
    o[1] = lo;
  }
}
void launch_geom_rbf_pairs(const double *pos, int S, const Graph &g, const float *lattice, int lat_stride, const float *offsets,
                           float coef, Dims d, float *unit4, float *edge0, hipStream_t st) {
  const int64_t total = (int64_t)S * g.E;
  if (total == 0) return;
  geom_rbf_pairs_kernel<double><<<(unsigned)((total + 255) / 256), 256, 0, st>>>(pos, S, g, lattice, lat_stride, offsets, coef, d,
                                                                                 unit4, edge0);
}
void launch_geom_rbf_pairs_pos32(const float *pos, int S, const Graph &g, const float *lattice, int lat_stride, const float *offsets,
                                 float coef, Dims d, float *unit4, float *edge0, hipStream_t st) {
  const int64_t total = (int64_t)S * g.E;
  if (total == 0) return;
  geom_rbf_pairs_kernel<float><<<(unsigned)((total + 255) / 256), 256, 0, st>>>(pos, S, g, lattice, lat_stride, offsets, coef, d,
                                                                                unit4, edge0);
}
template void launch_geom_rbf<float>(const double *, int, const Graph &, const float *, int,
                                     const float *, float, Dims, float *, float *, hipStream_t, bool);
template void launch_geom_rbf<double>(const double *, int, const Graph &, const double *, int,
                                      const double *, double, Dims, double *, double *,
                                      hipStream_t, bool);

// ============================================================================ node init
template <typename T>
__global__ void node_init_kernel(const T *__restrict__ table, int S, Graph g, Dims d,
                                 T *__restrict__ node, const int *__restrict__ types) {
  const int c4n = d.FnP / 4;
  const int64_t total = (int64_t)S * g.N * c4n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int q = (int)(i % c4n);
    const int64_t rown = i / c4n;
    const int n = (int)(rown % g.N);
    // atom type per (sample, atom) when the caller's atomic_numbers differ between samples
    // (_gnn.py:541-557, 642-643), else the reference structure's
    const int ty = types ? types[rown] : g.atom_type[n];
    store4(node + rown * d.FnP + 4 * q, load4<T>(table + ty * d.FnP + 4 * q));
  }
}
template <typename T>
void launch_node_init(const T *table, int S, const Graph &g, Dims d, T *node, const int *types, hipStream_t st) {
  const int64_t total = (int64_t)S * g.N * (d.FnP / 4);
  if (total == 0) return;
  unsigned blocks = (unsigned)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  node_init_kernel<T><<<blocks, 256, 0, st>>>(table, S, g, d, node, types);
}
template void launch_node_init<float>(const float *, int, const Graph &, Dims, float *, const int *, hipStream_t);
template void launch_node_init<double>(const double *, int, const Graph &, Dims, double *, const int *,
                                       hipStream_t);

// ============================================================================ node block
// NodeBlock (_gnn.py:141-151) with the concatenated Linear factorised:
//   c1_linear(cat[node[b], edge_e]) = (Wn node[b] + bias) + We edge_e = npc1[b] + bc1[e]
// One lane group per destination atom b walks the edges entering b (CSR over b, fixed
// order => deterministic, no atomics): LayerNorm(2Fn) -> sigmoid*tanh -> running sum,
// then LayerNorm(Fn) and tanh(node + .).
template <int LG, bool PAD, typename T>
__global__ __launch_bounds__(256) void node_agg_kernel(const T *__restrict__ npc1,
                                                       const T *__restrict__ bc1,
                                                       const T *__restrict__ node_in,
                                                       T *__restrict__ node_out, int S, Graph g,
                                                       Dims d, PassW<T> w) {
  constexpr int FP = LG * 4;
  const int64_t gid = ((int64_t)blockIdx.x * 256 + threadIdx.x) / LG;
  const int q = threadIdx.x % LG;
  if (gid >= (int64_t)S * g.N) return;
  const int s = (int)(gid / g.N), b = (int)(gid % g.N);
  const int nvalid = min(max(d.Fn - 4 * q, 0), 4);
  const T inv2n = (T)1 / (T)(2 * d.Fn), invn = (T)1 / (T)d.Fn;

  LnParams<T> pf{load4<T>(w.c1_norm.g + 4 * q), load4<T>(w.c1_norm.b + 4 * q)};
  LnParams<T> pc{load4<T>(w.c1_norm.g + FP + 4 * q), load4<T>(w.c1_norm.b + FP + 4 * q)};
  const Vec4<T> af = load4<T>(npc1 + gid * (2 * FP) + 4 * q);
  const Vec4<T> ac = load4<T>(npc1 + gid * (2 * FP) + FP + 4 * q);

  Vec4<T> acc{{0, 0, 0, 0}};
  const int beg = g.in_ptr[b], end = g.in_ptr[b + 1];
  const T *base = bc1 + (int64_t)s * g.E * (2 * FP) + 4 * q;
  for (int idx = beg; idx < end; ++idx) {
    const int e = g.in_edge[idx];
    Vec4<T> xf = load4<T>(base + (int64_t)e * (2 * FP));
    Vec4<T> xc = load4<T>(base + (int64_t)e * (2 * FP) + FP);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xf.v[i] += af.v[i];
      xc.v[i] += ac.v[i];
    }
    Vec4<T> gt = ln_gate<LG, PAD>(xf, xc, pf, pc, inv2n, nvalid);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc.v[i] += gt.v[i];
  }
  LnParams<T> pn{load4<T>(w.final_norm.g + 4 * q), load4<T>(w.final_norm.b + 4 * q)};
  Vec4<T> ln = ln_row<LG, PAD>(acc, pn, invn, nvalid);
  Vec4<T> old = load4<T>(node_in + gid * FP + 4 * q);
  Vec4<T> out;
#pragma unroll
  for (int i = 0; i < 4; ++i) out.v[i] = acc_tanh(old.v[i] + ln.v[i]);
  store4(node_out + gid * FP + 4 * q, out);
}

template <typename T>
void launch_node_agg(const T *npc1, const T *bc1, const T *node_in, T *node_out, int S,
                     const Graph &g, Dims d, const PassW<T> &w, hipStream_t st) {
  const int lg = d.FnP / 4;
  const int64_t threads = (int64_t)S * g.N * lg;
  if (threads == 0) return;
  const unsigned blocks = (unsigned)((threads + 255) / 256);
  const bool pad = d.Fn != d.FnP;
#define CALL(LGV, PADV) \
  node_agg_kernel<LGV, PADV, T><<<blocks, 256, 0, st>>>(npc1, bc1, node_in, node_out, S, g, d, w)
  RN_DISPATCH_LG(d.FnP, pad, CALL);
#undef CALL
}
template void launch_node_agg<float>(const float *, const float *, const float *, float *, int,
                                     const Graph &, Dims, const PassW<float> &, hipStream_t);
template void launch_node_agg<double>(const double *, const double *, const double *, double *,
                                      int, const Graph &, Dims, const PassW<double> &,
                                      hipStream_t);

// ============================================================================ edge block
// EdgeBlock (_gnn.py:223-228 c2, 270-291 c3, 351 residual).  The reference passes PyG's
// triplet tuple positionally (_gnn.py:650), so for a triplet k->j->i the concatenation is
//   [node_i, node_j, node_k, edge_(k->j), edge_(j->i)]   and the scatter target is (k->j).
// With d = (k->j) the destination edge and e = (j->i) a source edge leaving j = b_d:
//   c3_linear(...) = [Wj node[b_d] + Wk node[a_d] + W4 edge_d + bias]  (depends on d)  = P'_d
//                  + [Wi node[b_e] + W5 edge_e]                        (depends on e)  = Q'_e
// Both brackets come from the dense projections (pq, np3); the triplet stage is then
// add -> LayerNorm(2Fe) -> sigmoid*tanh -> sum over e (e in out(b_d), b_e != a_d, ascending
// e == the reference's scatter order): a segmented reduction with implicit triplet indices,
// because the out-edges of an atom are contiguous in the (a, b)-sorted edge list.
//
// Work decomposition: a workgroup owns ONE atom tile for the whole launch and walks the
// frames (the graph is identical in every frame), so the tile's topology is read once
// into LDS and every global load inside the frame loop has a ready address (no dependent
// index->row chains, which cost microseconds each under load).  Per frame the source rows
// Q' of the tile are staged in LDS once -- centred, with |q|^2 -- and reused by every
// destination edge entering the same atom (degree-fold reuse); one lane group per
// destination edge.  LayerNorm statistics use the pre-centred identity
//   x - mean(x) = p + q,  sum (x-mean)^2 = |p|^2 + |q|^2 + 2 p.q   (p, q centred rows)
// so a triplet costs one DPP reduction (p.q) instead of two.
template <typename T>
struct GateScale;
template <>
struct GateScale<float> {
  static constexpr float kF = -1.4426950408889634f;      // exp2(kF * y) = exp(-y)
  static constexpr float kC = 2.0f * 1.4426950408889634f;  // exp2(kC * y) = exp(2y)
  static constexpr float kClamp = 43.28f;                 // |kC * y| <= 15 * kC
};
template <>
struct GateScale<double> {
  static constexpr double kF = -1.4426950408889634;
  static constexpr double kC = 2.0 * 1.4426950408889634;
  static constexpr double kClamp = 115.0;  // tanh == 1 to 1e-34 there; exp2(115) finite
};
#ifndef RN_EXPERIMENT
#define RN_EXPERIMENT 0
#endif
__device__ __forceinline__ float gate_exp2(float yf, float yc) {
  yc = fminf(fmaxf(yc, -GateScale<float>::kClamp), GateScale<float>::kClamp);
#if RN_EXPERIMENT == 1  // timing-only: no transcendental instructions
  const float e1 = yf * 0.5f + 1.0f, e2 = yc * 0.25f + 1.0f;
  return (e2 - 1.0f) * ((1.0f + e1) * (1.0f + e2));
#else
  const float e1 = fast_exp2(yf), e2 = fast_exp2(yc);
  return (e2 - 1.0f) * fast_rcp((1.0f + e1) * (1.0f + e2));
#endif
}
__device__ __forceinline__ double gate_exp2(double yf, double yc) {
  yc = fmin(fmax(yc, -GateScale<double>::kClamp), GateScale<double>::kClamp);
  const double e1 = exp2(yf), e2 = exp2(yc);
  return (e2 - 1.0) / ((1.0 + e1) * (1.0 + e2));
}

// `VPL` = columns per lane and half row (4 or 8).  With 8, a lane group is half as wide, so
// the per-triplet overhead (dot product, DPP reduction, variance, addressing) is
// amortised over twice the gate evaluations per lane; used for Fe >= 64.
template <int VPL, typename T>
__device__ __forceinline__ void loadv(T (&dst)[VPL], const T *p) {
#pragma unroll
  for (int j = 0; j < VPL; j += 4) {
    const Vec4<T> t = load4<T>(p + j);
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[j + k] = t.v[k];
  }
}
template <int VPL, typename T>
__device__ __forceinline__ void storev(T *p, const T (&src)[VPL]) {
#pragma unroll
  for (int j = 0; j < VPL; j += 4) store4(p + j, Vec4<T>{{src[j], src[j + 1], src[j + 2], src[j + 3]}});
}

// LayerNorm over a row of width F held VPL columns per lane by a lane group.
template <int LG, int VPL, bool PAD, typename T>
__device__ __forceinline__ void ln_rowv(T (&x)[VPL], const T *gam, const T *bet, T inv_n, int nvalid) {
  T s = 0;
#pragma unroll
  for (int k = 0; k < VPL; ++k) s += x[k];
  const T mean = lg_sum<LG>(s) * inv_n;
  T qq = 0;
#pragma unroll
  for (int k = 0; k < VPL; ++k) {
    x[k] = (!PAD || k < nvalid) ? x[k] - mean : (T)0;
    qq += x[k] * x[k];
  }
  const T rstd = fast_rsq(lg_sum<LG>(qq) * inv_n + (T)1e-5);
  T g[VPL], b[VPL];
  loadv<VPL>(g, gam);
  loadv<VPL>(b, bet);
#pragma unroll
  for (int k = 0; k < VPL; ++k) x[k] = x[k] * rstd * g[k] + b[k];
}

#ifndef RN_AGG_WAVES
#define RN_AGG_WAVES 3
#endif
// `FASTG` (float32, chosen per pass on the host from the c3_norm_1 parameters): the
// LayerNorm scale is folded into the operands -- LDS holds q*gamma, registers hold p*gamma
// and p/gamma (so p.q is still one fma per column) -- and the overflow clamp of the gate is
// dropped because |gamma| sqrt(2Fe) + |beta| bounds its argument; 5 VALU instructions
// fewer per triplet and column pair.
template <int FP, int VPL, bool PAD, typename T, bool TAPE = false, bool FASTG = false>
__global__ __launch_bounds__(256, (sizeof(T) == 8 ? 1 : (VPL == 8 ? 2 : RN_AGG_WAVES))) void edge_agg_kernel(
    const T *__restrict__ pq, const T *__restrict__ np3, const T *__restrict__ c2pre,
    const T *__restrict__ edge_in, T *__restrict__ edge_out, int S, Graph g, Dims d, PassW<T> w,
    T *__restrict__ agg_out /* training tape: pre-LayerNorm triplet sums [S*E, FP], or null */) {
  constexpr int LG = FP / VPL;   // lanes per row
  constexpr int G = 256 / LG;    // lane groups (= destination edges in flight) per workgroup
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  // LDS carve-up (every region 16-byte aligned)
  const int maxR = g.max_tile_out_rows, maxD = g.max_tile_in_rows, maxN = g.max_tile_nodes;
  size_t off = 0;
  auto carve = [&](size_t bytes) {
    unsigned char *p = smem_raw + off;
    off += (bytes + 15) & ~size_t(15);
    return p;
  };
  constexpr int RS = 2 * FP;
  T *qrows = reinterpret_cast<T *>(carve((size_t)maxR * RS * sizeof(T)));  // centred Q' rows
  T *sq = reinterpret_cast<T *>(carve((size_t)maxR * sizeof(T)));           // |q|^2
  T *nj = reinterpret_cast<T *>(carve((size_t)maxN * 2 * FP * sizeof(T)));      // Wj node[j] + bias
  // per-destination LayerNorm parameters (read once per destination: keep them out of VGPRs)
  T *lnp = reinterpret_cast<T *>(carve((size_t)12 * FP * sizeof(T)));
  T *s_g3 = lnp + 8 * FP, *s_ig3 = lnp + 10 * FP;  // FASTG: scaled gamma of c3_norm_1, 1/gamma
  T *s_c3n2g = lnp, *s_c3n2b = lnp + FP, *s_c2n1g = lnp + 2 * FP, *s_c2n1b = lnp + 4 * FP,
    *s_c2n2g = lnp + 6 * FP, *s_c2n2b = lnp + 7 * FP;
  int *qb = reinterpret_cast<int *>(carve((size_t)maxR * 4));                   // b_e
  int *dl = reinterpret_cast<int *>(carve((size_t)maxD * 6 * 4));               // topology
  int *d_edge = dl, *d_a = dl + maxD, *d_bl = dl + 2 * maxD, *d_rb = dl + 3 * maxD,
      *d_cnt = dl + 4 * maxD, *d_skip = dl + 5 * maxD;
  for (int c = threadIdx.x; c < 2 * FP; c += 256) {
    s_c2n1g[c] = w.c2_norm_1.g[c];
    s_c2n1b[c] = w.c2_norm_1.b[c];
    if (FASTG) {
      const T gam = w.c3_norm_1.g[c] * (c < FP ? GateScale<T>::kF : GateScale<T>::kC);
      s_g3[c] = gam;
      s_ig3[c] = ((c % FP) < d.Fe) ? (T)1 / gam : (T)0;
    }
    if (c < FP) {
      s_c3n2g[c] = w.c3_norm_2.g[c];
      s_c3n2b[c] = w.c3_norm_2.b[c];
      s_c2n2g[c] = w.c2_norm_2.g[c];
      s_c2n2b[c] = w.c2_norm_2.b[c];
    }
  }

  const int tile = blockIdx.x % g.num_tiles;
  const int sg = blockIdx.x / g.num_tiles, nsg = gridDim.x / g.num_tiles;
  const int j0 = g.tile_begin[tile], j1 = g.tile_begin[tile + 1];
  const int eo0 = g.out_ptr[j0], rows = g.out_ptr[j1] - eo0;
  const int di0 = g.in_ptr[j0], dcount = g.in_ptr[j1] - di0;

  // ---- tile topology -> LDS (once per launch)
  for (int r = threadIdx.x; r < rows; r += 256) qb[r] = g.edge_b[eo0 + r];
  for (int i = threadIdx.x; i < dcount; i += 256) {
    const int dst = g.in_edge[di0 + i];
    const int ad = g.edge_a[dst], bd = g.edge_b[dst];
    const int rb = g.out_ptr[bd] - eo0, re = g.out_ptr[bd + 1] - eo0;
    const int rev = g.rev_edge[dst];  // edge (b_d -> a_d): its triplet (i == k) is excluded
    d_edge[i] = dst;
    d_a[i] = ad;
    d_bl[i] = bd - j0;  // tile-local index of the destination atom
    d_rb[i] = rb;
    d_cnt[i] = (re - rb) - (rev >= 0 ? 1 : 0);
    d_skip[i] = rev >= 0 ? rev - eo0 : re;
  }
  __syncthreads();

  const int grp = threadIdx.x / LG, q = threadIdx.x % LG;
  const int c0 = VPL * q;  // first column of this lane in either half
  const int nvalid = min(max(d.Fe - c0, 0), VPL);
  const T inv2n = (T)1 / (T)(2 * d.Fe), invn = (T)1 / (T)d.Fe;
  // c3_norm_1 with the exp2 scale of the gate folded in
  T g3f[VPL], b3f[VPL], g3c[VPL], b3c[VPL];
  loadv<VPL>(g3f, w.c3_norm_1.g + c0);
  loadv<VPL>(b3f, w.c3_norm_1.b + c0);
  loadv<VPL>(g3c, w.c3_norm_1.g + FP + c0);
  loadv<VPL>(b3c, w.c3_norm_1.b + FP + c0);
#pragma unroll
  for (int k = 0; k < VPL; ++k) {
    g3f[k] *= GateScale<T>::kF;
    b3f[k] *= GateScale<T>::kF;
    g3c[k] *= GateScale<T>::kC;
    b3c[k] *= GateScale<T>::kC;
  }

  for (int s = sg; s < S; s += nsg) {
    const int64_t erow0 = (int64_t)s * g.E, nrow0 = (int64_t)s * g.N;
    // ---- per-atom part of P': Wj node[j] + bias for the tile's atoms
    for (int i = threadIdx.x; i < (j1 - j0) * (2 * FP / 4); i += 256) {
      const int n = i / (2 * FP / 4), c = (i % (2 * FP / 4)) * 4;
      store4(nj + (size_t)n * 2 * FP + c, load4<T>(np3 + (nrow0 + j0 + n) * (6 * FP) + 2 * FP + c));
    }
    // ---- stage source rows: Q'_e = W5 edge_e + Wi node[b_e], centred, with |q|^2
    for (int r = grp; r < rows; r += G) {
      const T *qp = pq + (erow0 + eo0 + r) * (4 * FP) + 2 * FP + c0;
      const T *np = np3 + (nrow0 + qb[r]) * (6 * FP) + c0;
      T f[VPL], c[VPL], nf[VPL], nc[VPL];
      loadv<VPL>(f, qp);
      loadv<VPL>(c, qp + FP);
      loadv<VPL>(nf, np);
      loadv<VPL>(nc, np + FP);
      T sum = 0;
#pragma unroll
      for (int k = 0; k < VPL; ++k) {
        f[k] += nf[k];
        c[k] += nc[k];
        sum += f[k] + c[k];
      }
      const T mean = lg_sum<LG>(sum) * inv2n;
      T ss = 0;
#pragma unroll
      for (int k = 0; k < VPL; ++k) {
        f[k] = (!PAD || k < nvalid) ? f[k] - mean : (T)0;
        c[k] = (!PAD || k < nvalid) ? c[k] - mean : (T)0;
        ss += f[k] * f[k] + c[k] * c[k];
      }
      ss = lg_sum<LG>(ss);
      if (FASTG) {
        T sgf[VPL], sgc[VPL];
        loadv<VPL>(sgf, s_g3 + c0);
        loadv<VPL>(sgc, s_g3 + FP + c0);
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
          f[k] *= sgf[k];
          c[k] *= sgc[k];
        }
        ss *= inv2n;
      }
      storev<VPL>(qrows + (size_t)r * RS + c0, f);
      storev<VPL>(qrows + (size_t)r * RS + FP + c0, c);
      if (q == 0) sq[r] = ss;
    }
    __syncthreads();

    // ---- destination edges of the tile; the next destination's rows are fetched while the
    //      current one's triplets are evaluated
    T nxt_pf[VPL], nxt_pc[VPL], nxt_kf[VPL], nxt_kc[VPL];
    auto fetch = [&](int i) {
      const T *pp = pq + (erow0 + d_edge[i]) * (4 * FP) + c0;
      const T *nk = np3 + (nrow0 + d_a[i]) * (6 * FP) + 4 * FP + c0;
      loadv<VPL>(nxt_pf, pp);
      loadv<VPL>(nxt_pc, pp + FP);
      loadv<VPL>(nxt_kf, nk);
      loadv<VPL>(nxt_kc, nk + FP);
    };
    int i = grp;
    if (i < dcount) fetch(i);
    while (i < dcount) {
      // P'_d = W4 edge_d + Wk node[a_d] + (Wj node[b_d] + bias), centred
      T pf[VPL], pc[VPL];
      {
        T jf[VPL], jc[VPL];
        loadv<VPL>(jf, nj + (size_t)d_bl[i] * 2 * FP + c0);
        loadv<VPL>(jc, nj + (size_t)d_bl[i] * 2 * FP + FP + c0);
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
          pf[k] = nxt_pf[k] + nxt_kf[k] + jf[k];
          pc[k] = nxt_pc[k] + nxt_kc[k] + jc[k];
        }
      }
      const int inext = i + G;
#if RN_AGG_WAVES < 4   // (at 4 waves/SIMD there are no registers for the look-ahead)
      if (inext < dcount) fetch(inext);
#endif
      // this destination's c2 pre-activation and old embedding arrive during the triplet loop
      const int64_t drow = erow0 + d_edge[i];
      T c2f[VPL], c2c[VPL], old[VPL];
      loadv<VPL>(c2f, c2pre + drow * (2 * FP) + c0);
      loadv<VPL>(c2c, c2pre + drow * (2 * FP) + FP + c0);
      loadv<VPL>(old, edge_in + drow * FP + c0);

      T sum = 0;
#pragma unroll
      for (int k = 0; k < VPL; ++k) sum += pf[k] + pc[k];
      const T mean = lg_sum<LG>(sum) * inv2n;
      T sp = 0;
#pragma unroll
      for (int k = 0; k < VPL; ++k) {
        pf[k] = (!PAD || k < nvalid) ? pf[k] - mean : (T)0;
        pc[k] = (!PAD || k < nvalid) ? pc[k] - mean : (T)0;
        sp += pf[k] * pf[k] + pc[k] * pc[k];
      }
      sp = lg_sum<LG>(sp);

      const int rb = d_rb[i], cnt = d_cnt[i], rskip = d_skip[i];
      T acc[VPL];
#pragma unroll
      for (int k = 0; k < VPL; ++k) acc[k] = 0;
      if constexpr (FASTG) {
        // pd = p/gamma * (2/2Fe), pg = p*gamma; var + eps = pd.qg + (|p|^2/2Fe + eps) + |q|^2/2Fe
        T pdf[VPL], pdc[VPL];
        {
          T sgf[VPL], sgc[VPL], igf[VPL], igc[VPL];
          loadv<VPL>(sgf, s_g3 + c0);
          loadv<VPL>(sgc, s_g3 + FP + c0);
          loadv<VPL>(igf, s_ig3 + c0);
          loadv<VPL>(igc, s_ig3 + FP + c0);
          const T two_inv = (T)2 * inv2n;
#pragma unroll
          for (int k = 0; k < VPL; ++k) {
            pdf[k] = pf[k] * igf[k] * two_inv;
            pdc[k] = pc[k] * igc[k] * two_inv;
            pf[k] *= sgf[k];
            pc[k] *= sgc[k];
          }
        }
        const T spe = sp * inv2n + (T)1e-5;
        for (int t = 0; t < cnt; ++t) {
          const int r = rb + t + ((rb + t >= rskip) ? 1 : 0);
          const T *qr = qrows + (size_t)r * RS + c0;
          T qf[VPL], qc[VPL];
          loadv<VPL>(qf, qr);
          loadv<VPL>(qc, qr + FP);
          const T sqr = sq[r];
          T dot = 0;
#pragma unroll
          for (int k = 0; k < VPL; ++k) dot += pdf[k] * qf[k] + pdc[k] * qc[k];
          dot = lg_sum<LG>(dot);
          T ve = dot + (spe + sqr);
          ve = ve > (T)1e-5 ? ve : (T)1e-5;
          const T rstd = fast_rsq(ve);
#pragma unroll
          for (int k = 0; k < VPL; ++k) {
            const T e1 = fast_exp2((pf[k] + qf[k]) * rstd + b3f[k]);
            const T e2 = fast_exp2((pc[k] + qc[k]) * rstd + b3c[k]);
            acc[k] += (e2 - (T)1) * fast_rcp(((T)1 + e1) * ((T)1 + e2));
          }
        }
      } else {
      for (int t = 0; t < cnt; ++t) {
        const int r = rb + t + ((rb + t >= rskip) ? 1 : 0);
        const T *qr = qrows + (size_t)r * RS + c0;
        T qf[VPL], qc[VPL];
        loadv<VPL>(qf, qr);
        loadv<VPL>(qc, qr + FP);
        const T sqr = sq[r];
        T dot = 0;
#pragma unroll
        for (int k = 0; k < VPL; ++k) dot += pf[k] * qf[k] + pc[k] * qc[k];
#if RN_EXPERIMENT != 2  // timing-only variant 2: no cross-lane reduction
        dot = lg_sum<LG>(dot);
#endif
        T var = (sp + sqr + (T)2 * dot) * inv2n;
        var = var > (T)0 ? var : (T)0;
        const T rstd = fast_rsq(var + (T)1e-5);
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
          const T yf = ((pf[k] + qf[k]) * rstd) * g3f[k] + b3f[k];
          const T yc = ((pc[k] + qc[k]) * rstd) * g3c[k] + b3c[k];
          acc[k] += gate_exp2(yf, yc);
        }
      }
      }
      if (TAPE) storev<VPL>(agg_out + (erow0 + d_edge[i]) * FP + c0, acc);
      ln_rowv<LG, VPL, PAD>(acc, s_c3n2g + c0, s_c3n2b + c0, invn, nvalid);  // c3 (_gnn.py:291)

      // c2: gate(LayerNorm(c2_linear(node[b]*node[a]))) -> LayerNorm   (_gnn.py:223-228)
      {
        T sm = 0;
#pragma unroll
        for (int k = 0; k < VPL; ++k) sm += c2f[k] + c2c[k];
        const T m2 = lg_sum<LG>(sm) * inv2n;
        T q2 = 0;
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
          c2f[k] = (!PAD || k < nvalid) ? c2f[k] - m2 : (T)0;
          c2c[k] = (!PAD || k < nvalid) ? c2c[k] - m2 : (T)0;
          q2 += c2f[k] * c2f[k] + c2c[k] * c2c[k];
        }
        const T r2 = fast_rsq(lg_sum<LG>(q2) * inv2n + (T)1e-5);
        T gf[VPL], bf[VPL], gc[VPL], bc[VPL];
        loadv<VPL>(gf, s_c2n1g + c0);
        loadv<VPL>(bf, s_c2n1b + c0);
        loadv<VPL>(gc, s_c2n1g + FP + c0);
        loadv<VPL>(bc, s_c2n1b + FP + c0);
#pragma unroll
        for (int k = 0; k < VPL; ++k)
          c2f[k] = gate(c2f[k] * r2 * gf[k] + bf[k], c2c[k] * r2 * gc[k] + bc[k]);
        ln_rowv<LG, VPL, PAD>(c2f, s_c2n2g + c0, s_c2n2b + c0, invn, nvalid);
      }
      T out[VPL];
#pragma unroll
      for (int k = 0; k < VPL; ++k) out[k] = acc_tanh(old[k] + c2f[k] + acc[k]);
      storev<VPL>(edge_out + drow * FP + c0, out);
      i = inext;
#if RN_AGG_WAVES >= 4
      if (i < dcount) fetch(i);
#endif
    }
    __syncthreads();  // qrows / nj are restaged for the next frame
  }
}

static int num_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
      n = prop.multiProcessorCount;
    if (n <= 0) n = 256;
  }
  return n;
}

// Tunables (environment, read once).  Leaving VGPR/LDS room next to the persistent
// aggregation workgroups lets the MFMA-bound projection kernels of the other stream run on
// the same CUs at the same time (matrix pipe + HBM beside the VALU-bound triplet loop).
static int env_int(const char *name, int dflt) {
  const char *e = getenv(name);
  return e ? atoi(e) : dflt;
}
static int agg_wgs_per_cu_cap() {
  static int v = env_int("RN_POTGNN_AGG_WGS_PER_CU", 2);
  return v < 1 ? 1 : v;
}
static int agg_vpl() {
  static int v = env_int("RN_POTGNN_VPL", 4);
  return v;
}

size_t edge_agg_lds_bytes(const Graph &g, Dims d, size_t elem) {
  auto up = [](size_t b) { return (b + 15) & ~size_t(15); };
  return up((size_t)g.max_tile_out_rows * 2 * d.FeP * elem) + up((size_t)g.max_tile_out_rows * elem) +
         up((size_t)g.max_tile_nodes * 2 * d.FeP * elem) + up((size_t)12 * d.FeP * elem) +
         up((size_t)g.max_tile_out_rows * 4) + up((size_t)g.max_tile_in_rows * 6 * 4);
}

template <int FP, int VPL, bool PAD, typename T>
static hipError_t launch_edge_agg_cfg(const T *pq, const T *np3, const T *c2pre, const T *edge_in,
                                T *edge_out, int S, const Graph &g, Dims d, const PassW<T> &w,
                                size_t lds, T *agg_out, hipStream_t st) {
  // Persistent workgroups: one per (tile, frame group).  The grid is sized to exactly the
  // number of workgroups the chip holds at once (a partial second round would leave two
  // thirds of the CUs idle: measured 2.25 instead of 3 waves/SIMD).
  constexpr bool kFloat = sizeof(T) == 4;
  auto kern = agg_out ? &edge_agg_kernel<FP, VPL, PAD, T, true, false>
                      : ((kFloat && (w.c3_fast & 2)) ? &edge_agg_kernel<FP, VPL, PAD, T, false, kFloat>
                                               : &edge_agg_kernel<FP, VPL, PAD, T, false, false>);
  if (lds > kCuLdsBytes) return hipErrorLaunchOutOfResources;  // (validate_create_args refuses such graphs: never in a handle)
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, lds) != hipSuccess || per_cu < 1)
    per_cu = 1;
  per_cu = std::min(per_cu, agg_wgs_per_cu_cap());
  int nsg = per_cu * num_cus() / g.num_tiles;
  nsg = nsg < 1 ? 1 : (nsg > S ? S : nsg);
  (void)hipGetLastError();  // (what was tolerated above -- the occupancy query falls back to 1 -- is not this launch's status)
  kern<<<(unsigned)nsg * (unsigned)g.num_tiles, 256, lds, st>>>(pq, np3, c2pre, edge_in, edge_out, S,
                                                                g, d, w, agg_out);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_edge_agg(const T *pq, const T *np3, const T *c2pre, const T *edge_in, T *edge_out,
                     int S, const Graph &g, Dims d, const PassW<T> &w, T *agg_out, hipStream_t st) {
  if (S == 0 || g.E == 0) return hipSuccess;
  const size_t lds = edge_agg_lds_bytes(g, d, sizeof(T));
  const bool pad = d.Fe != d.FeP;
#define RN_EA(FPV, VPLV)                                                                          \
  do {                                                                                            \
    if (pad) return launch_edge_agg_cfg<FPV, VPLV, true, T>(pq, np3, c2pre, edge_in, edge_out, S, g, d, w, lds, agg_out, st); \
    return launch_edge_agg_cfg<FPV, VPLV, false, T>(pq, np3, c2pre, edge_in, edge_out, S, g, d, w, lds, agg_out, st); \
  } while (0)
  const bool wide = sizeof(T) == 4 && agg_vpl() == 8;  // 8 columns per lane: float32, opt-in
  switch (d.FeP) {
    case 16: RN_EA(16, 4); break;
    case 32: RN_EA(32, 4); break;
    case 64: if (wide) RN_EA(64, 8); else RN_EA(64, 4); break;
    case 128: if (wide) RN_EA(128, 8); else RN_EA(128, 4); break;
  }
#undef RN_EA
  return hipErrorInvalidValue;  // (no instantiation for this width: plan_dims pads to 16 / 32 / 64 / 128)
}
template hipError_t launch_edge_agg<float>(const float *, const float *, const float *, const float *,
                                           float *, int, const Graph &, Dims, const PassW<float> &,
                                           float *, hipStream_t);
template hipError_t launch_edge_agg<double>(const double *, const double *, const double *,
                                            const double *, double *, int, const Graph &, Dims,
                                            const PassW<double> &, double *, hipStream_t);

// ============================================================================ readout
// Edge 6-vectors from the 12-wide readout embedding and the bond direction, closed form of
// R diag(p,q,q) R^-1 = q I + (p - q) u u^T with R e_x = u (_gnn.py:372-415, _utils.py:24-65),
// then the per-frame mean over the E edges (_gnn.py:659-664) and de-standardisation
// alpha = vec6->3x3 * sigma + mu in float64 (_gnn.py:711,719-721).
template <typename T>
__global__ __launch_bounds__(256) void readout_reduce_kernel(const T *__restrict__ pol,
                                                             const T *__restrict__ unit4, int S,
                                                             Graph g,
                                                             const double *__restrict__ mean9,
                                                             const double *__restrict__ std9,
                                                             float *__restrict__ vec6,
                                                             double *__restrict__ alpha,
                                                             double *__restrict__ alpha_raw, int pol_stride) {
  __shared__ T red[4][6];
  __shared__ T fin[6];
  const int s = blockIdx.x;
  T a[6] = {0, 0, 0, 0, 0, 0};
  for (int e = threadIdx.x; e < g.E; e += 256) {
    const int64_t row = (int64_t)s * g.E + e;
    const Vec4<T> u = load4<T>(unit4 + row * 4);
    const Vec4<T> m0 = load4<T>(pol + row * pol_stride);
    const Vec4<T> m1 = load4<T>(pol + row * pol_stride + 4);
    const Vec4<T> m2 = load4<T>(pol + row * pol_stride + 8);
    const T ux = u.v[0], uy = u.v[1], uz = u.v[2];
    a[3] += (m0.v[0] - m0.v[1]) * (ux * uy);                 // xy <- emb 0,1
    a[4] += (m0.v[2] - m0.v[3]) * (ux * uz);                 // xz <- emb 2,3
    a[5] += (m1.v[0] - m1.v[1]) * (uy * uz);                 // yz <- emb 4,5
    a[0] += m1.v[3] + (m1.v[2] - m1.v[3]) * (ux * ux);       // xx <- emb 6,7
    a[1] += m2.v[1] + (m2.v[0] - m2.v[1]) * (uy * uy);       // yy <- emb 8,9
    a[2] += m2.v[3] + (m2.v[2] - m2.v[3]) * (uz * uz);       // zz <- emb 10,11
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    T v = a[k];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) red[wv][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    T v = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    v = v / (T)g.E;
    fin[threadIdx.x] = v;
    if (vec6) vec6[(int64_t)s * 6 + threadIdx.x] = (float)v;
  }
  __syncthreads();
  if (threadIdx.x < 9) {
    const int map[9] = {0, 3, 4, 3, 1, 5, 4, 5, 2};  // dataset/torch/utils.py:30-37
    const double v = (double)fin[map[threadIdx.x]];
    if (alpha) alpha[(int64_t)s * 9 + threadIdx.x] = v * std9[threadIdx.x] + mean9[threadIdx.x];
    if (alpha_raw) alpha_raw[(int64_t)s * 9 + threadIdx.x] = v;
  }
}

template <typename T>
void launch_readout_reduce(const T *pol, const T *unit4, int S, const Graph &g,
                           const double *mean9, const double *std9, float *vec6, double *alpha,
                           double *alpha_raw, hipStream_t st, int pol_stride) {
  if (S == 0) return;
  readout_reduce_kernel<T><<<S, 256, 0, st>>>(pol, unit4, S, g, mean9, std9, vec6, alpha, alpha_raw, pol_stride);
}
template void launch_readout_reduce<float>(const float *, const float *, int, const Graph &,
                                           const double *, const double *, float *, double *,
                                           double *, hipStream_t, int);
template void launch_readout_reduce<double>(const double *, const double *, int, const Graph &,
                                            const double *, const double *, float *, double *,
                                            double *, hipStream_t, int);

// ============================================================================ radius graph
// One-time neighbour search of the reference structure (_utils.py:118-137): all N^2
// minimum-image pair distances in float32 with the reference's operation order,
// adjacency[a*N + b] = (dist <= cutoff && a != b).  The host compacts the flags
// (row-major nonzero == edges sorted by (a, b)).
__global__ void radius_graph_kernel(const double *__restrict__ lattice, const double *__restrict__ pos,
                                    int N, float cutoff, unsigned char *__restrict__ adjacency) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)N * N) return;
  const int a = (int)(idx / N), b = (int)(idx % N);
  float f[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) f[k] = wrap_min_image((float)pos[b * 3 + k] - (float)pos[a * 3 + k]);
  float c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
    c[k] = f[0] * (float)lattice[k] + f[1] * (float)lattice[3 + k] + f[2] * (float)lattice[6 + k];
  const float dist = sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
  adjacency[idx] = (dist <= cutoff && a != b) ? 1 : 0;
}
void launch_radius_graph(const double *lattice, const double *pos, int N, float cutoff,
                         unsigned char *adjacency, hipStream_t st) {
  const int64_t total = (int64_t)N * N;
  if (total == 0) return;
  radius_graph_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(lattice, pos, N, cutoff, adjacency);
}

// ============================================================================ triplet listing
// Emits the triplets in exactly the order edge_agg_kernel consumes them (grouped by
// destination edge, then ascending source edge).  Test/introspection only.
__global__ void enum_triplets_kernel(Graph g, int *idx_i, int *idx_j, int *idx_k, int *slot5,
                                     int *slot6) {
  const int dst = blockIdx.x * blockDim.x + threadIdx.x;
  if (dst >= g.E) return;
  const int ad = g.edge_a[dst], bd = g.edge_b[dst];
  int t = g.trip_off[dst];
  for (int e = g.out_ptr[bd]; e < g.out_ptr[bd + 1]; ++e) {
    if (g.edge_b[e] == ad) continue;
    idx_i[t] = g.edge_b[e];
    idx_j[t] = bd;
    idx_k[t] = ad;
    slot5[t] = dst;
    slot6[t] = e;
    ++t;
  }
}
void launch_enum_triplets(const Graph &g, int *idx_i, int *idx_j, int *idx_k, int *slot5,
                          int *slot6, hipStream_t st) {
  if (g.E == 0) return;
  enum_triplets_kernel<<<(g.E + 255) / 256, 256, 0, st>>>(g, idx_i, idx_j, idx_k, slot5, slot6);
}

}  // namespace rn
