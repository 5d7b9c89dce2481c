// The EdgeBlock's c2 branch, once per ATOM PAIR (gfx950, float32 model, Fn and Fe padded to FP = 64, split-f16 MFMA).
//
//   c2 = LN_{Fe}(gate(LN_{2Fe}(c2_linear(node[b] * node[a]))))        (_EdgeBlock.forward, _gnn.py:223-228)
//
// depends on the unordered pair {a, b} only: the product commutes bit for bit, and every edge of a radius graph has its
// reverse, so edge d and rev_edge[d] get the identical row.  edge_block_ps_kernel computed it for both, in its most
// expensive place (a third of the producers' destination-side MFMAs, two LDS-DMA requests and a split per step, and the
// consumers' per-destination prologue).  Here it is a plain streaming kernel over S frames x NP pairs (Graph::pair_a /
// pair_b) that writes [S, NP, FP] float32 -- what the consumers call `c2v` -- and the EdgeBlock's `C2G` instantiation
// reads one 256-byte row per destination instead.
//
// Same arithmetic as the EdgeBlock's: the centred c2_linear (PassW::c2_WT_c / c2_bias_c: zero row mean, so LayerNorm(2Fe)
// needs the sum of squares only), weights and bias in the power-of-two prescale mfma_scale_c[4] (eps scaled with it), the
// operand split into f16 halves, three products per term with f32 accumulation seeded with the bias.  Padded columns are
// exact zeros on the way in and out, so widths below 64 work.
//
// A wave owns a 16-row tile and ALL 128 pre-activation columns (128 VGPRs of weight fragments): lane (l15, quad) multiplies
// k = 16 quad .. + 15 of row l15 and ends with columns 16 t + 4 quad .. + 3 of every 16-column tile t, i.e. column c of the
// filter half and column c of the core half in the same lane, so the gate needs no exchange; the two LayerNorm sums cross
// the row's four lanes.  A row never meets another row's data: a frame evaluated alone is bit-identical to the same frame
// in a batch.  No LDS-DMA, no spin waits, no hand-counted waits.
#include "fused_common.hpp"

namespace rn {

struct C2PairArgs {
  const float *node;  // updated node embedding [S*N, FP]
  float *out;         // [S*NP, FP]
  int64_t M;          // S * NP rows
  int N, NP;
  const int *pair_a, *pair_b;
  Dims d;
  PassW<float> w;
};

namespace {
constexpr int C2P_THREADS = 256;
}

__global__ __launch_bounds__(C2P_THREADS, 2) void c2_pairs_kernel(C2PairArgs a) {
  // per-column tables: the prescaled centred bias, c2_norm_1 (2 FP), c2_norm_2 (FP)
  __shared__ __attribute__((aligned(16))) float s_bias[2 * FP], s_g1[2 * FP], s_b1[2 * FP], s_g2[FP], s_b2[FP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, quad = lane >> 4;
  const float sc2 = a.w.mfma_scale_c[4];
  for (int c = tid; c < 2 * FP; c += C2P_THREADS) {
    s_bias[c] = a.w.c2_bias_c[c] * sc2;
    s_g1[c] = a.w.c2_norm_1.g[c];
    s_b1[c] = a.w.c2_norm_1.b[c];
    if (c < FP) {
      s_g2[c] = a.w.c2_norm_2.g[c];
      s_b2[c] = a.w.c2_norm_2.b[c];
    }
  }
  WaveB<true> bW[4];  // columns 32 p .. 32 p + 31: p = 0, 1 the filter half, 2, 3 the core half
#pragma unroll
  for (int p = 0; p < 4; ++p) bW[p].load(a.w.c2_WT_c, 2 * FP, 32 * p, l15, quad, sc2);
  __syncthreads();

  const float inv2n = 1.0f / (float)(2 * a.d.Fe), invn = 1.0f / (float)a.d.Fe;
  const float eps_c2 = 1e-5f * sc2 * sc2;  // the pre-activation carries the weights' prescale
  const int64_t ntiles = (a.M + 15) / 16, stride = (int64_t)gridDim.x * (C2P_THREADS / 64);

  // this lane's sixteen k of its row's two node rows
  f32x4 xb[4], xa[4];
  auto fetch = [&](int64_t tile) {
    int64_t row = tile * 16 + l15;  // (a tile beyond the last row: a valid row again, never stored)
    if (row >= a.M) row = a.M - 1;
    const int64_t s = row / a.NP;
    const int p = (int)(row - s * a.NP);
    const float *nb = a.node + (s * a.N + a.pair_b[p]) * FP + 16 * quad, *na = a.node + (s * a.N + a.pair_a[p]) * FP + 16 * quad;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      xb[j] = *reinterpret_cast<const f32x4 *>(nb + 4 * j);
      xa[j] = *reinterpret_cast<const f32x4 *>(na + 4 * j);
    }
  };
  int64_t tile = (int64_t)blockIdx.x * (C2P_THREADS / 64) + wave;
  if (tile < ntiles) fetch(tile);
  for (; tile < ntiles; tile += stride) {
    float af[KS];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 pr = xb[j] * xa[j];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[4 * j + i] = pr[i];
    }
    f16x8 ah[2], al[2];
    split_f16x8(af, ah[0], al[0]);
    split_f16x8(af + 8, ah[1], al[1]);
    if (tile + stride < ntiles) fetch(tile + stride);  // the next tile's rows, in flight under this tile's arithmetic

    // (the per-column tables are read per tile: hoisted out of the loop they would take 128 registers next to the weights')
    const int lq = launder(lane >> 4);  // = quad, opaque to the compiler
    // pre-activation: acc[p][t][i] = column 32 p + 16 t + 4 quad + i of row l15
    f32x4 acc[4][2];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[p][t] = *reinterpret_cast<const f32x4 *>(s_bias + 32 * p + 16 * t + 4 * lq);
      bW[p].product_split(ah, al, acc[p]);
    }
    // LayerNorm(2Fe) of a zero-mean row with exact zeros in its padded columns: the plain sum of squares
    float q = 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) q = fmaf(acc[p][t][i], acc[p][t][i], q);
    q = sum_xor32(sum_xor16(q));  // the row's four lanes l15 + 16 quad
    const float rstd2 = fast_rsq(q * inv2n + eps_c2);
    // gate, then LayerNorm(Fe) over the row's 64 columns (16 in this lane)
    float gv[2][2][4], sum = 0.f;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int c = 32 * p + 16 * t + 4 * lq;
        const Vec4<float> gf = load4<float>(s_g1 + c), bf = load4<float>(s_b1 + c);
        const Vec4<float> gc = load4<float>(s_g1 + FP + c), bc = load4<float>(s_b1 + FP + c);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          gv[p][t][i] = gate(acc[p][t][i] * rstd2 * gf.v[i] + bf.v[i], acc[p + 2][t][i] * rstd2 * gc.v[i] + bc.v[i]);
          sum += gv[p][t][i];
        }
      }
    const float mean = sum_xor32(sum_xor16(sum)) * invn;
    float qq = 0.f;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int c = 32 * p + 16 * t + 4 * lq + i;
          gv[p][t][i] = c < a.d.Fe ? gv[p][t][i] - mean : 0.f;
          qq = fmaf(gv[p][t][i], gv[p][t][i], qq);
        }
    const float rstd = fast_rsq(sum_xor32(sum_xor16(qq)) * invn + 1e-5f);
    // A row beyond the last was fetched as the last row again and is stored as such, the same bits to the same place: behind
    // a conditional store the wait for the next tile's rows, requested before these stores, has to wait for the stores too
    const int64_t row = tile * 16 + l15 < a.M ? tile * 16 + l15 : a.M - 1;
    {
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int c = 32 * p + 16 * t + 4 * lq;
          const Vec4<float> g2 = load4<float>(s_g2 + c), b2 = load4<float>(s_b2 + c);
          f32x4 y;
#pragma unroll
          for (int i = 0; i < 4; ++i) y[i] = gv[p][t][i] * rstd * g2.v[i] + b2.v[i];
          *reinterpret_cast<f32x4 *>(a.out + row * FP + c) = y;
        }
    }
  }
}

void launch_c2_pairs(const float *node, float *out, int S, const Graph &g, Dims d, const PassW<float> &w, hipStream_t st) {
  const int64_t M = (int64_t)S * g.NP;
  if (M == 0) return;
  C2PairArgs a{node, out, M, g.N, g.NP, g.pair_a, g.pair_b, d, w};
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
    if (cus <= 0) cus = 256;
  }
  const int64_t ntiles = (M + 15) / 16, per_wg = C2P_THREADS / 64;
  const int64_t grid = std::min<int64_t>((ntiles + per_wg - 1) / per_wg, (int64_t)2 * cus);
  c2_pairs_kernel<<<(unsigned)grid, C2P_THREADS, 0, st>>>(a);
}

}  // namespace rn
