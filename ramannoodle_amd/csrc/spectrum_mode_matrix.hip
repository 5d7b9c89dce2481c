// On-device mode-by-mode interference matrices of MD Raman bands: the pair spectra between all channels of a set of
// polarizability increments (the phonon modes of PotGNN.calc_mode_increments), summed over weighted bins.  What
// ModeMDRamanSpectrum.measure_interference reduces (include/rn_potgnn.h, rn_md_raman_mode_matrix).
//
// Definition.  Increments incr[t][c][9] (N steps, C channels), weights W[K][21] (forms M_k), a start table of Q segments,
// W frames per segment (n = W - 1 increments), a taper tau[0..n-1] and bin weights bw[B][bins].  With the series and the
// zero-padded transforms X_{q,c,j}(f), f = 0..L-1, of spectrum_modes.hip, the segment-averaged pair spectrum of
// rn_md_raman_partial_segments is the core's back half applied to
//   P_k[m][n](f) = (1/Q) sum_q sum_{j,l} M_k[j][l] Re(X_{q,m,j}(f) conj X_{q,n,l}(f))
// and the back half (inverse transform, positive lags 0..n-1 scaled by 1/L, length-n transform, real part of bins
// 1..bins) is linear in P and the same for every row:
//   I[bin](P) = sum_f T[bin][f] P(f),   T[bin][f] = (1/L) sum_{tau=0}^{n-1} cos(2 pi tau (f/L - (bin+1)/n))
// so that, with u_b[f] = sum_bin bw[b][bin] T[bin][f],
//   out[b][k][m][n] = sum_bin bw[b][bin] I_k[m][n][bin] = sum_{q,f,j} Re(X_{q,m,j}(f) conj Y_{b,k,q,n,j}(f))
//   Y_{b,k,q,n,j}(f) = (u_b[f] / Q) sum_l M_k[j][l] X_{q,n,l}(f)
// The folded half-spectrum is used: the series are real, so P is even in f and the sum runs over f = 0..L/2 with
// u'_b[f] = u_b[f] + u_b[L - f] for 0 < f < L/2 and u'_b[f] = u_b[f] at f = 0 and f = L/2.
// u'_b / Q is computed once per call on the host (rn_md_raman_mode_matrix_response), from the closed form of the sum
// over tau, a Dirichlet kernel whose phases are reduced in integers: with a = f n - (bin+1) L, h = pi a / (L n) and
// H = pi a / L,
//   sum_tau cos(2 tau h) = sin H cos H cos h / sin h + sin^2 H,   and n where a = 0 (mod L n)
// For 0 < f < L/2 the two folded sums share sin H cos H and sin^2 H up to a sign and their cotangents add up to
// sin(2 pi f / L) / (sin^2(pi f / L) - sin^2(pi (bin+1) / n)): one division per (bin, f) from tables over f, except
// where that difference cancels.  Only bins whose weight is not zero are visited.  u' is uploaded with the forms.
//
// Pipeline, per block of Bs segments and Cb channels (x[Bs][Cb][6][L], Cb a multiple of kTile): the builder of
// spectrum_modes.hip (no summed channel here) -> 6 Cb Bs batched forward FFTs of length L -> mode_matrix_kernel.
//
// mode_matrix_kernel: one real product of a C x (Q (L/2+1) 12) operand with its transformed self, on
// v_mfma_f64_16x16x4_f64.  A four-wave workgroup owns a tile of kTile = 64 channels m x 64 channels n of one
// configuration k and one band b (blockIdx.y, blockIdx.z); only tiles with m-tile <= n-tile exist.  It walks the block's
// segments in order and the frequencies in ascending tiles of kFreqs = 4; per frequency the reduction dimension is the
// 12 reals r = 2 j + (re, im), three k-steps.  The transforms are frequency-contiguous per (channel, component), so both
// operands go through LDS, [channel][frequency of the tile][12] with a row stride of kStride = 4 * 12 + 2 = 50 doubles:
// the loads are 16 bytes a lane (one complex value), contiguous along f; an operand read (eight bytes a lane) is served
// in two groups of 32 lanes, sixteen channels x two quads, whose doubles start at banks 2 (50 c + quad) = 36 c + 2 quad
// (mod 64): 18 c (mod 32) takes every even value once over c = 0..15, so a group touches every bank once.  The first
// operand is X_m as it is; the second is formed at staging, Y_n(f) = (u'_b[f] / Q) M_k X_n(f), on VALU by the thread
// that owns (n, f), once per workgroup, the form read from LDS.  A wave holds 16 m x 64 n in four accumulators; result
// register j of lane (l15, quad) of accumulator s is m = 16 wave + 4 j + quad, n = 16 s + l15.  The values of the next
// frequency tile are requested before the products of this one.  Channels past C are zero series (the builder pads a
// block to whole tiles), frequencies past L/2 are zeros in LDS (u' is padded with zeros, the first operand selected);
// loads are unconditional from clamped addresses: nothing is read past an array.  The accumulators are stored to
// acc[b][k][m][n] of the block pair, all 64 x 64 of the tile; the host keeps m <= n and writes the mirror.
//
// Order.  Every element (b, k, m, n) is summed by one lane in one order: segments in table order, frequency tiles
// ascending, frequencies ascending within a tile, k-steps ascending, the instruction's own order within a k-step.  When
// the segments go through in blocks the accumulators continue from the stored partial result (`first` starts them at
// zero), and tiles are aligned to the whole channel range, so the blocking changes nothing: repeated calls and
// different workspace_limits are bit-identical; there are no atomics.  A channel of zeros has X = 0 exactly, hence a
// row and a column that are exactly zero.
// Blocking.  The channels go through in blocks of Cb = whole tiles; with more than one block, the pairs of blocks
// (I <= J) go through two buffers.  A buffer is built and transformed again whenever neither holds the (block, segment
// block) that is wanted: with one segment block a row of pairs (I, I), (I, I+1), ... keeps block I and builds each J
// once, one build and transform per pair; with several segment blocks every pair builds both of its blocks for every
// segment block.  Either way the builds and transforms grow with the square of the number of channel blocks, as the
// pairs do.  Nothing is done about it: a larger workspace_limit is the remedy.
// float64 throughout.  A plan cache of its own, keyed by (device, n, Cb, Bs, buffers).  All work runs on the null stream
// (after a synchronise of the caller's stream in the _device entry).
#include <cmath>
#include <vector>

#include "spectrum_segment_core.hpp"

namespace {
using namespace rn_spectrum;

constexpr int kTile = 64;                        // channels per tile, both ways: 16 m per wave
constexpr int kFreqs = 4;                        // frequencies per tile
constexpr int kReals = 2 * kComponents;          // the reduction dimension of one frequency
constexpr int kStride = kFreqs * kReals + 2;     // LDS row stride in doubles (see the head of this file)
constexpr int kKSteps = kReals / 4;              // k-steps of the 16x16x4 instruction per frequency
constexpr int kMatrixThreads = 256;
constexpr int kLoadsA = kTile * kComponents * kFreqs / kMatrixThreads;  // complex values a thread stages of X_m
constexpr int64_t kMostChannels = (int64_t)1 << 30;
constexpr int64_t kMostGrid = 65535;             // K and B: gridDim.y and gridDim.z
static_assert(kTile * kFreqs == kMatrixThreads, "one thread per (n, f) of the second operand");

typedef double f64x4_t __attribute__((ext_vector_type(4)));

// xm, xn: the transforms of the block pair's channels, [segment][Cb][6][L]; u: [B][fpad], u'_b / Q padded with zeros to
// whole frequency tiles; acc: [B][K][Cb][Cb]
__global__ void __launch_bounds__(kMatrixThreads)
    mode_matrix_kernel(const hipfftDoubleComplex *__restrict__ xm, const hipfftDoubleComplex *__restrict__ xn, int64_t L,
                       int Cb, int count, const double *__restrict__ w, int64_t K, const double *__restrict__ u,
                       int64_t fpad, int square, int first, double *__restrict__ acc) {
  __shared__ __attribute__((aligned(16))) double as[kTile * kStride];  // [m][f][12], row stride 50
  __shared__ __attribute__((aligned(16))) double bs[kTile * kStride];  // [n][f][12]
  __shared__ double ms[kFormSize];
  const int tiles = Cb / kTile;
  int mt, nt;
  if (square) {
    upper_pair((int)blockIdx.x, tiles, mt, nt);
  } else {
    mt = (int)blockIdx.x / tiles;
    nt = (int)blockIdx.x % tiles;
  }
  const int64_t k = blockIdx.y, band = blockIdx.z;
  load_forms(w, k, 1, 1, K, ms);
  const double *ub = u + band * fpad;
  const int64_t half = L / 2 + 1;                          // frequencies 0..L/2
  const int64_t ftiles = fpad / kFreqs;
  const int64_t segment = (int64_t)Cb * kComponents * L;   // complex values of one segment of x
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, quad = lane >> 4;

  // Staging.  First operand: item i = thread + 256 e is (channel i / 24, component (i / 4) % 6, frequency i % 4).
  // Second operand: the thread owns (channel thread / 4, frequency thread % 4) and all six components.
  const int fs = threadIdx.x % kFreqs;
  const hipfftDoubleComplex *src_a[kLoadsA];
  int dst_a[kLoadsA];
#pragma unroll
  for (int e = 0; e < kLoadsA; ++e) {
    const int i = threadIdx.x + kMatrixThreads * e;
    const int ch = i / (kComponents * kFreqs), comp = (i / kFreqs) % kComponents;
    src_a[e] = xm + ((int64_t)(mt * kTile + ch) * kComponents + comp) * L;
    dst_a[e] = ch * kStride + fs * kReals + 2 * comp;
  }
  const int nb = threadIdx.x / kFreqs;
  const hipfftDoubleComplex *src_b = xn + (int64_t)(nt * kTile + nb) * kComponents * L;
  const int dst_b = nb * kStride + fs * kReals;

  hipfftDoubleComplex ra[kLoadsA], rb[kComponents];
  double uf = 0.0;
  bool live = false;
  auto load_tile = [&](int64_t it) {  // tile `it` of the walk over (segment, frequency tile)
    const int64_t b = it / ftiles, f = (it % ftiles) * kFreqs + fs;
    live = f < half;
    const int64_t at = b * segment + (live ? f : 0);
#pragma unroll
    for (int e = 0; e < kLoadsA; ++e) ra[e] = src_a[e][at];
#pragma unroll
    for (int c = 0; c < kComponents; ++c) rb[c] = src_b[at + c * L];
    uf = ub[f];
  };
  const int64_t walk = (int64_t)count * ftiles;
  load_tile(0);

  f64x4_t sum[kTile / 16];
#pragma unroll
  for (int s = 0; s < kTile / 16; ++s) {
    if (first) {
      sum[s] = f64x4_t{0.0, 0.0, 0.0, 0.0};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t m = mt * kTile + wave * 16 + 4 * j + quad, n = nt * kTile + s * 16 + l15;
        sum[s][j] = acc[(((band * K + k) * Cb + m) * Cb) + n];
      }
    }
  }
  __syncthreads();  // the form is in LDS

  for (int64_t it = 0; it < walk; ++it) {
#pragma unroll
    for (int e = 0; e < kLoadsA; ++e)
      *reinterpret_cast<double2 *>(as + dst_a[e]) = live ? make_double2(ra[e].x, ra[e].y) : make_double2(0.0, 0.0);
#pragma unroll
    for (int j = 0; j < kComponents; ++j) {
      double re = 0.0, im = 0.0;
#pragma unroll
      for (int l = 0; l < kComponents; ++l) {
        re = fma(ms[j * kComponents + l], rb[l].x, re);
        im = fma(ms[j * kComponents + l], rb[l].y, im);
      }
      *reinterpret_cast<double2 *>(bs + dst_b + 2 * j) = make_double2(uf * re, uf * im);
    }
    __syncthreads();
    if (it + 1 < walk) load_tile(it + 1);
    // first operand: lane (l15, quad) holds channel 16 wave + l15, real 4 ks + quad; second: channel 16 s + l15
    const double *a = as + (wave * 16 + l15) * kStride + quad, *b = bs + l15 * kStride + quad;
#pragma unroll
    for (int f = 0; f < kFreqs; ++f)
#pragma unroll
      for (int ks = 0; ks < kKSteps; ++ks) {
        const double av = a[f * kReals + 4 * ks];
#pragma unroll
        for (int s = 0; s < kTile / 16; ++s)
          sum[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b[s * 16 * kStride + f * kReals + 4 * ks], sum[s], 0, 0, 0);
      }
    __syncthreads();  // the next tile is written over these
  }

#pragma unroll
  for (int s = 0; s < kTile / 16; ++s)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t m = mt * kTile + wave * 16 + 4 * j + quad, n = nt * kTile + s * 16 + l15;
      acc[(((band * K + k) * Cb + m) * Cb) + n] = sum[s][j];
    }
}

// plans + work buffers of one (device, n, Cb, Bs, buffers)
struct MatrixPlans {
  int device = -1;
  int64_t n = 0, L = 0;
  int Cb = 0, B = 0;  // channels per block (whole tiles), segments per block
  int buffers = 0;    // 1: one block holds every channel; 2: pairs of blocks
  DeviceBuffer x[2], acc, u, source, tau, w, starts;
  size_t fixed_bytes = 0;  // x + the plan's work area
  FftPlan plan_x;
};

PlanCache<MatrixPlans> g_matrix_cache;  // apart from the caches of the other reducers
PhaseTimer g_timer;                     // builder, forward FFTs, product kernel, copies; under g_matrix_cache.mutex

int64_t padded_frequencies(int64_t L) { return (L / 2 + 1 + kFreqs - 1) / kFreqs * kFreqs; }

// sum_{tau=0}^{n-1} cos(2 pi tau a / (L n)), the phases reduced in integers (see the head of this file)
double dirichlet(int64_t a, int64_t n, int64_t L) {
  const double pi = 3.141592653589793238462643383279502884;
  int64_t small = a % (L * n);  // h modulo pi: every term is even in h and has period pi in it
  if (small < 0) small += L * n;
  if (small == 0) return (double)n;
  int64_t big = a % L;          // H modulo pi likewise
  if (big < 0) big += L;
  const double h = pi * ((double)small / ((double)L * (double)n)), H = pi * ((double)big / (double)L);
  const double sH = std::sin(H), cH = std::cos(H);
  return sH * cH * std::cos(h) / std::sin(h) + sH * sH;
}

}  // namespace

// Host only.  bin_weights: [B][bins] -> response: [B][fpad], u'_b[f] * scale for f = 0..L/2 (L = padded_length(n)),
// zeros up to fpad = padded_frequencies(L)
extern "C" int rn_md_raman_mode_matrix_response(int64_t n, const double *bin_weights, int64_t B, int64_t bins,
                                                double scale, double *response) {
  if (!bin_weights || !response || n < 2 || n > (int64_t)1 << 28 || B < 1 || bins != num_bins(n))
    return RN_ERR_INVALID_ARGUMENT;
  const int64_t L = padded_length(n), fpad = padded_frequencies(L), half = L / 2;
  const double pi = 3.141592653589793238462643383279502884;
  std::fill_n(response, (size_t)B * fpad, 0.0);
  // per frequency: sin^2 alpha, sin 2 alpha (alpha = pi f / L) and P = sin H cos H, S = sin^2 H, which depend on the
  // bin by whole turns only (H = pi f n / L - pi (bin + 1))
  std::vector<double> s2a(half + 1), sin2a(half + 1), p(half + 1), s(half + 1);
  for (int64_t f = 0; f <= half; ++f) {
    const double sa = std::sin(pi * ((double)f / (double)L)), sh = std::sin(pi * ((double)(f * n % L) / (double)L));
    s2a[f] = sa * sa;
    sin2a[f] = std::sin(2.0 * pi * ((double)f / (double)L));
    p[f] = 0.5 * std::sin(2.0 * pi * ((double)(f * n % L) / (double)L));
    s[f] = sh * sh;
  }
  for (int64_t b = 0; b < B; ++b)
    for (int64_t bin = 0; bin < bins; ++bin) {
      const double weight = bin_weights[b * bins + bin];
      if (weight == 0.0) continue;
      double *out = response + b * fpad;
      const double sb = std::sin(pi * ((double)(bin + 1) / (double)n)), s2b = sb * sb;
      out[0] += weight * dirichlet(-(bin + 1) * L, n, L);
      out[half] += weight * dirichlet(half * n - (bin + 1) * L, n, L);
      for (int64_t f = 1; f < half; ++f) {
        // T[bin][f] + T[bin][L - f] = (P (cot(alpha - beta) + cot(alpha + beta)) + 2 S) / L with beta = pi (bin + 1) / n,
        // and the two cotangents add up to sin 2 alpha / (sin^2 alpha - sin^2 beta); where that difference cancels
        // (f / L next to (bin + 1) / n) the two sums are taken one by one, their phases reduced in integers
        const double den = s2a[f] - s2b;
        const double t = std::fabs(den) < 1e-3 * s2b
                             ? dirichlet(f * n - (bin + 1) * L, n, L) + dirichlet((L - f) * n - (bin + 1) * L, n, L)
                             : p[f] * sin2a[f] / den + 2.0 * s[f];
        out[f] += weight * t;
      }
    }
  const double factor = scale / (double)L;
  for (int64_t i = 0; i < B * fpad; ++i) response[i] *= factor;
  return RN_OK;
}

namespace {

// d_incr: device float64[N][C][9] -> out: host [B][K][C][C]
int matrix_on_device(MatrixPlans &s, const double *d_incr, int64_t C, int64_t K, int64_t Q, int64_t B, double *out) {
  const int64_t L = s.L, fpad = padded_frequencies(L);
  const int Cb = s.Cb, tiles = Cb / kTile;
  const int64_t blocks = (C + Cb - 1) / Cb;
  std::vector<double> host((size_t)B * K * Cb * Cb);
  int64_t held_block[2] = {-1, -1}, held_q[2] = {-1, -1};
  // the buffer that holds the transforms of channel block `block` of the segments from q0 on, building them in a
  // buffer other than `keep` if none does; -1: a transform failed
  auto transforms = [&](int64_t block, int64_t q0, int count, int keep) -> int {
    for (int i = 0; i < s.buffers; ++i)
      if (held_block[i] == block && held_q[i] == q0) return i;
    const int i = s.buffers == 2 && keep == 0 ? 1 : 0;
    const int64_t c0 = block * Cb;
    const int cc = (int)std::min<int64_t>(Cb, C - c0);
    g_timer.mark(0);
    build_channel_segments_kernel<<<dim3(blocks_of_256(L), (unsigned)s.B, (unsigned)Cb), 256>>>(
        d_incr, s.tau.as<const double>(), s.n, L, C, s.starts.as<const int64_t>(), q0, count, c0, cc, Cb,
        s.x[i].as<hipfftDoubleComplex>());
    g_timer.mark(1);
    held_block[i] = held_q[i] = -1;
    if (!s.plan_x.exec(s.x[i].ptr, HIPFFT_FORWARD)) return -1;
    held_block[i] = block;
    held_q[i] = q0;
    return i;
  };
  for (int64_t bi = 0; bi < blocks; ++bi)
    for (int64_t bj = bi; bj < blocks; ++bj) {
      const int square = bi == bj;
      const unsigned pairs = (unsigned)(square ? tiles * (tiles + 1) / 2 : tiles * tiles);
      for (int64_t q0 = 0; q0 < Q; q0 += s.B) {
        const int count = (int)std::min<int64_t>(s.B, Q - q0);
        const int im = transforms(bi, q0, count, -1);
        const int in = im < 0 || square ? im : transforms(bj, q0, count, im);
        if (im < 0 || in < 0) return RN_ERR_HIP;
        g_timer.mark(2);
        mode_matrix_kernel<<<dim3(pairs, (unsigned)K, (unsigned)B), kMatrixThreads>>>(
            s.x[im].as<hipfftDoubleComplex>(), s.x[in].as<hipfftDoubleComplex>(), L, Cb, count, s.w.as<const double>(),
            K, s.u.as<const double>(), fpad, square, q0 == 0, s.acc.as<double>());
      }
      g_timer.mark(3);
      if (hipGetLastError() != hipSuccess) return RN_ERR_HIP;
      if (hipMemcpy(host.data(), s.acc.ptr, host.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return RN_ERR_HIP;
      g_timer.close();
      const int64_t m0 = bi * Cb, n0 = bj * Cb;
      for (int64_t bk = 0; bk < B * K; ++bk)
        for (int64_t m = m0; m < std::min<int64_t>(C, m0 + Cb); ++m)
          for (int64_t n = std::max<int64_t>(m, n0); n < std::min<int64_t>(C, n0 + Cb); ++n) {
            const double v = host[((size_t)bk * Cb + (m - m0)) * Cb + (n - n0)];
            out[(bk * C + m) * C + n] = v;
            out[(bk * C + n) * C + m] = v;
          }
    }
  return RN_OK;
}

// both entries: increments (float64[N][C][9]) from `src`; starts (host [Q]), taper (host [W-1]), weights (host [K][21]),
// bin_weights (host [B][bins]) -> matrices (host [B][K][C][C])
int md_raman_mode_matrix(Source src, int64_t N, int C, int64_t W, const int64_t *starts, int64_t Q, const double *taper,
                         const double *weights, int64_t K, const double *bin_weights, int64_t B, int device,
                         size_t workspace_limit, double *matrices, int64_t bins) {
  for (const void *q : {(const void *)src.data, (const void *)starts, (const void *)taper, (const void *)weights,
                        (const void *)bin_weights, (const void *)matrices})
    if (!q) return RN_ERR_INVALID_ARGUMENT;
  if (C < 1 || C > kMostChannels || N < 1 || N > (int64_t)1 << 40) return RN_ERR_INVALID_ARGUMENT;
  if (K < 1 || K > kMostGrid || B < 1 || B > kMostGrid) return RN_ERR_INVALID_ARGUMENT;
  int rc = check_table(N + 1, W, starts, Q, 1, bins);  // N increments join N + 1 frames
  if (rc != RN_OK) return rc;
  const int64_t n = W - 1;
  rc = check_call({src.data, taper, weights, matrices}, n, bins, device);
  if (rc != RN_OK) return rc;
  if (bins == 0) {  // no bin to sum over
    std::fill_n(matrices, (size_t)B * K * C * C, 0.0);
    return RN_OK;
  }
  if ((rc = src.wait()) != RN_OK) return rc;
  const int64_t L = padded_length(n), fpad = padded_frequencies(L);
  const int64_t all_tiles = ((int64_t)C + kTile - 1) / kTile;
  const size_t cz = sizeof(hipfftDoubleComplex);
  const size_t limit = workspace_limit ? workspace_limit : kDefaultWorkspace;
  const size_t base = (size_t)n * sizeof(double) + (size_t)K * kPairs * sizeof(double) + (size_t)Q * sizeof(int64_t) +
                      (size_t)B * fpad * sizeof(double);
  if (limit <= base) return RN_ERR_OUT_OF_MEMORY;
  const size_t avail = limit - base;
  const size_t tile_segment = (size_t)kTile * kComponents * L * cz;  // one segment's series of one tile of channels
  auto buffers_of = [&](int64_t tb) { return tb < all_tiles ? 2 : 1; };
  auto acc_bytes = [&](int64_t tb) {  // (saturating: B, K and the channels of a block may each be large)
    const double v = (double)B * (double)K * (double)(tb * kTile) * (double)(tb * kTile) * sizeof(double);
    return v < 9e18 ? (size_t)v : (size_t)9e18;
  };
  auto bytes = [&](int64_t tb, int64_t bs) { return buffers_of(tb) * bs * tb * tile_segment + acc_bytes(tb); };
  // tiles per block: as many as the caps and the limit allow one segment of; then as many segments as fit beside them
  int64_t tb = balanced(all_tiles, std::min<int64_t>({all_tiles, kMaxChannels / kTile,
                                                      std::max<int64_t>(1, (int64_t)(kMaxBlockBytes / tile_segment))}));
  while (tb > 1 && bytes(tb, 1) > avail) tb = balanced(all_tiles, (tb + 1) / 2);
  if (bytes(tb, 1) > avail) return RN_ERR_OUT_OF_MEMORY;
  auto segments_of = [&](int64_t tb) {
    const size_t per_segment = buffers_of(tb) * tb * tile_segment;
    const int64_t cap = std::max<int64_t>(1, (int64_t)(kMaxBlockBytes / (tb * tile_segment)));
    return balanced(Q, std::min<int64_t>({Q, kMaxSegments, cap, (int64_t)((avail - acc_bytes(tb)) / per_segment)}));
  };
  int64_t bs = segments_of(tb);
  std::lock_guard<std::mutex> lock(g_matrix_cache.mutex);
  MatrixPlans *sp = nullptr;
  for (;;) {  // (the plan's work area may not fit beside the blocks: halve the segments, then the channels)
    const int Cb = (int)(tb * kTile), nbuf = buffers_of(tb);
    sp = g_matrix_cache.find([&](const MatrixPlans &e) {
      return e.device == device && e.n == n && e.Cb == Cb && e.B == bs && e.buffers == nbuf;
    });
    if (!sp) {
      MatrixPlans &e = g_matrix_cache.emplace_front();
      e.device = device;
      e.n = n;
      e.L = L;
      e.Cb = Cb;
      e.B = (int)bs;
      e.buffers = nbuf;
      rc = RN_OK;
      for (int i = 0; i < nbuf && rc == RN_OK; ++i) rc = e.x[i].ensure((size_t)bs * tb * tile_segment);
      if (rc == RN_OK && !e.plan_x.make((int)L, (int)(kComponents * Cb * bs))) rc = RN_ERR_HIP;
      if (rc != RN_OK) {
        g_matrix_cache.drop_front();
        return rc;
      }
      e.fixed_bytes = nbuf * bs * tb * tile_segment + e.plan_x.work_bytes();
      sp = &e;
    }
    if (sp->fixed_bytes + acc_bytes(tb) <= avail) break;
    g_matrix_cache.drop_front();
    if (bs > 1) {
      bs = balanced(Q, (bs + 1) / 2);
    } else if (tb > 1) {
      tb = balanced(all_tiles, (tb + 1) / 2);
      if (bytes(tb, 1) > avail) return RN_ERR_OUT_OF_MEMORY;
      bs = segments_of(tb);
    } else {
      return RN_ERR_OUT_OF_MEMORY;
    }
  }
  g_matrix_cache.trim();
  MatrixPlans &s = *sp;
  const double *d_incr = nullptr;
  if ((rc = src.on_device(s.source, (size_t)N * C * 9 * sizeof(double), &d_incr)) != RN_OK) return rc;
  std::vector<double> response((size_t)B * fpad);
  if ((rc = rn_md_raman_mode_matrix_response(n, bin_weights, B, bins, 1.0 / (double)Q, response.data())) != RN_OK)
    return rc;
  if ((rc = upload(s.tau, taper, (size_t)n)) != RN_OK) return rc;
  if ((rc = upload(s.w, weights, (size_t)K * kPairs)) != RN_OK) return rc;
  if ((rc = upload(s.u, response.data(), response.size())) != RN_OK) return rc;
  if ((rc = upload(s.starts, starts, (size_t)Q)) != RN_OK) return rc;
  if ((rc = s.acc.ensure(acc_bytes(tb))) != RN_OK) return rc;
  g_timer.reset();
  rc = matrix_on_device(s, d_incr, C, K, Q, B, matrices);
  g_timer.collect();
  return rc;
}

}  // namespace

extern "C" int rn_md_raman_mode_matrix(const double *increments, int64_t N, int C, int64_t segment_steps,
                                       const int64_t *starts, int64_t Q, const double *taper, const double *weights,
                                       int64_t K, const double *bin_weights, int64_t B, int device,
                                       size_t workspace_limit, double *matrices, int64_t num_bins) {
  return md_raman_mode_matrix(Source::host(increments), N, C, segment_steps, starts, Q, taper, weights, K, bin_weights, B,
                              device, workspace_limit, matrices, num_bins);
}

extern "C" int rn_md_raman_mode_matrix_device(const double *d_increments, int64_t N, int C, int64_t segment_steps,
                                              const int64_t *starts, int64_t Q, const double *taper,
                                              const double *weights, int64_t K, const double *bin_weights, int64_t B,
                                              int device, size_t workspace_limit, double *matrices, int64_t num_bins,
                                              void *stream) {
  return md_raman_mode_matrix(Source::device(d_increments, stream), N, C, segment_steps, starts, Q, taper, weights, K,
                              bin_weights, B, device, workspace_limit, matrices, num_bins);
}

extern "C" int rn_md_raman_mode_matrix_set_profiling(int enabled) {
  return g_timer.set_profiling(g_matrix_cache.mutex, enabled);
}

extern "C" int rn_md_raman_mode_matrix_phase_times(double *millis) {
  return g_timer.phase_times(g_matrix_cache.mutex, millis);
}
