// On-device replicate spectra of the segment-averaged (Welch) MD Raman spectrum: R linear combinations of the Q
// segments' spectra (bootstrap draws, delete-one-block jackknife means, block means), from which the front end takes
// standard errors and confidence bands.  What measure_segment_replicates of ramannoodle_amd/replicates.py reduces before
// the laser / Bose-Einstein corrections (include/rn_potgnn.h, rn_md_raman_segment_replicates).
//
// Definition.  With the transforms X_{q,j}(f), f = 0..L-1, of rn_md_raman_segments_at (segment q of the start table, the
// six tapered difference components, zero-padded to L), the packed weights w_k[21] of configuration k and the
// replicate weights V[R][Q],
//   rep[r][k][bin] = backhalf_bin( pbar[r][k] ),   pbar[r][k](f) = sum_q V[r][q] P_qk(f),
//   P_qk(f) = sum_{p<21} w_k[p] CV_p[q](f),        CV_p[q](f) = Re(X_{q,j(p)}(f) conj X_{q,l(p)}(f))
// The back half (inverse transform, positive lags scaled by 1/L, length-n transform, real bins) is linear, so the
// combination is formed before it, as average = 1 forms the mean: 6 Q forward transforms and 2 R K more, and no
// per-segment row ever exists.  With V[r][q] = 1/Q a row is rn_md_raman_segments_at's mean up to the order of the sums.
//
// Pipeline, per block of B segments: build_segments_at_kernel (the core's) -> 6 B batched forward FFTs of length L into
// x[B][6][L] -> replicate_power_kernel, which accumulates into pbar; after the last block the core's back half
// (segment_rows_to_host) over the block's rows.
//
// replicate_power_kernel: the sum over q is the float64 matrix product V[R x Q] . CV[Q x (21 L)] on
// v_mfma_f64_16x16x4_f64, whose right operand is generated in registers and never exists in memory.  A wave owns 16
// frequencies (f0 + l15) and one tile of 16 replicates; the reduction dimension is the segment index, four per k-step.
// Lane (l15, quad) of the wave:
//   first operand   V[tile's replicate l15][segment 4 ks + quad], one double, read from the transposed, zero-padded
//                   copy vt[Qpad][Rpad] (sixteen lanes read 128 contiguous bytes; no LDS: each value is used once);
//                   zero for a segment past the block's count
//   second operand  the lane loads the six complex values of x at (segment 4 ks + quad, frequency f0 + l15), 16 lanes
//                   contiguous along f, and forms the 21 pair powers: the same lane feeds them to the 21 products
//   accumulators    one per pair: result register j of lane (l15, quad) is replicate 4 j + quad, frequency f0 + l15
//                   (the f64 instruction's own map).  21 x 8 registers.  Two tiles per wave (42 accumulators) were
//                   tried: the compiler then spills (profiles/replicate_spectra.txt), so a wave keeps one.
// The values of the next k-step are requested before the products of this one.  The epilogue contracts the 21
// accumulators with each configuration's weights (scalar loads: k is uniform), in pair order as contract() does, and
// writes pbar[(replicate, k)][f], 16 lanes to 256 contiguous bytes of a row.  Tails: segments past the block's count
// enter with a zero first operand, replicates past R and frequencies past L are computed from clamped addresses and
// not stored; nothing is read past an array.
//
// Order.  Every (r, k, f) is summed by one lane: segments in table order, four per k-step in the instruction's own
// order, then the 21 pairs ascending; no atomics, so repeated calls with the same arguments are bit-identical.  When the
// segments go through in several blocks (always multiples of four, so the k-steps hold the same segments whatever the
// block size), each block's contracted sum is added to the stored partial result (`first` starts it at zero).  The
// contraction over the pairs is then taken per block and not once over all segments, so a workspace_limit that changes the
// number of segment blocks changes the rounding: such runs agree to rounding error (1e-10 of the maximum in the tests),
// not bit for bit.  Blocks of replicates and of configurations change nothing: those are independent outputs.
//
// Blocking.  x holds B segments (all Q, or a multiple of four); the rows of pbar are (replicate, configuration) of a
// block of Rb replicates (all R, or a multiple of 16) and all K configurations, or, when 16 K rows do not fit, of one
// tile of 16 replicates and Kb configurations.  With more than one block of rows and of segments, the segments are
// transformed again for every block of rows, as in run_segments.  float64 throughout.  A plan cache of its own, keyed
// by (device, n, segments per block, rows per block).  All work runs on the null stream (after a synchronise of the
// caller's stream in the _device entry).
#include <cmath>
#include <vector>

#include "spectrum_segment_core.hpp"

namespace {
using namespace rn_spectrum;

constexpr int kReplicateThreads = 256;                        // four waves
constexpr int kTile = 16;                                     // replicates per tile, frequencies per wave
constexpr int kWaves = kReplicateThreads / 64;
constexpr int kStep = 4;                                      // segments per k-step
constexpr int64_t kMaxReplicates = (int64_t)1 << 31;

typedef double f64x4_t __attribute__((ext_vector_type(4)));

// x: [B][6][L], the transforms of the block's segments (`count` of them real, the rest zero series); vt: [Qpad][Rpad],
// V transposed and zero-padded to multiples of 4 and 16; the block's segments are q0 .. q0+count-1 of the table, its
// replicates r0 .. r0+rc-1, its configurations k0 .. k0+kc-1; pbar: slot (r - r0) * kc + (k - k0), each a row of L
__global__ void __launch_bounds__(kReplicateThreads)
    replicate_power_kernel(const hipfftDoubleComplex *__restrict__ x, int64_t L, int B, int count,
                           const double *__restrict__ vt, int64_t Rpad, int64_t q0, int64_t r0, int rc,
                           const double *__restrict__ w, int64_t k0, int kc, int first,
                           hipfftDoubleComplex *__restrict__ pbar) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, quad = lane >> 4;
  const int64_t f = ((int64_t)blockIdx.x * kWaves + wave) * kTile + l15;
  const int64_t fc = std::min<int64_t>(f, L - 1);
  const int rt = (int)blockIdx.y * kTile;  // the wave's first replicate within the block
  const double *va = vt + std::min<int64_t>(r0 + rt + l15, Rpad - 1);

  hipfftDoubleComplex cur[kComponents], nxt[kComponents];
  double a, an;
  auto load_step = [&](int ks, hipfftDoubleComplex *v, double &av) {
    const int seg = kStep * ks + quad;
    const hipfftDoubleComplex *xs = x + (int64_t)std::min(seg, B - 1) * kComponents * L + fc;
#pragma unroll
    for (int c = 0; c < kComponents; ++c) v[c] = xs[c * L];
    const double value = va[(q0 + seg) * Rpad];  // (q0 + seg < Qpad: q0 and Qpad are multiples of four)
    av = seg < count ? value : 0.0;
  };

  f64x4_t acc[kPairs];
#pragma unroll
  for (int p = 0; p < kPairs; ++p) acc[p] = f64x4_t{0.0, 0.0, 0.0, 0.0};

  const int steps = (count + kStep - 1) / kStep;
  load_step(0, cur, a);
  for (int ks = 0; ks < steps; ++ks) {
    const int ahead = std::min(ks + 1, steps - 1);  // (the last step loads itself again: no branch around the loads)
    load_step(ahead, nxt, an);
    double cv[kPairs];
    int p = 0;
#pragma unroll
    for (int j = 0; j < kComponents; ++j)
#pragma unroll
      for (int l = j; l < kComponents; ++l) cv[p++] = cur[j].x * cur[l].x + cur[j].y * cur[l].y;
#pragma unroll
    for (int q = 0; q < kPairs; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, cv[q], acc[q], 0, 0, 0);
#pragma unroll
    for (int c = 0; c < kComponents; ++c) cur[c] = nxt[c];
    a = an;
  }

  if (f >= L) return;
  for (int kl = 0; kl < kc; ++kl) {
    const double *wk = w + (k0 + kl) * kPairs;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int rl = rt + 4 * j + quad;
      if (rl >= rc) continue;
      double v = 0.0;
#pragma unroll
      for (int p = 0; p < kPairs; ++p) v = fma(wk[p], acc[p][j], v);
      hipfftDoubleComplex *out = pbar + ((int64_t)rl * kc + kl) * L + f;
      if (!first) v += out->x;
      *out = make_double2(v, 0.0);
    }
  }
}

// plans + work buffers of one (device, n, B, rows per block), and the replicate weights of the call
struct ReplicatePlans : SegmentPlans {
  DeviceBuffer vt;
};

PlanCache<ReplicatePlans> g_replicate_cache;  // apart from the caches of the other reducers
PhaseTimer g_timer;                           // builder, forward FFTs, product kernel, back half; under the cache's mutex

int64_t round_up(int64_t v, int64_t to) { return (v + to - 1) / to * to; }

// both entries: alpha (float64[S][3][3]) from `src`; starts (host [Q]), taper (host [W-1]), weights (host [K][21]),
// replicate_weights (host [R][Q]) -> intensities (host [R][K][bins])
int md_raman_segment_replicates(Source src, int64_t S, int64_t W, const int64_t *starts, int64_t Q, const double *taper,
                                const double *weights, int64_t K, const double *replicate_weights, int64_t R, int device,
                                size_t workspace_limit, double *intensities, int64_t bins) {
  for (const void *q : {(const void *)src.data, (const void *)starts, (const void *)taper, (const void *)weights,
                        (const void *)replicate_weights, (const void *)intensities})
    if (!q) return RN_ERR_INVALID_ARGUMENT;
  if (K < 1 || K > ((int64_t)1 << 40) || R < 1 || R > kMaxReplicates) return RN_ERR_INVALID_ARGUMENT;
  int rc = check_table(S, W, starts, Q, 1, bins);
  if (rc != RN_OK) return rc;
  for (int64_t i = 0; i < R * Q; ++i)
    if (!std::isfinite(replicate_weights[i])) return RN_ERR_INVALID_ARGUMENT;
  const int64_t n = W - 1;
  rc = check_call({src.data, taper, weights, intensities}, n, bins, device);
  if (rc != RN_OK || bins == 0) return rc;
  if ((rc = src.wait()) != RN_OK) return rc;

  const int64_t L = padded_length(n), Rpad = round_up(R, kTile), Qpad = round_up(Q, kStep);
  const size_t cz = sizeof(hipfftDoubleComplex);
  const size_t limit = workspace_limit ? workspace_limit : kDefaultWorkspace;
  const size_t base = (size_t)n * sizeof(double) + (size_t)K * kPairs * sizeof(double) + (size_t)Q * sizeof(int64_t) +
                      (size_t)Rpad * Qpad * sizeof(double);
  // B segments per block (all Q, or a multiple of four) and the rows of a block, Rb replicates x Kb configurations
  // (all R or a multiple of 16, and all K; or one tile of replicates and some of the K): half of `avail` each, the
  // rest to whichever can still use it.  The least is four segments (or all Q) and one row of each replicate of a tile.
  const int64_t tile = std::min<int64_t>(R, kTile);
  int64_t Rb = 0, Kb = 0;
  auto choose = [&](size_t avail, int *series, int *B, int *rows) {
    *series = kComponents;
    const size_t per_segment = (size_t)kComponents * L * cz, per_row = (size_t)L * cz + (size_t)bins * sizeof(double);
    const int64_t bmin = std::min<int64_t>(Q, kStep);
    const int64_t bcap = std::min<int64_t>({Q, kMaxSegments, (int64_t)(kMaxBlockBytes / per_segment)});
    const double all_rows = (double)R * (double)K;
    const int64_t rcap = std::min<int64_t>({kMaxRows, (int64_t)(kMaxBlockBytes / ((size_t)L * cz)),
                                            all_rows < (double)kMaxRows ? R * K : kMaxRows});
    if (bcap < bmin || rcap < tile || avail < bmin * per_segment + tile * per_row) return false;
    int64_t b = std::max(bmin, std::min<int64_t>(bcap, (int64_t)(avail / 2 / per_segment)));
    int64_t r = std::max(tile, std::min<int64_t>(rcap, (int64_t)((avail - b * per_segment) / per_row)));
    b = std::min<int64_t>(bcap, (int64_t)((avail - r * per_row) / per_segment));
    if (b < Q) b = round_up(balanced(Q, b / kStep * kStep), kStep);
    r = std::min<int64_t>(rcap, (int64_t)((avail - b * per_segment) / per_row));
    if (r >= tile * K) {
      Rb = std::min<int64_t>(R, r / K);
      if (Rb < R) Rb = round_up(balanced(R, Rb / kTile * kTile), kTile);
      Kb = K;
    } else {
      Rb = tile;
      Kb = balanced(K, r / tile);
    }
    *B = (int)b;
    *rows = (int)(Rb * Kb);
    return true;
  };
  std::lock_guard<std::mutex> lock(g_replicate_cache.mutex);
  ReplicatePlans *sp = nullptr;
  rc = get_segment_plans(g_replicate_cache, device, n, limit, base, choose, &sp);
  if (rc != RN_OK) return rc;
  ReplicatePlans &s = *sp;
  const double *d_alpha = nullptr;
  if ((rc = src.on_device(s.source, (size_t)S * 9 * sizeof(double), &d_alpha)) != RN_OK) return rc;
  if ((rc = upload_taper_and_weights(s, taper, weights, K)) != RN_OK) return rc;
  if ((rc = upload(s.starts, starts, (size_t)Q)) != RN_OK) return rc;
  {
    std::vector<double> vt((size_t)Qpad * Rpad, 0.0);
    for (int64_t r = 0; r < R; ++r)
      for (int64_t q = 0; q < Q; ++q) vt[(size_t)q * Rpad + r] = replicate_weights[r * Q + q];
    if ((rc = upload(s.vt, vt.data(), vt.size())) != RN_OK) return rc;
  }

  g_timer.reset();
  const int B = s.B;
  auto *x = s.x.as<hipfftDoubleComplex>(), *p = s.p.as<hipfftDoubleComplex>();
  const unsigned gf = (unsigned)((L + kWaves * kTile - 1) / (kWaves * kTile));
  std::vector<double> some;  // the rows of a block that holds some of the K configurations
  int64_t held = -1;         // the first segment of the block whose transforms x holds
  auto run = [&]() -> int {
    for (int64_t r0 = 0; r0 < R; r0 += Rb) {
      const int rcount = (int)std::min<int64_t>(Rb, R - r0);
      for (int64_t k0 = 0; k0 < K; k0 += Kb) {
        const int kc = (int)std::min<int64_t>(Kb, K - k0);
        for (int64_t q0 = 0; q0 < Q; q0 += B) {
          const int count = (int)std::min<int64_t>(B, Q - q0);
          if (held != q0) {
            g_timer.mark(0);
            build_segments_at_kernel<<<dim3(blocks_of_256(L), (unsigned)B), 256>>>(
                d_alpha, s.tau.as<const double>(), n, L, s.starts.as<const int64_t>(), q0, count, x);
            g_timer.mark(1);
            held = -1;
            if (!s.plan_x.exec(s.x.ptr, HIPFFT_FORWARD)) return RN_ERR_HIP;
            held = q0;
          }
          g_timer.mark(2);
          replicate_power_kernel<<<dim3(gf, (unsigned)((rcount + kTile - 1) / kTile)), kReplicateThreads>>>(
              x, L, B, count, s.vt.as<const double>(), Rpad, q0, r0, rcount, s.w.as<const double>(), k0, kc, q0 == 0, p);
        }
        g_timer.mark(3);
        const int rows = rcount * kc;
        if (kc == K) {
          if (int e = segment_rows_to_host(s, rows, intensities + r0 * K * bins)) return e;
        } else {
          some.resize((size_t)rows * bins);
          if (int e = segment_rows_to_host(s, rows, some.data())) return e;
          for (int i = 0; i < rcount; ++i)
            std::copy_n(some.data() + (size_t)i * kc * bins, (size_t)kc * bins, intensities + ((r0 + i) * K + k0) * bins);
        }
        g_timer.close();
      }
    }
    return RN_OK;
  };
  rc = run();
  g_timer.collect();
  return rc;
}

}  // namespace

extern "C" int rn_md_raman_segment_replicates(const double *alpha, int64_t S, int64_t segment_steps,
                                              const int64_t *starts, int64_t Q, const double *taper,
                                              const double *weights, int64_t K, const double *replicate_weights,
                                              int64_t R, int device, size_t workspace_limit, double *intensities,
                                              int64_t num_bins) {
  return md_raman_segment_replicates(Source::host(alpha), S, segment_steps, starts, Q, taper, weights, K,
                                     replicate_weights, R, device, workspace_limit, intensities, num_bins);
}

extern "C" int rn_md_raman_segment_replicates_device(const double *d_alpha, int64_t S, int64_t segment_steps,
                                                     const int64_t *starts, int64_t Q, const double *taper,
                                                     const double *weights, int64_t K, const double *replicate_weights,
                                                     int64_t R, int device, size_t workspace_limit, double *intensities,
                                                     int64_t num_bins, void *stream) {
  return md_raman_segment_replicates(Source::device(d_alpha, stream), S, segment_steps, starts, Q, taper, weights, K,
                                     replicate_weights, R, device, workspace_limit, intensities, num_bins);
}

extern "C" int rn_md_raman_segment_replicates_set_profiling(int enabled) {
  return g_timer.set_profiling(g_replicate_cache.mutex, enabled);
}

extern "C" int rn_md_raman_segment_replicates_phase_times(double *millis) {
  return g_timer.phase_times(g_replicate_cache.mutex, millis);
}
