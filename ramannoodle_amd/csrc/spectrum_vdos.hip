// On-device vibrational density of states (VDOS) of an MD run, whole and by atom group: what
// VibrationalDensityOfStates.measure / measure_segments reduce (include/rn_potgnn.h, rn_md_vdos).
//
// Definition.  Fractional positions f[t][i][c] (S frames, N atoms, wrapped into the cell or not), lattices Lat[t] (rows =
// lattice vectors; one for the run or one per frame), masses m[i], group labels g(i) in [0, G), a start table, W frames
// per segment (n = W - 1 steps) and a taper tau[0..n-1]:
//   minimum-image step   df[t] = f[t+1] - f[t];  df -= rint(df)            (round to nearest even, as np.rint)
//   Cartesian step       u[t] = df[t] @ M[t],  M[t] = Lat (fixed cell) or (Lat[t] + Lat[t+1]) / 2 (a lattice per frame:
//                        the motion relative to the deforming cell); not divided by the timestep
//   segment series       x_{q,i,c}[t] = tau[t] sqrt(m[i]) u[starts[q] + t][i][c],  t = 0..n-1
//   row (q, g)           D_{q,g}(f) = sum_{i: g(i) = g} sum_c C(x_{q,i,c})(f), C = calc_signal_spectrum's transform, bins
//                        1..num_bins of fftfreq(n)
// Everything after the power spectrum is linear, so with X the zero-padded transform (length L = padded_length(n))
//   P_{q,g}(w) = sum_{i in g, c} |X_{q,i,c}(w)|^2
// goes through the shared back half once per row (spectrum_segment_core.hpp: inverse transform, positive lags scaled by
// 1/L, length-n transform, real bins): 3 N forward transforms per segment, G back halves.  average = 1 is the mean over
// the Q segments taken on P.
//
// Pipeline, per block of B segments and A atoms (x[B][A][3][L], atoms in index order):
//   series builder: a transpose.  The positions have a stride of 24 N bytes along time, the rows of x are contiguous
//   along time.  A workgroup stages 65 frames x 32 atoms (96 doubles, contiguous in memory) in LDS, reading along the
//   atoms (768-byte runs per frame), then each wave takes an atom and its 64 lanes 64 consecutive steps: six LDS reads
//   (row stride 97 doubles = 194 dwords: lane t starts at bank 2t mod 64, no conflict within a 32-lane half), the
//   arithmetic above, three 1 KiB runs written.  Steps n <= t < L and segments past the block's count are zeroed.
//   -> 3 A B batched forward FFTs of length L
//   -> group power kernel: p[slot][w] (+)= sum over the block's atoms of the slot's group, and over the block's segments
//   for average = 1.  One thread owns its (slot, w) for the whole call; it walks the group's atoms in ascending index
//   (the host sorts the atom indices by group once per call, stably) and the segments in table order; a `first` flag
//   starts the sum at zero and later blocks go on from p.  No atomics: repeated calls are bit-identical.
// Blocking.  One segment of all atoms is 3 N L complex doubles (3.2 GB at 256 atoms and L = 2^18), so atoms go through
// in blocks as well as segments.  Either a segment's atoms fit one block (A = N, B >= 1) or they do not (B = 1, A < N):
// both give the order "segment by segment, atom by atom" for every (slot, w), so the sums do not depend on the block
// sizes.  When G rows do not fit either, the groups go through in blocks and the series are transformed again for each.
// float64 throughout.  A plan cache of its own, keyed by (device, n, 3 A, B, slots).  All work runs on the null stream
// (after a synchronise of the caller's stream in the _device entry).
#include "kernels.hpp"
#include "spectrum_steps.hpp"

namespace {
using namespace rn_spectrum;
using rn::kMaxGroups;

constexpr int kTileSteps = 64;                  // steps per builder tile: one per lane
constexpr int kTileAtoms = 32;                  // atoms per builder tile
constexpr int kTileCols = 3 * kTileAtoms;       // doubles per staged frame
constexpr int kTileStride = kTileCols + 1;      // LDS row stride in doubles (odd: see the head of this file)
constexpr int kBuilderThreads = 256;
constexpr int kGroupPowerThreads = 64;          // one wave per workgroup: L / 64 workgroups per slot
constexpr int64_t kMaxAtomsPerBlock = (int64_t)kTileAtoms * 65535;  // gridDim.y of the builder

// segment b = blockIdx.z of the block (segments q0 .. q0+count-1), atoms a0 .. a0+ac-1 (slot a - a0 of the A slots):
// x[b][a - a0][c][t] = tau[t] sqrt_mass[a] u[starts[q0+b] + t][a][c] for t < n; zero for n <= t < L and for b >= count
__global__ void __launch_bounds__(kBuilderThreads)
    build_series_kernel(const double *__restrict__ pos, const double *__restrict__ lat, int per_frame, int64_t N,
                        const double *__restrict__ sqrt_mass, const double *__restrict__ tau, int64_t n, int64_t L,
                        const int64_t *__restrict__ starts, int64_t q0, int count, int64_t a0, int ac, int64_t A,
                        hipfftDoubleComplex *__restrict__ x) {
  __shared__ double raw[(kTileSteps + 1) * kTileStride];
  const int64_t t0 = (int64_t)blockIdx.x * kTileSteps;
  const int tile_a = blockIdx.y * kTileAtoms;               // first atom of the tile, within the block
  const int b = blockIdx.z;
  const int atoms = std::min(kTileAtoms, ac - tile_a);           // >= 1 by the grid
  const bool live = b < count && t0 < n;
  const int64_t start = live ? starts[q0 + b] : 0;
  if (live) {
    // frames start + t0 .. start + t0 + 64, no further than the segment's last frame start + n
    const int frames = (int)std::min<int64_t>(kTileSteps + 1, n + 1 - t0);
    const int cols = 3 * atoms;
    const double *src = pos + ((start + t0) * N + a0 + tile_a) * 3;
    for (int i = threadIdx.x; i < (kTileSteps + 1) * kTileCols; i += kBuilderThreads) {
      const int r = i / kTileCols, col = i % kTileCols;
      raw[r * kTileStride + col] = (r < frames && col < cols) ? src[(int64_t)r * N * 3 + col] : 0.0;
    }
  }
  __syncthreads();
  const int lane = threadIdx.x % kTileSteps, wave = threadIdx.x / kTileSteps;
  const int64_t t = t0 + lane;
  if (t >= L) return;
  const bool step = live && t < n;
  double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  double w = 0.0;
  if (step) {
    const double *l0 = lat + (per_frame ? (start + t) * 9 : 0);
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = per_frame ? 0.5 * (l0[k] + l0[9 + k]) : l0[k];
    w = tau[t];
  }
  for (int a = wave; a < atoms; a += kBuilderThreads / kTileSteps) {
    double u[3] = {0.0, 0.0, 0.0};
    if (step) {
      const double *r0 = raw + lane * kTileStride + 3 * a, *r1 = r0 + kTileStride;
      double d[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        d[k] = r1[k] - r0[k];
        d[k] -= rint(d[k]);
      }
      const double s = w * sqrt_mass[a0 + tile_a + a];
#pragma unroll
      for (int c = 0; c < 3; ++c) u[c] = s * (d[0] * m[c] + d[1] * m[3 + c] + d[2] * m[6 + c]);
    }
    hipfftDoubleComplex *row = x + (((int64_t)b * A + tile_a + a) * 3) * L + t;
#pragma unroll
    for (int c = 0; c < 3; ++c) row[c * L] = make_double2(u[c], 0.0);
  }
}

// where the block's atoms of each group lie in the atom list sorted by group: list[lo[g]] .. list[hi[g] - 1]
struct GroupRanges {
  int lo[kMaxGroups], hi[kMaxGroups];
};

// Slot s = blockIdx.y of p.  average = 1: slot j is group g0 + j and sums the block's `count` segments in order;
// average = 0: slot b gc + j is group g0 + j of segment b.  p[s][w] (+)= inv_q sum over the slot's segments, then over
// the group's atoms of the block in ascending index, of |X_x|^2 + |X_y|^2 + |X_z|^2; `first` starts at zero.  Slots
// without a group or a segment (j >= gc, b >= count) add nothing, so the first launch zeroes them.
__global__ void __launch_bounds__(kGroupPowerThreads)
    group_power_kernel(const hipfftDoubleComplex *__restrict__ x, int64_t L, int64_t A, int64_t a0, int count,
                       const int32_t *__restrict__ list, GroupRanges ranges, int g0, int gc, int average, double inv_q,
                       int first, hipfftDoubleComplex *__restrict__ p) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= L) return;
  const int slot = blockIdx.y;
  const int j = average ? slot : slot % gc;
  const int b0 = average ? 0 : slot / gc;
  const int b1 = average ? count : std::min(b0 + 1, count);
  hipfftDoubleComplex *out = p + (int64_t)slot * L + f;
  double acc = first ? 0.0 : out->x;
  if (j < gc) {
    const int lo = ranges.lo[g0 + j], hi = ranges.hi[g0 + j];
    for (int b = b0; b < b1; ++b) {
      const hipfftDoubleComplex *xb = x + (int64_t)b * A * 3 * L + f;
#pragma unroll 4
      for (int i = lo; i < hi; ++i) {
        const hipfftDoubleComplex *xa = xb + (list[i] - a0) * 3 * L;
        const hipfftDoubleComplex vx = xa[0], vy = xa[L], vz = xa[2 * L];
        const double s = (vx.x * vx.x + vx.y * vx.y) + (vy.x * vy.x + vy.y * vy.y) + (vz.x * vz.x + vz.y * vz.y);
        acc = fma(s, inv_q, acc);
      }
    }
  }
  *out = make_double2(acc, 0.0);
}

// the plans and buffers of spectrum_steps.hpp (series = 3 A) and what this reducer adds to them
struct VdosPlans : StepPlans {
  DeviceBuffer list;  // atom indices sorted by group, int32[N]; the square roots of the masses are in `w`
};
PlanCache<VdosPlans> g_vdos_cache;  // apart from the caches of the other reducers
PhaseTimer g_timer;                 // builder, forward FFTs, power kernel, back half; under g_vdos_cache.mutex

// A atoms and B segments per block and the slots of p (groups per block gr: slots = gr, or B gr for average = 0) for
// `avail` bytes; false when one atom of one segment and one row do not fit
bool choose_vdos_blocks(size_t avail, int64_t L, int64_t bins, int64_t N, int G, int64_t Q, int average, int64_t *A,
                        int *B, int *gr) {
  const size_t cz = sizeof(hipfftDoubleComplex);
  const size_t per_atom = 3 * (size_t)L * cz, per_row = (size_t)L * cz + (size_t)bins * sizeof(double);
  if (avail < per_atom + per_row) return false;
  const int64_t rows_most = std::min<int64_t>(kMaxRows, std::max<int64_t>(1, (int64_t)(kMaxBlockBytes / ((size_t)L * cz))));
  const int64_t groups =
      std::max<int64_t>(1, std::min<int64_t>({(int64_t)G, rows_most, (int64_t)(std::min(avail / 2, avail - per_atom) / per_row)}));
  const size_t left = avail - (size_t)groups * per_row;  // >= per_atom
  const int64_t atoms_fit = (int64_t)(std::min(left, std::max(kMaxBlockBytes, per_atom)) / per_atom);
  *gr = (int)groups;
  if (atoms_fit < N || N > kMaxAtomsPerBlock) {
    *A = balanced(N, std::min(atoms_fit, kMaxAtomsPerBlock));
    *B = 1;
    return true;
  }
  *A = N;
  const size_t per_segment = (size_t)N * per_atom;
  int64_t b = std::min<int64_t>({Q, kMaxSegments, std::max<int64_t>(1, (int64_t)(kMaxBlockBytes / per_segment))});
  if (average)
    b = std::min<int64_t>(b, (int64_t)(left / per_segment));
  else
    b = std::min<int64_t>({b, (int64_t)(avail / (per_segment + (size_t)groups * per_row)), rows_most / groups});
  *B = (int)balanced(Q, std::max<int64_t>(1, b));
  return true;
}

// d_pos: device float64[S][N][3], d_lat: device float64[1 or S][9] -> out: host [G][bins] (average) or [Q][G][bins]
int vdos_on_device(VdosPlans &s, int groups_per_block, const double *d_pos, const double *d_lat, int per_frame, int64_t N,
                   const std::vector<int32_t> &list, const std::vector<int> &group_begin, int G, int64_t Q, int average,
                   double *out) {
  const int64_t L = s.L, bins = num_bins(s.n), A = s.series / 3;
  const int B = s.B;
  auto *x = s.x.as<hipfftDoubleComplex>(), *p = s.p.as<hipfftDoubleComplex>();
  const unsigned tiles_t = (unsigned)((L + kTileSteps - 1) / kTileSteps);
  const unsigned power_x = (unsigned)((L + kGroupPowerThreads - 1) / kGroupPowerThreads);
  std::vector<double> rows;  // the block's rows, when they are not contiguous in `out`
  int rc;
  for (int g0 = 0; g0 < G; g0 += groups_per_block) {
    const int gc = std::min(groups_per_block, G - g0);
    for (int64_t q0 = 0; q0 < Q; q0 += B) {
      const int count = (int)std::min<int64_t>(B, Q - q0);
      bool first = !average || q0 == 0;
      for (int64_t a0 = 0; a0 < N; a0 += A) {
        const int ac = (int)std::min<int64_t>(A, N - a0);
        GroupRanges ranges;
        bool any = false;
        for (int g = 0; g < kMaxGroups; ++g) {
          ranges.lo[g] = ranges.hi[g] = 0;
          if (g < g0 || g >= g0 + gc) continue;
          const auto lo = list.begin() + group_begin[g], hi = list.begin() + group_begin[g + 1];
          ranges.lo[g] = (int)(std::lower_bound(lo, hi, (int32_t)a0) - list.begin());
          ranges.hi[g] = (int)(std::lower_bound(lo, hi, (int32_t)(a0 + ac)) - list.begin());
          any = any || ranges.hi[g] > ranges.lo[g];
        }
        if (!any && !first) continue;  // none of the block's atoms is in these groups
        if (any) {
          g_timer.mark(0);
          build_series_kernel<<<dim3(tiles_t, (unsigned)((ac + kTileAtoms - 1) / kTileAtoms), (unsigned)B),
                                kBuilderThreads>>>(d_pos, d_lat, per_frame, N, s.w.as<const double>(),
                                                   s.tau.as<const double>(), s.n, L, s.starts.as<const int64_t>(), q0,
                                                   count, a0, ac, A, x);
          g_timer.mark(1);
          if (!s.plan_x.exec(x, HIPFFT_FORWARD)) return RN_ERR_HIP;
        }
        g_timer.mark(2);
        group_power_kernel<<<dim3(power_x, (unsigned)s.R), kGroupPowerThreads>>>(
            x, L, A, a0, any ? count : 0, s.list.as<const int32_t>(), ranges, g0, gc, average,
            average ? 1.0 / (double)Q : 1.0, first, p);
        first = false;
      }
      if (average) continue;
      g_timer.mark(3);
      if (gc == G) {
        rc = segment_rows_to_host(s, count * G, out + q0 * G * bins);
      } else {
        rows.resize((size_t)count * gc * bins);
        rc = segment_rows_to_host(s, count * gc, rows.data());
        for (int b = 0; rc == RN_OK && b < count; ++b)
          std::copy_n(rows.data() + (size_t)b * gc * bins, (size_t)gc * bins, out + ((q0 + b) * G + g0) * bins);
      }
      g_timer.close();
      if (rc != RN_OK) return rc;
    }
    if (average) {
      g_timer.mark(3);
      rc = segment_rows_to_host(s, gc, out + (int64_t)g0 * bins);
      g_timer.close();
      if (rc != RN_OK) return rc;
    }
  }
  return RN_OK;
}

// both entries: positions (float64[S][N][3]) and lattices (float64[1 or S][3][3]) from `pos` / `lat`; the rest host arrays
int md_vdos(Source pos, Source lat, int64_t num_lattices, int64_t S, int32_t N, const double *masses,
            const int32_t *labels, int G, int64_t W, const int64_t *starts, int64_t Q, const double *taper, int average,
            int device, size_t workspace_limit, double *densities, int64_t bins) {
  if (!labels || G < 1 || G > kMaxGroups) return RN_ERR_INVALID_ARGUMENT;
  for (int32_t i = 0; i < N; ++i)
    if (labels[i] < 0 || labels[i] >= G) return RN_ERR_INVALID_ARGUMENT;
  int64_t n = 0;
  std::vector<double> sqrt_mass;
  int rc = begin_step_call(pos, lat, num_lattices, S, N, masses, W, starts, Q, taper, average, device, bins, densities,
                           &n, &sqrt_mass);
  if (rc != RN_OK || bins == 0) return rc;

  // the atoms sorted by group, stably: ascending index within a group
  std::vector<int> group_begin(G + 1, 0);
  for (int32_t i = 0; i < N; ++i) ++group_begin[labels[i] + 1];
  for (int g = 0; g < G; ++g) group_begin[g + 1] += group_begin[g];
  std::vector<int32_t> list(N);
  {
    std::vector<int> next(group_begin.begin(), group_begin.end() - 1);
    for (int32_t i = 0; i < N; ++i) list[next[labels[i]]++] = i;
  }

  const size_t limit = workspace_limit ? workspace_limit : kDefaultWorkspace;
  const size_t base = (size_t)n * sizeof(double) + (size_t)Q * sizeof(int64_t) +
                      (size_t)N * (sizeof(double) + sizeof(int32_t));  // the taper, the table, sqrt(m), the atom list
  std::lock_guard<std::mutex> lock(g_vdos_cache.mutex);
  VdosPlans *sp = nullptr;
  int groups_per_block = 0;
  const int64_t L = padded_length(n);
  auto choose = [&](size_t avail, int *series, int *B, int *slots) {
    int64_t A = 0;
    if (!choose_vdos_blocks(avail, L, bins, N, G, Q, average, &A, B, &groups_per_block)) return false;
    *series = (int)(3 * A);
    *slots = average ? groups_per_block : *B * groups_per_block;
    return true;
  };
  if ((rc = get_segment_plans(g_vdos_cache, device, n, limit, base, choose, &sp)) != RN_OK) return rc;
  VdosPlans &s = *sp;
  const double *d_pos = nullptr, *d_lat = nullptr;
  if ((rc = stage_step_call(s, pos, lat, num_lattices, S, N, taper, starts, Q, &d_pos, &d_lat)) != RN_OK ||
      (rc = upload(s.w, sqrt_mass.data(), (size_t)N)) != RN_OK || (rc = upload(s.list, list.data(), (size_t)N)) != RN_OK)
    return rc;
  g_timer.reset();
  rc = vdos_on_device(s, groups_per_block, d_pos, d_lat, num_lattices != 1, N, list, group_begin, G, Q, average,
                      densities);
  g_timer.collect();
  return rc;
}

}  // namespace

extern "C" int rn_md_vdos(const double *positions, const double *lattices, int64_t num_lattices, int64_t S, int32_t N,
                          const double *masses, const int32_t *labels, int G, int64_t segment_steps,
                          const int64_t *starts, int64_t Q, const double *taper, int average, int device,
                          size_t workspace_limit, double *densities, int64_t num_bins) {
  return md_vdos(Source::host(positions), Source::host(lattices), num_lattices, S, N, masses, labels, G, segment_steps,
                 starts, Q, taper, average, device, workspace_limit, densities, num_bins);
}

extern "C" int rn_md_vdos_device(const double *d_positions, const double *d_lattices, int64_t num_lattices, int64_t S,
                                 int32_t N, const double *masses, const int32_t *labels, int G, int64_t segment_steps,
                                 const int64_t *starts, int64_t Q, const double *taper, int average, int device,
                                 size_t workspace_limit, double *densities, int64_t num_bins, void *stream) {
  return md_vdos(Source::device(d_positions, stream), Source::device(d_lattices, stream), num_lattices, S, N, masses,
                 labels, G, segment_steps, starts, Q, taper, average, device, workspace_limit, densities, num_bins);
}

extern "C" int rn_md_vdos_set_profiling(int enabled) { return g_timer.set_profiling(g_vdos_cache.mutex, enabled); }

extern "C" int rn_md_vdos_phase_times(double *millis) { return g_timer.phase_times(g_vdos_cache.mutex, millis); }
