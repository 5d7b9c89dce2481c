// On-device mode-projected VDOS of an MD run: the power spectrum of the run's mass-weighted steps projected onto given
// vectors (the harmonic eigenvectors: the normal-mode decomposition of MD), one row per vector.  What
// ModeVibrationalDensityOfStates.measure / measure_segments reduce (include/rn_potgnn.h, rn_md_mode_vdos).
//
// Definition.  Fractional positions f[t][i][c] (S frames, N atoms, wrapped into the cell or not), lattices Lat[t] (rows =
// lattice vectors; one for the run or one per frame), masses m[i], projection vectors v[k][i][c] (k = 0..M-1,
// 1 <= M <= 3 N, applied as given: normalisation is the caller's), a start table, W frames per segment (n = W - 1 steps)
// and a taper tau[0..n-1]:
//   minimum-image step   df[t] = f[t+1] - f[t];  df -= rint(df)            (round to nearest even, as np.rint)
//   Cartesian step       u[t] = df[t] @ M[t],  M[t] = Lat (fixed cell) or (Lat[t] + Lat[t+1]) / 2 (a lattice per frame);
//                        not divided by the timestep: exactly the step of spectrum_vdos.hip
//   mode series          y_{q,k}[t] = tau[t] sum_{i,c} v[k][i][c] sqrt(m[i]) u[starts[q] + t][i][c],  t = 0..n-1
//   row (q, k)           D_{q,k}(f) = C(y_{q,k})(f), C = calc_signal_spectrum's transform, bins 1..num_bins of fftfreq(n)
// computed as in the VDOS: with Y the zero-padded transform (length L = padded_length(n)), P_{q,k}(w) = |Y_{q,k}(w)|^2
// goes through the shared back half (spectrum_segment_core.hpp, segment_rows_to_host) once per row.  average = 1 is the
// mean over the Q segments taken on P.  For a complete orthonormal set the rows sum to the one-group VDOS (Parseval).
//
// Pipeline, per block of B segments and Mb modes (x[B][Mb][L], contiguous along t):
//   projection kernel: a float64 tall-skinny product (steps x 3N by 3N x modes) on the matrix pipe with the minimum-image
//   step fused into its operand.  A workgroup (4 waves) owns 64 steps x 64 modes of one segment and walks the atoms in
//   ascending tiles of 32.  Per atom tile a thread (one of 32 atoms x 8 groups of steps) loads its atom's three
//   doubles of nine consecutive frames (768-byte runs per frame across the atoms), makes the atom's eight steps from
//   them in registers (minimum image, then the step's lattice or midpoint, which the workgroup keeps in LDS) and
//   writes them to the 64 x 96 step tile in LDS (row stride 97 doubles: the sixteen lanes of an operand read start at
//   banks 2 l15 mod 32 and touch every bank once).  Then v_mfma_f64_16x16x4_f64 runs over the tile's 24 k-steps: a
//   wave holds 16 modes x 64 steps in four accumulators.  The vectors (sqrt(m) folded in on the host: vw[k][3i+c])
//   are the instruction's first operand, read from global memory once per atom tile (24 doubles per lane,
//   L2-resident), the steps the second, read from LDS.  Result register j of lane (l15, quad) is then mode 4 j + quad
//   at step l15 (kernels_gemm.hip, rowgemm_f64_mfma_kernel; tools/mfma_f64_layout_probe.hip), so sixteen lanes store
//   a contiguous 256-byte run along t.  The frames of the next atom tile are requested before the products of this one
//   and land in registers while the matrix pipe works.  The remainder of 3N to the tile and of the modes to the tile
//   are zeros in LDS / registers; nothing is read past an array.  The taper multiplies the accumulator at the store;
//   steps n <= t < L and segment slots past the block's count are zeroed by the same kernel.
//   The sum over (i, c) has one order: atom tiles ascending, k-steps ascending, the instruction's own order within a
//   k-step.  It does not depend on B or Mb, and there are no atomics: repeated calls are bit-identical.
//   -> Mb B batched forward FFTs of length L
//   -> diagonal power kernels: p[slot][w] = |X[slot][w]|^2 (average = 0), pbar[k][w] (+)= sum_b |X[b][k][w]|^2 / Q in
//   segment order (average = 1).  One thread owns its (slot, w).
// Blocking.  One segment of M series is M L complex doubles (3.2 GB at M = 768 and L = 2^18), so the modes go through
// in an outer loop of blocks of Mb (a short last block is padded with zero vectors), each through run_segments with
// series = rows = Mb.  Modes are independent, so every row's arithmetic is the same whatever Mb and B are.
// float64 throughout.  A plan cache of its own, keyed by (device, n, Mb, B, R).  All work runs on the null stream (after
// a synchronise of the caller's stream in the _device entry).
// What this reducer shares with spectrum_vdos.hip is in spectrum_steps.hpp: the entry front end, the staging of
// positions and lattices and the plans entry that holds the staged lattices.  The step arithmetic is written out in
// both kernels (spectrum_steps.hpp says why): there a lane owns a step and reads two staged frames from LDS, here a
// thread owns an atom's eight steps and keeps nine frames in registers, so that the loads overlap the products.
#include "spectrum_steps.hpp"

namespace {
using namespace rn_spectrum;

constexpr int kTileSteps = 64;                  // steps per tile
constexpr int kTileModes = 64;                  // modes per tile: 16 per wave
constexpr int kTileAtoms = 32;                  // atoms per tile
constexpr int kTileCols = 3 * kTileAtoms;       // doubles per frame of the tile
constexpr int kTileStride = kTileCols + 1;      // LDS row stride in doubles (odd: see the head of this file)
constexpr int kKSteps = kTileCols / 4;          // k-steps of the 16x16x4 instruction per atom tile
constexpr int kProjectThreads = 256;
constexpr int kStepsPerThread = kTileSteps / (kProjectThreads / kTileAtoms);  // steps an atom's thread makes per tile
constexpr int kDiagThreads = 256;
constexpr int64_t kMaxModesPerBlock = (int64_t)kTileModes * 65535;  // gridDim.y of the projection kernel

typedef double f64x4_t __attribute__((ext_vector_type(4)));

// segment b = blockIdx.z of the block (segments q0 .. q0+count-1), modes k0 .. k0+kc-1 (slot k - k0 of the Mb slots):
// x[b][k - k0][t] = tau[t] sum_j vw[k][j] u[starts[q0+b] + t][j] for t < n and k - k0 < kc; zero for n <= t < L, for
// kc <= k - k0 < Mb and for b >= count.  K3 = 3 N columns of vw and of a frame.
__global__ void __launch_bounds__(kProjectThreads, 2)
    project_steps_kernel(const double *__restrict__ pos, const double *__restrict__ lat, int per_frame, int64_t K3,
                         const double *__restrict__ vw, const double *__restrict__ tau, int64_t n, int64_t L,
                         const int64_t *__restrict__ starts, int64_t q0, int count, int64_t k0, int kc, int Mb,
                         hipfftDoubleComplex *__restrict__ x) {
  __shared__ double steps[kTileSteps * kTileStride];  // the tile's Cartesian steps: [step][column], odd row stride
  __shared__ double mid[kTileSteps * 9];              // the lattice of each step (a lattice per frame: the midpoint)
  const int64_t t0 = (int64_t)blockIdx.x * kTileSteps;
  const int b = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, quad = lane >> 4;
  const int mode0 = blockIdx.y * kTileModes + wave * 16;  // the wave's first mode, within the block
  hipfftDoubleComplex *xb = x + (int64_t)b * Mb * L;
  if (b >= count || t0 >= n) {  // (the same for the whole workgroup: no barrier is skipped by a part of it)
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int mode = mode0 + 4 * j + quad;
        const int64_t t = t0 + 16 * s + l15;
        if (mode < Mb && t < L) xb[(int64_t)mode * L + t] = make_double2(0.0, 0.0);
      }
    return;
  }
  const int64_t start = starts[q0 + b];
  // frames start + t0 .. start + t0 + 64, no further than the segment's last frame start + n: frames - 1 steps
  const int frames = (int)std::min<int64_t>(kTileSteps + 1, n + 1 - t0);
  // Loads are unconditional, from a clamped address, with the zero selected (or multiplied in) afterwards: a
  // conditional load makes the compiler branch around each one and wait for it alone.
  for (int i = threadIdx.x; i < kTileSteps * 9; i += kProjectThreads) {
    const int t = i / 9, k = i % 9;
    const bool in = t < frames - 1;
    // (for a fixed cell both reads are the one lattice and (x + x) / 2 = x exactly)
    const double *l0 = lat + (per_frame && in ? (start + t0 + t) * 9 : 0), *l1 = l0 + (per_frame && in ? 9 : 0);
    mid[i] = 0.5 * (l0[k] + l1[k]);
  }
  const bool mode_live = mode0 + l15 < kc;  // the mode whose vector this lane holds (first operand: row l15)
  const double *vrow = vw + (k0 + (mode_live ? mode0 + l15 : 0)) * K3;
  f64x4_t acc[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) acc[s] = f64x4_t{0.0, 0.0, 0.0, 0.0};

  // Staging: thread (group = threadIdx.x / 32, atom = threadIdx.x % 32) loads the atom's three doubles of the nine
  // frames 8 group .. 8 group + 8 (one pointer that advances by a frame) and makes the atom's eight steps
  // 8 group .. 8 group + 7 from them in registers.  The loads of the next tile are issued before the products of this
  // one and land while the matrix pipe works.
  const int step0 = kStepsPerThread * (threadIdx.x / kTileAtoms), stage_col = 3 * (threadIdx.x % kTileAtoms);
  const double *frame0 = pos + (start + t0) * K3;
  double staged[kStepsPerThread + 1][3];
  auto load_tile = [&](int64_t c0) {
    const double *first = frame0 + c0 + (c0 + stage_col < K3 ? stage_col : 0), *p = first + step0 * K3;
#pragma unroll
    for (int j = 0; j <= kStepsPerThread; ++j) {
      const double *q = step0 + j < frames ? p : first;
#pragma unroll
      for (int k = 0; k < 3; ++k) staged[j][k] = q[k];
      p += K3;
    }
  };
  load_tile(0);
  __syncthreads();  // mid
  for (int64_t c0 = 0; c0 < K3; c0 += kTileCols) {  // the atom tile's first column
    const int cols = (int)std::min<int64_t>(kTileCols, K3 - c0);
    // the wave's vectors for this tile: vw[mode0 + l15][c0 + 4 ks + quad], zero past the modes or the columns.  The
    // zero is a product with 0 (every entry of vw is finite): a select lets the compiler sink the load into a branch.
    double a[kKSteps];
#pragma unroll
    for (int ks = 0; ks < kKSteps; ++ks) {
      const int col = 4 * ks + quad;
      a[ks] = vrow[col < cols ? c0 + col : 0] * ((mode_live && col < cols) ? 1.0 : 0.0);
    }
    // frames -> steps: minimum image, then the step's lattice; zero past the segment's steps and the atoms
#pragma unroll
    for (int j = 0; j < kStepsPerThread; ++j) {
      const int t = step0 + j;
      const bool in = t < frames - 1 && stage_col < cols;
      double d[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        d[k] = staged[j + 1][k] - staged[j][k];
        d[k] -= rint(d[k]);
      }
      const double *m = mid + 9 * t;
#pragma unroll
      for (int c = 0; c < 3; ++c)
        steps[t * kTileStride + stage_col + c] = in ? d[0] * m[c] + d[1] * m[3 + c] + d[2] * m[6 + c] : 0.0;
    }
    __syncthreads();
    if (c0 + kTileCols < K3) load_tile(c0 + kTileCols);
    // second operand: lane (l15, quad) holds step 16 s + l15, column 4 ks + quad
#pragma unroll
    for (int ks = 0; ks < kKSteps; ++ks)
#pragma unroll
      for (int s = 0; s < 4; ++s)
        acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], steps[(16 * s + l15) * kTileStride + 4 * ks + quad], acc[s],
                                                      0, 0, 0);
    __syncthreads();  // the next tile's steps are written over these
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int64_t t = t0 + 16 * s + l15;
    if (t >= L) continue;
    const double w = tau[t < n ? t : 0];  // (unconditional: see the staging loads)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int mode = mode0 + 4 * j + quad;
      if (mode < Mb) xb[(int64_t)mode * L + t] = make_double2(t < n ? w * acc[s][j] : 0.0, 0.0);
    }
  }
}

// average = 0.  Slot j = blockIdx.y of p: the power of series r0 + j of x (series r = b Mb + mode of the block); slots
// >= count are zeroed.
__global__ void __launch_bounds__(kDiagThreads)
    diagonal_power_kernel(const hipfftDoubleComplex *__restrict__ x, int64_t L, int64_t r0, int count,
                          hipfftDoubleComplex *__restrict__ p) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= L) return;
  const int j = blockIdx.y;
  double v = 0.0;
  if (j < count) {
    const hipfftDoubleComplex z = x[(r0 + j) * L + f];
    v = z.x * z.x + z.y * z.y;
  }
  p[(int64_t)j * L + f] = make_double2(v, 0.0);
}

// average = 1.  Slot i = blockIdx.y of pbar (mode r0 + i of the block, i < rc): pbar[i][f] (+)= sum over the block's
// `count` segments, in order, of |X[b][r0 + i][f]|^2 inv_q; `first` starts the sum at zero; slots >= rc are zeroed.
// One thread owns its (mode, f) for the whole call.
__global__ void __launch_bounds__(kDiagThreads)
    diagonal_mean_power_kernel(const hipfftDoubleComplex *__restrict__ x, int64_t L, int Mb, int count, int64_t r0,
                               int rc, double inv_q, int first, hipfftDoubleComplex *__restrict__ pbar) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= L) return;
  const int i = blockIdx.y;
  hipfftDoubleComplex *out = pbar + (int64_t)i * L + f;
  double acc = (first || i >= rc) ? 0.0 : out->x;
  if (i < rc)
    for (int b = 0; b < count; ++b) {
      const hipfftDoubleComplex z = x[((int64_t)b * Mb + r0 + i) * L + f];
      acc = fma(z.x * z.x + z.y * z.y, inv_q, acc);
    }
  *out = make_double2(acc, 0.0);
}

// the plans and buffers of spectrum_steps.hpp (series = rows = Mb; the weighted vectors are in `w`), apart from the other
// reducers' caches
PlanCache<StepPlans> g_mode_cache;
PhaseTimer g_timer;  // projection, forward FFTs, power kernel, back half; under g_mode_cache.mutex

// the most modes per block whose series and rows of one segment fit `avail` bytes and the caps of the core; 0: not one
int64_t modes_per_block(size_t avail, int64_t L, int64_t bins, int64_t M) {
  const size_t cz = sizeof(hipfftDoubleComplex);
  const size_t per_mode = 2 * (size_t)L * cz + (size_t)bins * sizeof(double);  // one series, one row
  const int64_t most = std::min<int64_t>(
      {M, kMaxModesPerBlock, kMaxRows, std::max<int64_t>(1, (int64_t)(kMaxBlockBytes / ((size_t)L * cz)))});
  return std::min<int64_t>(most, (int64_t)(avail / per_mode));
}

// d_pos: device float64[S][N][3], d_lat: device float64[1 or S][9], s.w: vw[M][3N] -> out: host [M][bins] (average) or
// [Q][M][bins]
int mode_vdos_on_device(SegmentPlans &s, const double *d_pos, const double *d_lat, int per_frame, int64_t K3, int64_t M,
                        int64_t Q, int average, double *out) {
  const int64_t L = s.L, bins = num_bins(s.n);
  const int Mb = s.series, B = s.B;
  auto *x = s.x.as<hipfftDoubleComplex>(), *p = s.p.as<hipfftDoubleComplex>();
  const unsigned tiles_t = (unsigned)((L + kTileSteps - 1) / kTileSteps);
  const unsigned tiles_m = (unsigned)((Mb + kTileModes - 1) / kTileModes);
  const unsigned diag_x = (unsigned)((L + kDiagThreads - 1) / kDiagThreads);
  const int64_t segments = average ? 1 : Q;
  std::vector<double> rows;  // a block's rows, when they are not the rows of `out`
  for (int64_t k0 = 0; k0 < M; k0 += Mb) {
    const int kc = (int)std::min<int64_t>(Mb, M - k0);
    auto build = [&](int64_t q0, int count) {
      g_timer.mark(0);
      project_steps_kernel<<<dim3(tiles_t, tiles_m, (unsigned)B), kProjectThreads>>>(
          d_pos, d_lat, per_frame, K3, s.w.as<const double>(), s.tau.as<const double>(), s.n, L,
          s.starts.as<const int64_t>(), q0, count, k0, kc, Mb, x);
      g_timer.mark(1);
    };
    auto mean_power = [&](int count, int64_t r0, int rc, bool first) {
      g_timer.mark(2);
      diagonal_mean_power_kernel<<<dim3(diag_x, (unsigned)s.R), kDiagThreads>>>(x, L, Mb, count, r0, rc,
                                                                                 1.0 / (double)Q, first, p);
      g_timer.mark(3);
    };
    auto row_power = [&](int64_t r0, int rc) {
      g_timer.mark(2);
      diagonal_power_kernel<<<dim3(diag_x, (unsigned)s.R), kDiagThreads>>>(x, L, r0, rc, p);
      g_timer.mark(3);
    };
    int rc;
    if (Mb == M) {
      rc = run_segments(s, Q, Mb, average, build, mean_power, row_power, out);
    } else {
      rows.resize((size_t)segments * Mb * bins);
      rc = run_segments(s, Q, Mb, average, build, mean_power, row_power, rows.data());
      for (int64_t q = 0; rc == RN_OK && q < segments; ++q)
        std::copy_n(rows.data() + (size_t)q * Mb * bins, (size_t)kc * bins, out + (q * M + k0) * bins);
    }
    g_timer.close();
    if (rc != RN_OK) return rc;
  }
  return RN_OK;
}

// both entries: positions (float64[S][N][3]) and lattices (float64[1 or S][3][3]) from `pos` / `lat`; the rest host arrays
int md_mode_vdos(Source pos, Source lat, int64_t num_lattices, int64_t S, int32_t N, const double *masses,
                 const double *vectors, int32_t M, int64_t W, const int64_t *starts, int64_t Q, const double *taper,
                 int average, int device, size_t workspace_limit, double *densities, int64_t bins) {
  if (!vectors || M < 1 || (int64_t)M > 3 * (int64_t)N) return RN_ERR_INVALID_ARGUMENT;
  const int64_t K3 = 3 * (int64_t)N;
  for (int64_t j = 0; j < (int64_t)M * K3; ++j)
    if (!std::isfinite(vectors[j])) return RN_ERR_INVALID_ARGUMENT;
  int64_t n = 0;
  std::vector<double> sqrt_mass;
  int rc = begin_step_call(pos, lat, num_lattices, S, N, masses, W, starts, Q, taper, average, device, bins, densities,
                           &n, &sqrt_mass);
  if (rc != RN_OK || bins == 0) return rc;

  // sqrt(m) folded into the vectors, once per call
  std::vector<double> vw((size_t)M * K3);
  for (int64_t k = 0; k < M; ++k)
    for (int64_t j = 0; j < K3; ++j) vw[k * K3 + j] = vectors[k * K3 + j] * sqrt_mass[j / 3];

  const int64_t L = padded_length(n);
  const size_t limit = workspace_limit ? workspace_limit : kDefaultWorkspace;
  const size_t base = (size_t)n * sizeof(double) + (size_t)Q * sizeof(int64_t) +
                      vw.size() * sizeof(double);  // the taper, the table, the weighted vectors
  if (limit <= base) return RN_ERR_OUT_OF_MEMORY;
  std::lock_guard<std::mutex> lock(g_mode_cache.mutex);
  int64_t most = modes_per_block(limit - base, L, bins, M);
  if (most < 1) return RN_ERR_OUT_OF_MEMORY;
  StepPlans *sp = nullptr;
  for (;;) {  // (the plans' work areas may not fit beside the largest block: halve it)
    const int Mb = (int)balanced(M, most);
    rc = get_segment_plans(g_mode_cache, device, n, Mb, Q, Mb, average, limit, base, &sp);
    if (rc != RN_ERR_OUT_OF_MEMORY || most == 1) break;
    most = (most + 1) / 2;
  }
  if (rc != RN_OK) return rc;
  StepPlans &s = *sp;
  const double *d_pos = nullptr, *d_lat = nullptr;
  if ((rc = stage_step_call(s, pos, lat, num_lattices, S, N, taper, starts, Q, &d_pos, &d_lat)) != RN_OK ||
      (rc = upload(s.w, vw.data(), vw.size())) != RN_OK)
    return rc;
  g_timer.reset();
  rc = mode_vdos_on_device(s, d_pos, d_lat, num_lattices != 1, K3, M, Q, average, densities);
  g_timer.collect();
  return rc;
}

}  // namespace

extern "C" int rn_md_mode_vdos(const double *positions, const double *lattices, int64_t num_lattices, int64_t S,
                               int32_t N, const double *masses, const double *vectors, int32_t M,
                               int64_t segment_steps, const int64_t *starts, int64_t Q, const double *taper,
                               int average, int device, size_t workspace_limit, double *densities, int64_t num_bins) {
  return md_mode_vdos(Source::host(positions), Source::host(lattices), num_lattices, S, N, masses, vectors, M,
                      segment_steps, starts, Q, taper, average, device, workspace_limit, densities, num_bins);
}

extern "C" int rn_md_mode_vdos_device(const double *d_positions, const double *d_lattices, int64_t num_lattices,
                                      int64_t S, int32_t N, const double *masses, const double *vectors, int32_t M,
                                      int64_t segment_steps, const int64_t *starts, int64_t Q, const double *taper,
                                      int average, int device, size_t workspace_limit, double *densities,
                                      int64_t num_bins, void *stream) {
  return md_mode_vdos(Source::device(d_positions, stream), Source::device(d_lattices, stream), num_lattices, S, N,
                      masses, vectors, M, segment_steps, starts, Q, taper, average, device, workspace_limit, densities,
                      num_bins);
}

extern "C" int rn_md_mode_vdos_set_profiling(int enabled) {
  return g_timer.set_profiling(g_mode_cache.mutex, enabled);
}

extern "C" int rn_md_mode_vdos_phase_times(double *millis) { return g_timer.phase_times(g_mode_cache.mutex, millis); }
