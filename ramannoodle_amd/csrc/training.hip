// One training step: the taped forward with batch-statistics BatchNorm, the parameter (and input) gradients, the running
// statistics and the device-resident Adam step -- through host buffers (float32 / float64) or with everything where it
// already is (float32).  Host only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "forward.hpp"

namespace rn {

// Sum `n` device doubles over the ranks of a data-parallel training run (no-op without a reducer).
void reduce_over_ranks(rn_potgnn *h, double *dev, size_t n, hipStream_t st) {
  if (!h->reducer) return;
  std::vector<double> host(n);
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipMemcpy(host.data(), dev, n * sizeof(double), hipMemcpyDeviceToHost));
  if (h->reducer(host.data(), (int64_t)n, h->reducer_ctx) != 0)
    throw HipError{hipErrorUnknown, "the statistics reducer (data-parallel training) failed"};
  HIP_TRY(hipMemcpy(dev, host.data(), n * sizeof(double), hipMemcpyHostToDevice));
}

// refresh `packed` (and the float64 copy, when it exists) from the device weights
void sync_host(rn_potgnn *h) {
  if (!h->host_stale) return;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h->packed.data(), h->f32.weights.p, h->packed.size() * sizeof(float), hipMemcpyDeviceToHost));
  h->host_stale = false;
  if (h->f64.ready) upload_weights<double>(h);
}

// ---- training: forward with batch-statistics BatchNorm, then parameter gradients (float32 for
// the product path; float64 for validating the reverse pass against float64 autograd)
// The taped forward + the training-mode readout (batch-statistics BatchNorm) over the S structures whose positions (and, per
// h->train_lat / h->train_types, lattices and atom types) sit in h->io_pos / io_lat / io_types; everything is enqueued on lane
// 0's stream, the standardised 6-vectors end up in h->io_vec6 / io_alpha and the batch statistics in P.mv.
template <typename T>
ForwardIO<T> train_io(rn_potgnn *h) {  // what the pending (or starting) train_forward runs with
  ForwardIO<T> io;
  io.pos = h->io_pos.as<double>();
  io.lat = h->train_lat ? h->io_lat.as<T>() : nullptr;
  io.types = h->train_types ? h->io_types.as<int>() : nullptr;
  return io;
}
template <typename T>
ChunkRun<T> train_forward_core(rn_potgnn *h, int S) {
  Precision<T> &P = prec<T>(h);
  const PackedLayout &L = h->lay;
  const Graph &g = h->g;
  const Dims d = h->d;
  const int HP = std::max(d.FeP, 32);
  ChunkRun<T> c = taped_forward<T>(h, train_io<T>(h), S);
  hipStream_t st = c.st();
  const int64_t R = (int64_t)S * g.E;
  T *Wd = P.weights.template as<T>();
  P.tape_z1.ensure((size_t)R * HP * sizeof(T));
  P.bn_stats.ensure(sizeof(double) * 6 * HP);  // forward sums (+ row count during the reduction) | backward sums | own copy
  DeviceBuf &mv = P.mv;
  mv.ensure(sizeof(T) * 2 * HP);
  const T *edgeP = P.tape_edge[h->cfg.num_message_passes].template as<T>();
  // z1 = edge W0^T + b0 ; h1 = ssp(BN_batch(z1)) ; then the rest of the readout as in eval
  launch_rowgemm<T>(edgeP, R, d.FeP, P.ro.W0T, HP, P.tape_z1.template as<T>(), nullptr, Wd + L.b0p, false, 0,
                    nullptr, g, st);
  {
    // batch statistics over every row of the batch -- of all ranks in a data-parallel run
    double *stats = P.bn_stats.template as<double>();
    launch_bn_col_sums<T>(P.tape_z1.template as<T>(), R, HP, stats, st);
    h->bn_count = (double)R;
    if (h->reducer) {
      const double rows = (double)R;  // slot 2HP is outside the range col_sums clears
      HIP_TRY(hipMemcpy(stats + 2 * HP, &rows, sizeof(double), hipMemcpyHostToDevice));
      reduce_over_ranks(h, stats, (size_t)2 * HP + 1, st);  // [sum z | sum z^2 | rows]
      HIP_TRY(hipMemcpy(&h->bn_count, stats + 2 * HP, sizeof(double), hipMemcpyDeviceToHost));
    }
    launch_bn_train_apply<T>(P.tape_z1.template as<T>(), R, HP, d.Fe, stats, h->bn_count, Wd + L.bn_w, Wd + L.bn_b,
                             c.bufA, mv.template as<T>(), st);
  }
  launch_rowgemm<T>(c.bufA, R, HP, P.ro.W3T, HP, c.bufB, P.ones, P.ro.b3, true, 0, nullptr, g, st);
  launch_rowgemm<T>(c.bufB, R, HP, P.ro.W5T, 32, c.bufA, nullptr, P.ro.b5, false, 0, nullptr, g, st);
  h->io_vec6.ensure((size_t)S * 6 * sizeof(float));
  h->io_alpha.ensure((size_t)S * 9 * sizeof(double));
  const double *ms = h->d_mean_std.as<double>();
  launch_readout_reduce<T>(c.bufA, c.unit4, S, g, ms, ms + 9, h->io_vec6.as<float>(), nullptr,
                           h->io_alpha.as<double>() /* standardised 3x3 in double */, st);
  HIP_TRY(hipGetLastError());
  return c;
}
// The kernels that rewrite the float32 weights on the device run on lane 0.  An evaluation that returned unfinished (the
// to-device entry, a device entry without synchronisation) may still read them on lane 1, whose last kernels of a lane pair
// are ordered behind nothing on lane 0: `st` waits for the other lanes' last evaluation first.
static void after_other_lanes(rn_potgnn *h, hipStream_t st) {
  for (auto &ln : h->f32.lanes)
    if (ln.stream.s && ln.stream.s != st && ln.done.e) HIP_TRY(hipStreamWaitEvent(st, ln.done.e, 0));
}

// running statistics where the weights live (torch: momentum 0.1, unbiased variance) and everything derived from them
static void train_running_stats(rn_potgnn *h, hipStream_t st) {
  Precision<float> &P = h->f32;
  const PackedLayout &L = h->lay;
  const Dims d = h->d;
  const int HP = std::max(d.FeP, 32);
  float *Wd = P.weights.as<float>();
  const double rows = h->bn_count;
  after_other_lanes(h, st);
  launch_bn_running(Wd + L.bn_rm, Wd + L.bn_rv, P.mv.as<float>(), P.mv.as<float>() + HP, d.Fe, 0.1,
                    rows / std::max(rows - 1.0, 1.0), st);
  device_setup<float>(h, Wd, st);
  h->host_stale = true;
}

// The forward of a training step, enqueued on lane 0 (returned): the taped forward and the training-mode readout over S
// structures.  `dev` null: the host entry has staged positions, lattices and atom types into io_pos / io_lat / io_types;
// else they are device arrays and are copied there on the lane's stream (the reverse pass reads the positions again).
struct DeviceBatch {
  const double *pos;     // [S][N][3]
  const float *lat;      // [S][9] or null
  const int32_t *types;  // [S][N] or null
};
template <typename T>
hipStream_t train_forward_enqueue(rn_potgnn *h, int S, bool lat, bool types, const DeviceBatch *dev) {
  hipStream_t st = prec<T>(h).lanes[0].stream.get();
  auto bring = [&](DeviceBuf &to, const void *from, size_t bytes) {
    if (!from) return;
    to.ensure(bytes);
    HIP_TRY(hipMemcpyAsync(to.p, from, bytes, hipMemcpyDeviceToDevice, st));
  };
  if (dev) {
    bring(h->io_pos, dev->pos, (size_t)S * h->g.N * 3 * sizeof(double));
    bring(h->io_lat, dev->lat, (size_t)S * 9 * sizeof(float));
    bring(h->io_types, dev->types, (size_t)S * h->g.N * sizeof(int32_t));
  }
  h->train_lat = lat;
  h->train_types = types;
  (void)train_forward_core<T>(h, S);
  return st;
}

// Through host buffers: stage, enqueue, synchronise, copy out.
template <typename T>
void train_forward(rn_potgnn *h, const double *host_pos, int S, T *vec6, T *batch_mean, T *batch_var, const double *host_lat,
                   const int32_t *host_types) {
  ensure_precision<T>(h);
  const int Fe = h->d.Fe, HP = std::max(h->d.FeP, 32);
  stage<double>(h->io_pos, host_pos, (size_t)S * h->g.N * 3 * sizeof(double));
  // per-sample lattices (in the arithmetic of the run, as the reference's forward casts them) and atom types: the graph
  // topology stays the reference structure's (_gnn.py:603-611, 541-557)
  stage_lattices<T>(h, host_lat, S);
  stage_types(h, host_types, S);
  hipStream_t st = train_forward_enqueue<T>(h, S, host_lat != nullptr, host_types != nullptr, nullptr);
  HIP_TRY(hipStreamSynchronize(st));
  check_ps_fail(h);
  if constexpr (sizeof(T) == 4) {
    HIP_TRY(hipMemcpy(vec6, h->io_vec6.p, (size_t)S * 6 * sizeof(float), hipMemcpyDeviceToHost));
    if (h->device_training) {
      train_running_stats(h, st);
      HIP_TRY(hipStreamSynchronize(st));
    }
  } else {  // the standardised tensor, at full precision
    std::vector<double> raw((size_t)S * 9);
    HIP_TRY(hipMemcpy(raw.data(), h->io_alpha.p, raw.size() * sizeof(double), hipMemcpyDeviceToHost));
    pick_vec6(raw.data(), S, vec6);
  }
  std::vector<T> mvh(2 * HP);
  HIP_TRY(hipMemcpy(mvh.data(), prec<T>(h).mv.p, sizeof(T) * 2 * HP, hipMemcpyDeviceToHost));
  for (int k = 0; k < Fe; ++k) {
    batch_mean[k] = mvh[k];
    batch_var[k] = mvh[HP + k];
  }
  h->train_S = S;
  h->train_prec = (int)sizeof(T);
}

// The same step with everything where it already is (device-resident training, float32): positions [S][N][3] float64,
// optional lattices [S][9] float32 and atom types [S][N] int32, and the [S][6] result are DEVICE buffers; work is ordered
// after `user` and `user` is made to wait for it; no host round trip, no synchronisation.
void train_forward_device(rn_potgnn *h, const double *d_pos, int S, const float *d_lat, const int32_t *d_types, float *d_vec6,
                          hipStream_t user) {
  ensure_precision<float>(h);
  behind_caller(h, user, h->f32.lanes, 1);
  const DeviceBatch dev{d_pos, d_lat, d_types};
  hipStream_t st = train_forward_enqueue<float>(h, S, d_lat != nullptr, d_types != nullptr, &dev);
  HIP_TRY(hipMemcpyAsync(d_vec6, h->io_vec6.p, (size_t)S * 6 * sizeof(float), hipMemcpyDeviceToDevice, st));
  train_running_stats(h, st);
  hand_back(h, user, h->f32.lanes, 1, false);
  h->train_S = S;
  h->train_prec = 4;
}

template <typename T>
static int pending_frames(rn_potgnn *h) {
  if (h->train_S <= 0 || h->train_prec != (int)sizeof(T))
    throw HipError{hipErrorInvalidValue, "train_backward without a train_forward of the same precision"};
  return h->train_S;
}

// The reverse pass of the pending train_forward, enqueued on lane 0 (returned): parameter gradients into P.grad and, where
// asked for, input gradients into the device arrays d_dpos / d_dlat.  The cotangents [S][6] are a host array (staged with
// a blocking copy) or, `on_device`, a device array.
template <typename T>
hipStream_t train_backward_enqueue(rn_potgnn *h, int S, const T *dvec6, bool on_device, double *d_dpos, double *d_dlat) {
  Precision<T> &P = prec<T>(h);
  ChunkRun<T> c(h, P.lanes[0], train_io<T>(h), S);
  hipStream_t st = c.st();
  const size_t seed_bytes = (size_t)S * 6 * sizeof(T);
  if (on_device) {
    P.seeds.ensure(seed_bytes);
    HIP_TRY(hipMemcpyAsync(P.seeds.p, dvec6, seed_bytes, hipMemcpyDeviceToDevice, st));
  } else {
    stage<T>(P.seeds, dvec6, seed_bytes);
  }
  P.grad.ensure(h->lay.total * sizeof(T));
  HIP_TRY(hipMemsetAsync(P.grad.p, 0, h->lay.total * sizeof(T), st));
  Reverse<T> rv{S, 1, P.seeds.template as<T>(), nullptr, P.grad.template as<T>(), true};
  rv.in_dpos = d_dpos;  // (input gradients, when asked for, from the same reverse pass)
  rv.in_dlat = d_dlat;
  reverse_pass<T>(h, c, rv);
  return st;
}

template <typename T>
void train_backward(rn_potgnn *h, const T *dvec6, T *grads, double *host_dpos, double *host_dlat) {
  Precision<T> &P = prec<T>(h);
  const int S = pending_frames<T>(h);
  const size_t npos = (size_t)S * h->g.N * 3;
  double *d_dpos = nullptr, *d_dlat = nullptr;
  if (host_dpos || host_dlat) {  // device scratch for the host outputs, copied out below
    P.in_grads.ensure((npos + (size_t)S * 9) * sizeof(double));
    d_dpos = host_dpos ? P.in_grads.template as<double>() : nullptr;
    d_dlat = host_dlat ? P.in_grads.template as<double>() + npos : nullptr;
  }
  hipStream_t st = train_backward_enqueue<T>(h, S, dvec6, false, d_dpos, d_dlat);
  HIP_TRY(hipStreamSynchronize(st));
  h->train_S = 0;  // (the pending forward is consumed whether or not the check below throws)
  check_ps_fail(h);
  if (host_dpos) HIP_TRY(hipMemcpy(host_dpos, d_dpos, npos * sizeof(double), hipMemcpyDeviceToHost));
  if (host_dlat) HIP_TRY(hipMemcpy(host_dlat, d_dlat, (size_t)S * 9 * sizeof(double), hipMemcpyDeviceToHost));
  if (sizeof(T) == 4) h->grads_on_device = true;
  if (!grads) return;
  std::vector<T> gp(h->lay.total);
  HIP_TRY(hipMemcpy(gp.data(), P.grad.p, gp.size() * sizeof(T), hipMemcpyDeviceToHost));
  unpack_weights<T>(h->lay, gp.data(), grads, false);
}

// With the cotangents [S][6] in a DEVICE buffer: the gradients stay in HBM (device-resident training), nothing is
// synchronised: `user` waits for the lane, the Adam step runs on the lane's stream.
void train_backward_device(rn_potgnn *h, const float *d_dvec6, hipStream_t user, double *d_dpos, double *d_dlat) {
  const int S = pending_frames<float>(h);
  behind_caller(h, user, h->f32.lanes, 1);
  (void)train_backward_enqueue<float>(h, S, d_dvec6, true, d_dpos, d_dlat);
  hand_back(h, user, h->f32.lanes, 1, false);
  h->train_S = 0;
  h->grads_on_device = true;
}

// One Adam step on the device weights from the gradients of the last backward, on lane 0; the host mirror of what the
// host looks at afterwards is refreshed with one download.
void adam_step(rn_potgnn *h, double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step) {
  Precision<float> &P = h->f32;
  const PackedLayout &L = h->lay;
  const size_t n = L.total;
  hipStream_t st = P.lanes[0].stream.get();
  if (!h->trainable_mask.p) {  // first step: moments, mask and the table of derived ranges
    h->adam_m.ensure(n * sizeof(float));
    h->adam_v.ensure(n * sizeof(float));
    HIP_TRY(hipMemset(h->adam_m.p, 0, n * sizeof(float)));
    HIP_TRY(hipMemset(h->adam_v.p, 0, n * sizeof(float)));
    const std::vector<unsigned char> mask = trainable_mask(L);
    h->trainable_mask.ensure(mask.size());
    HIP_TRY(hipMemcpy(h->trainable_mask.p, mask.data(), mask.size(), hipMemcpyHostToDevice));
    const std::vector<DerivedOp> ops = derived_ops(L, &h->derived_first_stage);
    h->derived_ops.ensure(ops.size() * sizeof(DerivedOp));
    HIP_TRY(hipMemcpy(h->derived_ops.p, ops.data(), ops.size() * sizeof(DerivedOp), hipMemcpyHostToDevice));
    h->num_derived_ops = (int)ops.size();
  }
  float *w = P.weights.as<float>();
  after_other_lanes(h, st);
  launch_adam(w, P.grad.as<float>(), h->adam_m.as<float>(), h->adam_v.as<float>(),
              h->trainable_mask.as<unsigned char>(), n, lr, beta1, beta2, eps, weight_decay, step, st,
              (h->plan.use_ps && h->ps_fail.p) ? h->ps_fail.as<int>() : nullptr);
  launch_refresh_derived(w, h->derived_ops.as<DerivedOp>(), h->derived_first_stage, st);
  launch_refresh_derived(w, h->derived_ops.as<DerivedOp>() + h->derived_first_stage, h->num_derived_ops - h->derived_first_stage, st);
  device_setup<float>(h, w, st);
  HIP_TRY(hipGetLastError());
  // The host looks at three kinds of entries after a step: c3_norm_1's folded constants (the triplet loop's folded-scale
  // variant is chosen from them), the prescale pairs (which double as the finiteness flags of the weight blocks,
  // mfma_f16_range_ok) and the readout block of the split-f16 range guard.  One gather kernel + ONE download into pinned
  // memory (2 P + 1 separate small downloads cost a round trip each: 0.2 ms of a 0.3 ms step).
  {
    std::vector<long long> seg;
    long long total = 0;
    auto add = [&](Span s) {
      seg.push_back((long long)s.begin);
      seg.push_back(total);
      seg.push_back((long long)s.count);
      total += (long long)s.count;
    };
    for (int p = 0; p < L.P; ++p) {
      add(L.c3_norm_1(p));    // the folded-gate criterion reads gamma and beta
      add(L.mfma_scales(p));  // the prescale pairs double as finiteness flags
    }
    add(L.readout());
    if (h->step_seg.bytes < seg.size() * sizeof(long long)) {
      h->step_seg.ensure(seg.size() * sizeof(long long));
      HIP_TRY(hipMemcpy(h->step_seg.p, seg.data(), seg.size() * sizeof(long long), hipMemcpyHostToDevice));
      h->step_stage.ensure((size_t)total * sizeof(float));
      h->step_host.ensure((size_t)total * sizeof(float));
    }
    launch_gather_segments(w, h->step_seg.as<long long>(), (int)(seg.size() / 3), h->step_stage.as<float>(), st);
    HIP_TRY(hipMemcpyAsync(h->step_host.p, h->step_stage.p, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t i = 0; i < seg.size(); i += 3)
      std::memcpy(h->packed.data() + seg[i], h->step_host.as<float>() + seg[i + 1], (size_t)seg[i + 2] * sizeof(float));
  }
  HIP_TRY(hipStreamSynchronize(st));
  // The taped forward of this step ran the role-specialised EdgeBlock and nothing has looked at its time-out word since.  If it
  // is set the Adam kernel has applied nothing (it reads the same word), so weights, moments and the host mirror are those of
  // before the step; the gradients are void either way and the handle says so before the error leaves.
  h->grads_on_device = false;
  h->train_S = 0;
  h->host_stale = true;
  refresh_pass_flags<float>(h);
  refresh_mfma_mode(h);
  check_ps_fail(h);
}

#define RN_TRAINING_INSTANCES(T)                                                                              \
  template void train_forward<T>(rn_potgnn *, const double *, int, T *, T *, T *, const double *, const int32_t *); \
  template void train_backward<T>(rn_potgnn *, const T *, T *, double *, double *);
RN_TRAINING_INSTANCES(float)
RN_TRAINING_INSTANCES(double)

}  // namespace rn
