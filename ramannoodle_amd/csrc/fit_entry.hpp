// What the entries of the two window fits share (lineshape.hip, peakfit.hip): the arguments they have in common, the
// checks of the sizes and of the fit table, the device workspace with its staging, and the way results come back.
//
// The table (row_index, first_bin, num_bins, each [F]) and the results are host arrays; they and, for the host entry,
// the rows pass through grow-only device buffers.  Copies and the kernel are enqueued on the caller's stream (the host
// entry: the null stream), and the entry returns after synchronising it once, also after a failure.
// An entry checks in this order: check_sizes, its own scalars, F = 0 (RN_OK, nothing is touched), null pointers, then
// per fit check_row, its own least number of bins, check_window and whatever else it asks of a fit.
#pragma once
#include "entry_runtime.hpp"

namespace rn_fit {

using rn_spectrum::DeviceBuffer;
using rn_spectrum::ErrorText;
using rn_spectrum::FirstError;
using rn_spectrum::Fit;
using rn_spectrum::Workspace;

struct FitArgs {
  const double *rows;  // [num_rows][bins]: host, or HBM written by work on `stream`
  bool rows_on_host;
  int64_t num_rows, bins;
  const int64_t *row_index, *first_bin, *num_bins;
  int64_t F;
  int max_iterations;
  double *out;  // [F][outputs]
  int32_t *status, *iterations;
  hipStream_t stream;
  bool any_null() const { return !rows || !row_index || !first_bin || !num_bins || !out || !status || !iterations; }
};

inline int check_sizes(const FitArgs &a, ErrorText &error) {
  if (a.F < 0) return error.fail(RN_ERR_INVALID_ARGUMENT, "F = %lld is negative", (long long)a.F);
  if (a.max_iterations < 1)
    return error.fail(RN_ERR_INVALID_ARGUMENT, "max_iterations = %d is not positive", a.max_iterations);
  if (a.num_rows < 1 || a.bins < 1 || a.bins > INT32_MAX || a.F > ((int64_t)1 << 30))
    return error.fail(RN_ERR_INVALID_ARGUMENT, "num_rows = %lld, bins = %lld or F = %lld is out of range",
                      (long long)a.num_rows, (long long)a.bins, (long long)a.F);
  return RN_OK;
}

inline int check_row(const FitArgs &a, int64_t f, ErrorText &error) {
  if (a.row_index[f] < 0 || a.row_index[f] >= a.num_rows)
    return error.fail(RN_ERR_INVALID_ARGUMENT, "fit %lld: row %lld is outside [0, %lld)", (long long)f,
                      (long long)a.row_index[f], (long long)a.num_rows);
  return RN_OK;
}

inline int check_window(const FitArgs &a, int64_t f, ErrorText &error) {
  if (a.first_bin[f] < 0 || a.first_bin[f] > a.bins || a.num_bins[f] > a.bins - a.first_bin[f])
    return error.fail(RN_ERR_INVALID_ARGUMENT, "fit %lld: bins [%lld, %lld + %lld) are outside [0, %lld)", (long long)f,
                      (long long)a.first_bin[f], (long long)a.first_bin[f], (long long)a.num_bins[f], (long long)a.bins);
  return RN_OK;
}

inline unsigned fit_blocks(int64_t F, int waves) { return (unsigned)((F + waves - 1) / waves); }  // a wave per fit

// The workspace of one of the two modules, with `outputs` doubles per fit; `own` are the module's further buffers.
struct FitWorkspace : Workspace {
  const int outputs;
  DeviceBuffer rows, table, out, flags;  // the host entry's rows; the table [3][F]; out [F][outputs]; status, iterations
  explicit FitWorkspace(int outputs, std::initializer_list<DeviceBuffer *> own = {})
      : Workspace{&rows, &table, &out, &flags}, outputs(outputs) {
    buffers.insert(buffers.end(), own);
  }
  int64_t *column(const FitArgs &a, int i) const { return table.as<int64_t>() + i * a.F; }  // 0 .. 2, as in FitArgs
  double *d_out() const { return out.as<double>(); }
  int32_t *d_status() const { return flags.as<int32_t>(); }
  int32_t *d_iterations(const FitArgs &a) const { return flags.as<int32_t>() + a.F; }

  int ensure(const FitArgs &a) {
    const size_t count = (size_t)a.F;
    if ((a.rows_on_host && rows.ensure(row_bytes(a), Fit::kGrowOnly) != RN_OK) ||
        table.ensure(3 * count * sizeof(int64_t), Fit::kGrowOnly) != RN_OK ||
        out.ensure(count * outputs * sizeof(double), Fit::kGrowOnly) != RN_OK ||
        flags.ensure(2 * count * sizeof(int32_t), Fit::kGrowOnly) != RN_OK)
      return RN_ERR_OUT_OF_MEMORY;
    return RN_OK;
  }
  static int no_memory(const FitArgs &a, ErrorText &error) {
    return error.fail(RN_ERR_OUT_OF_MEMORY, "no device memory for %lld fits of %lld rows of %lld bins", (long long)a.F,
                      (long long)a.num_rows, (long long)a.bins);
  }
  // enqueues the copies of the rows (host entry) and of the table; the rows on the device
  const double *stage(const FitArgs &a, FirstError &ok) {
    const size_t column_bytes = (size_t)a.F * sizeof(int64_t);
    const double *d_rows = a.rows;
    if (a.rows_on_host) {
      ok(hipMemcpyAsync(rows.ptr, a.rows, row_bytes(a), hipMemcpyHostToDevice, a.stream));
      d_rows = rows.as<const double>();
    }
    ok(hipMemcpyAsync(column(a, 0), a.row_index, column_bytes, hipMemcpyHostToDevice, a.stream));
    ok(hipMemcpyAsync(column(a, 1), a.first_bin, column_bytes, hipMemcpyHostToDevice, a.stream));
    ok(hipMemcpyAsync(column(a, 2), a.num_bins, column_bytes, hipMemcpyHostToDevice, a.stream));
    return d_rows;
  }
  // enqueues the copies of the results, waits for the stream and returns the status of the call
  int finish(const FitArgs &a, FirstError &ok, ErrorText &error) {
    const size_t count = (size_t)a.F;
    ok(hipMemcpyAsync(a.out, out.ptr, count * outputs * sizeof(double), hipMemcpyDeviceToHost, a.stream));
    ok(hipMemcpyAsync(a.status, d_status(), count * sizeof(int32_t), hipMemcpyDeviceToHost, a.stream));
    ok(hipMemcpyAsync(a.iterations, d_iterations(a), count * sizeof(int32_t), hipMemcpyDeviceToHost, a.stream));
    const hipError_t waited = hipStreamSynchronize(a.stream);  // (also after a failure: the buffers may be in use)
    ok(waited);
    if (ok.first != hipSuccess) return error.fail(RN_ERR_HIP, "%s", hipGetErrorString(ok.first));
    return RN_OK;
  }

 private:
  static size_t row_bytes(const FitArgs &a) { return (size_t)a.num_rows * (size_t)a.bins * sizeof(double); }
};

}  // namespace rn_fit
