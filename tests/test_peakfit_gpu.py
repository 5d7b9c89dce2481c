"""Multi-peak fits on the GPU (``csrc/peakfit.hip``) against the host statement (``peakfit.fit_peaks_host``): every
instantiation of the kernel on window sizes around a wave and around the on-chip capacity, tables that end inside a
workgroup, noisy rows, determinism, degenerate fits among good ones, the device-pointer entry and its stream order, and
``fit_peaks_multi`` on the rows of ``measure_segments``."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from ramannoodle_amd import _lib
from ramannoodle_amd.peakfit import OUTPUTS, _fit_window, fit_peaks_host, fit_peaks_multi, window_capacity
from ramannoodle_amd.spectrum import ModeVibrationalDensityOfStates
from tests.lineshape_cases import SPACING, window
from tests.peakfit_cases import (BASELINES, SHAPES, axis_from, errors_deviation, fits_deviation, model,
                                 noise_free_family, noisy_family, num_parameters)
from tests.test_peakfit import FIELDS, _assert_same
from tests.test_polarized_spectra_gpu import _sleep_cycles

pytestmark = pytest.mark.gpu

# The noisy family, device minus host, measured on the MI355X on the 210 rows of
# test_noisy_family_against_the_host_statement (profiles/peak_fits.txt): the parameters on the relative measure of
# peakfit_cases.fits_deviation (worst 4.558e-9 for P = 2, 99th percentile 2.9e-9; 1.010e-8 for P = 4, 99th percentile
# 7.8e-9) and the standard errors relative to themselves (4.750e-9 and 1.088e-8).  The bounds are 20 x the worst, for the
# instruction's order of the sums and the fused multiply-adds of the kernel; a deviation above 1e-6 would mean that the
# kernel departs from the recipe.
NOISY_MEASURED = {2: 4.558e-9, 4: 1.010e-8}
NOISY_ERRORS_MEASURED = {2: 4.750e-9, 4: 1.088e-8}
CEILING = 1e-6


def _raw_device_fits(rows, row_index, first_bin, num_bins, origin, centres, widths, dho, linear, max_iterations=400):
    """``rn_peakfit_fit`` itself: ``(out[F][32], status[F], iterations[F])`` in bin units."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    table = [np.ascontiguousarray(column, dtype=np.int64) for column in (row_index, first_bin, num_bins)]
    real = [np.ascontiguousarray(column, dtype=np.float64) for column in (origin, centres, widths)]
    count = len(table[0])
    out = np.full((count, OUTPUTS), -7.0)
    status, iterations = np.full(count, -7, dtype=np.int32), np.full(count, -7, dtype=np.int32)
    rc = _lib.load().rn_peakfit_fit(0, C.c_void_p(rows.ctypes.data), rows.shape[0], rows.shape[1],
                                    *(C.c_void_p(column.ctypes.data) for column in table), count, int(dho), int(linear),
                                    real[1].shape[1], *(C.c_void_p(column.ctypes.data) for column in real),
                                    max_iterations, C.c_void_p(out.ctypes.data), C.c_void_p(status.ctypes.data),
                                    C.c_void_p(iterations.ctypes.data))
    assert rc == _lib.RN_OK, _lib.load().rn_peakfit_last_error()
    return out, status, iterations


_NOISE_FREE = {}


def noise_free(peaks, shape, baseline):
    """The noise-free family at the six window sizes, two seeds each, as the table of the C entry, and the host
    statement of each fit, computed once: ``(rows, table columns.., host out[F][32])``."""
    key = (peaks, shape, baseline)
    if key not in _NOISE_FREE:
        capacity = window_capacity()
        p = num_parameters(peaks, baseline)
        sizes = (p + 2, 63, 64, 65, capacity, capacity + 1)
        origin = 40.0 if shape == "dho" else 2048.0
        w, rows, _, first, centres, _, _ = noise_free_family(peaks, sizes, 2, shape, baseline, origin)
        n = np.repeat(sizes, 2)
        in_bins = (centres - w[first][:, None]) / SPACING
        widths = np.repeat((n / (8.0 * peaks))[:, None], peaks, axis=1)
        host = [_fit_window(rows[f, first[f]:first[f] + n[f]], origin + first[f], in_bins[f], widths[f], shape == "dho",
                            baseline == "linear", 400) for f in range(len(rows))]
        assert all(status == 0 for _, status, _ in host)
        _NOISE_FREE[key] = (rows, np.arange(len(rows)), first, n, origin + first, in_bins, widths,
                            np.array([out for out, _, _ in host]))
    return _NOISE_FREE[key]


def raw_deviation(out, want, peaks, linear, n):
    """The relative measure on raw outputs: per peak heights over the height, positions and widths over the width; the
    baseline and ``n`` x the slope over the smallest height."""
    h, x0, g = (want[:, k:3 * peaks:3] for k in range(3))
    dh, dx0, dg = (np.abs(out[:, k:3 * peaks:3] - want[:, k:3 * peaks:3]) for k in range(3))
    worst = np.max([dh / h, dx0 / g, dg / g], axis=0).max(axis=1)
    smallest = h.min(axis=1)
    worst = np.maximum(worst, np.abs(out[:, 3 * peaks] - want[:, 3 * peaks]) / smallest)
    if linear:
        worst = np.maximum(worst, np.abs(out[:, 3 * peaks + 1] - want[:, 3 * peaks + 1]) * n / smallest)
    return worst


@pytest.mark.parametrize("count", [1, 5, 4097])
@pytest.mark.parametrize("baseline", BASELINES)
@pytest.mark.parametrize("shape", SHAPES)
def test_noise_free_windows_against_the_host_statement(shape, baseline, count):
    """n = p + 2, 63, 64, 65, capacity and capacity + 1 for one to four peaks.  F = 1 and 5: fewer fits than a
    workgroup's waves, and a table that ends inside a workgroup (so does 4097)."""
    for peaks in (1, 2, 3, 4):
        rows, row_index, first, n, origin, centres, widths, host = noise_free(peaks, shape, baseline)
        rng = np.random.default_rng(count + peaks)
        picks = np.concatenate([rng.permutation(len(rows)) for _ in range(count // len(rows) + 1)])[:count]
        if count == 5:
            picks = np.array([len(rows) - 1, 0, len(rows) - 3, 5, 7])  # capacity + 1, p + 2, capacity, 64, 65
        out, status, iterations = _raw_device_fits(rows, row_index[picks], first[picks], n[picks], origin[picks],
                                                   centres[picks], widths[picks], shape == "dho", baseline == "linear")
        np.testing.assert_array_equal(status, 0)
        assert iterations.min() >= 1
        want = host[picks]
        p = num_parameters(peaks, baseline)
        deviation = raw_deviation(out, want, peaks, baseline == "linear", n[picks])
        print(f"noise-free {shape} {baseline} P = {peaks}, F = {count}: worst device-minus-host deviation "
              f"{deviation.max():.3e}")
        assert deviation.max() <= 1e-10
        assert np.all(np.isnan(out[:, p:14])) and np.all(np.isnan(out[:, 14 + p:28]))  # the unused slots
        assert np.all(np.isfinite(out[:, 14:14 + p])) and np.all(out[:, 28] <= 1e-20)
        np.testing.assert_array_equal(out[:, 29], want[:, 29])            # the maximum
        np.testing.assert_allclose(out[:, 30:], want[:, 30:], rtol=1e-12)  # the moments


@pytest.fixture(scope="module", params=[2, 4])
def noisy(request):
    peaks = request.param
    w, rows, windows, _, centres = noisy_family(210, peaks, seed=20261021 + peaks)
    return peaks, w, rows, windows, centres, fit_peaks_host(w, rows, windows, centres)


def test_noisy_family_against_the_host_statement(noisy):
    peaks, w, rows, windows, centres, host = noisy
    np.testing.assert_array_equal(host.status, 0)
    device = fit_peaks_multi(w, rows, windows, centres, device=0)
    np.testing.assert_array_equal(device.status, 0)
    deviation = fits_deviation(device, host)
    errors = errors_deviation(device, host)
    print(f"noisy family, P = {peaks}: worst device-minus-host deviation {deviation.max():.3e} "
          f"(99th percentile {np.percentile(deviation, 99):.3e}), of the standard errors {errors.max():.3e} "
          f"(99th percentile {np.percentile(errors, 99):.3e}), most iterations {device.iterations.max()}")
    assert deviation.max() <= CEILING and errors.max() <= CEILING, "the kernel departs from the recipe"
    assert deviation.max() <= 20.0 * NOISY_MEASURED[peaks]
    assert errors.max() <= 20.0 * NOISY_ERRORS_MEASURED[peaks]
    np.testing.assert_allclose(device.rss, host.rss, rtol=1e-9)
    np.testing.assert_allclose(device.integral, host.integral, rtol=1e-12)
    np.testing.assert_allclose(device.centroid, host.centroid, rtol=1e-12)


def test_determinism_order_and_table_length(noisy):
    _, w, rows, windows, centres, _ = noisy
    first = fit_peaks_multi(w, rows, windows, centres, device=0)
    _assert_same(fit_peaks_multi(w, rows, windows, centres, device=0), first)
    backwards = fit_peaks_multi(w, rows[::-1], windows[::-1], centres[::-1], device=0)
    prefix = fit_peaks_multi(w, rows[:77], windows[:77], centres[:77], device=0)
    for name in FIELDS:
        np.testing.assert_array_equal(getattr(backwards, name)[::-1], getattr(first, name), err_msg=name)
        np.testing.assert_array_equal(getattr(prefix, name), getattr(first, name)[:77], err_msg=name)


@pytest.mark.parametrize("kind", ["nan", "zero", "flat"])
def test_degenerate_fits_leave_their_neighbours_alone(kind):
    """The degenerate window at every position of a four-fit workgroup (five fits: the table ends in the next one)."""
    w = axis_from(2048.0, 200)
    good = np.zeros((5, 200))
    for f in range(5):
        good[f, 20:20 + 129] = (model(129, [(3.0 + f, 50.3 + 2 * f, 4.0 + f), (2.0, 80.6 - f, 5.0)], 0.2, 0.0)
                                * (1 + 0.01 * np.cos(np.arange(129))))
    one_window = window(w, 20, 129)
    centres = w[20] + SPACING * np.array([50.0, 80.0])
    clean = fit_peaks_multi(w, good, one_window, centres, device=0)
    np.testing.assert_array_equal(clean.status, 0)
    for place in range(4):
        rows = good.copy()
        if kind == "nan":
            rows[place, 20 + 70] = np.nan  # (lane 6's second bin)
        else:
            rows[place] = 0.0 if kind == "zero" else 2.5
        fits = fit_peaks_multi(w, rows, one_window, centres, device=0)
        others = np.arange(5) != place
        for name in FIELDS:
            np.testing.assert_array_equal(getattr(fits, name)[others], getattr(clean, name)[others], err_msg=name)
        for name in FIELDS[:-2]:
            assert np.all(np.isnan(getattr(fits, name)[place])), name
        assert fits.status[place] == 2 and fits.iterations[place] == 0
        np.testing.assert_array_equal(fits.status, fit_peaks_host(w, rows, one_window, centres).status)


def test_iteration_limit_and_a_singular_curvature_on_the_device():
    """Status 1 after one solve; twins whose first step is refused keep columns that are equal bit for bit, so the
    elimination meets a pivot that is exactly zero and every error is NaN (test_peakfit.py has the reasoning)."""
    w, rows, windows, _, centres = noisy_family(7, 2, seed=5)
    fits = fit_peaks_multi(w, rows, windows, centres, device=0, max_iterations=1)
    np.testing.assert_array_equal(fits.status, 1)
    np.testing.assert_array_equal(fits.iterations, 1)
    row = np.zeros(64)
    row[10:43] = model(33, [(2.0, 11.3, 2.5), (1.2, 21.6, 3.0)], 0.25, 0.0)
    w = axis_from(2048.0, 64)
    arguments = (w, row, window(w, 10, 33), w[10] + SPACING * np.array([31.0, 31.0]))
    twins = fit_peaks_multi(*arguments, hwhm=1.5, device=0, max_iterations=1)
    host = fit_peaks_host(*arguments, hwhm=1.5, max_iterations=1)
    assert twins.status == 1 and host.status == 1
    for name in ("height_error", "position_error", "hwhm_error", "baseline_error"):
        assert np.all(np.isnan(getattr(twins, name))), name
    for name in ("height", "position", "hwhm", "baseline"):
        np.testing.assert_array_equal(getattr(twins, name), getattr(host, name), err_msg=name)
    np.testing.assert_allclose(twins.rss, host.rss, rtol=1e-12)


def test_device_tensor_entry_is_the_host_array_entry(noisy):
    _, w, rows, windows, centres, _ = noisy
    want = fit_peaks_multi(w, rows, windows, centres, device=0)
    tensor = torch.tensor(rows, device="cuda")
    _assert_same(fit_peaks_multi(w, tensor, windows, centres), want)
    _assert_same(fit_peaks_multi(w, tensor, windows, centres, device=0), want)
    peaks = fit_peaks_multi(w, tensor[3], np.stack([windows[3], windows[3]]), centres[3])  # (W,2) on one row
    np.testing.assert_array_equal(peaks.position, np.stack([want.position[3]] * 2))
    with pytest.raises(ValueError, match="contiguous float64 CUDA tensor"):
        fit_peaks_multi(w, tensor.float(), windows, centres)
    with pytest.raises(ValueError, match="contiguous float64 CUDA tensor"):
        fit_peaks_multi(w, tensor.cpu(), windows, centres)


def test_waits_for_the_producer_stream(noisy):
    """The rows are written on a side stream behind a bounded sleep; the fit, called with that stream current, must
    see the finished rows (rows of zeros are degenerate: status 2)."""
    _, w, rows, windows, centres, _ = noisy
    source = torch.tensor(rows, device="cuda")
    want = fit_peaks_multi(w, source, windows, centres)  # (also grows the workspace outside the window)
    target = torch.zeros_like(source)
    assert np.all(fit_peaks_multi(w, target, windows, centres).status == 2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit_peaks_multi(w, source, windows, centres)
    call_ms = 1e3 * (time.perf_counter() - t0)
    cycles = _sleep_cycles()
    side = torch.cuda.Stream()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        start.record()
        torch.cuda._sleep(cycles)
        end.record()
        target.copy_(source)
        got = fit_peaks_multi(w, target, windows, centres)
    torch.cuda.synchronize()
    slept = start.elapsed_time(end)
    assert slept <= 2000.0, f"the sleep held the stream {slept:.0f} ms"
    assert slept >= 10.0 * call_ms, f"the sleep held the stream {slept:.1f} ms, a call takes {call_ms:.2f} ms"
    _assert_same(got, want)


def two_mode_trajectory(frames=80, atoms=3, modes=4, seed=3):
    """Every atom moves with two frequencies, so every mode's VDOS row has two peaks: plumbing only, no physics."""
    rng = np.random.default_rng(seed)
    lattice = np.array([[5.0, 0.0, 0.0], [0.3, 5.2, 0.0], [0.0, -0.2, 4.9]])
    t = np.arange(frames)[:, None, None]
    phase = rng.uniform(0, 6.0, size=(2, 1, atoms, 3))
    positions = (rng.random((1, atoms, 3)) + 0.01 * np.cos(1.3 * t + phase[0]) + 0.007 * np.cos(2.1 * t + phase[1])
                 + 0.0005 * rng.normal(size=(frames, atoms, 3)))
    return positions, lattice, rng.normal(size=(modes, atoms, 3)), 1.0 + rng.random(atoms)


@pytest.mark.parametrize("shape", SHAPES)
def test_fit_peaks_multi_on_the_rows_of_measure_segments(shape):
    """The two-peak rows ``[modes][segments][19]`` of a small mode-VDOS: the device call has the shapes of the host call
    and agrees with it (these fits take some 200 iterations each, so the bound is the ceiling of the noisy family)."""
    positions, lattice, vectors, masses = two_mode_trajectory()
    vdos = ModeVibrationalDensityOfStates(positions, 2.0, lattice, vectors, masses)
    w, rows = vdos.measure_segments(41, 13, "hann", False)
    assert rows.ndim == 3 and len(w) == 19
    centres = w[[7, 12]]  # 1.3 and 2.1 rad per step on the 40-point grid, less the dropped zero bin
    whole = [w[0] - 1.0, w[-1] + 1.0]
    host = fit_peaks_multi(w, rows, whole, centres, shape=shape)
    device = fit_peaks_multi(w, rows, whole, centres, shape=shape, device=0)
    for name in FIELDS:
        assert getattr(device, name).shape == getattr(host, name).shape, name
    assert device.position.shape == rows.shape[:-1] + (2,) and device.rss.shape == rows.shape[:-1]
    np.testing.assert_array_equal(host.status, 0)
    np.testing.assert_array_equal(device.status, 0)
    deviation = fits_deviation(device, host)
    print(f"measure_segments rows, {shape}: worst device-minus-host deviation {deviation.max():.3e}, iterations "
          f"{device.iterations.min()} to {device.iterations.max()} (host {host.iterations.min()} to {host.iterations.max()})")
    assert deviation.max() <= CEILING
    on_tensor = fit_peaks_multi(w, torch.tensor(rows, device="cuda"), whole, centres, shape=shape)
    _assert_same(on_tensor, device)
