"""Lorentzian line-shape fits on the GPU (``csrc/lineshape.hip``) against the host statement
(``lineshape.fit_lorentzians_host``): window sizes around a wave and around the on-chip capacity, tables that end inside a
workgroup, degenerate fits among good ones, determinism, the device-pointer entry and its stream order, and
``fit_peaks`` of the device-resident mode-VDOS classes."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from ramannoodle_amd import _lib
from ramannoodle_amd.lineshape import (_fit_window, fit_lorentzians, fit_lorentzians_host, mode_windows,
                                       window_capacity)
from ramannoodle_amd.spectrum import (DeviceModeVibrationalDensityOfStates,
                                      DeviceModeVibrationalDensityOfStatesEnsemble)
from tests.lineshape_cases import axis, fits_deviation, lorentzian, noisy_family, relative_deviation, window
from tests.test_lineshape import FIELDS, _assert_same, peak_arguments, small_trajectory
from tests.test_polarized_spectra_gpu import _sleep_cycles

pytestmark = pytest.mark.gpu

# The noisy family, device minus host on the relative measure.  Measured on the MI355X on the 210 rows of
# test_noisy_family_against_the_host_statement: 9.559e-9 at worst, 4.7e-9 at the 99th percentile
# (profiles/lineshape_fit.txt).  The bound is 20 x the worst, for the reordering of the sums and the fused multiply-adds
# of the kernel; a deviation above 1e-6 would mean that the kernel departs from the recipe.
NOISY_MEASURED = 9.559e-9
NOISY_BOUND = 20.0 * NOISY_MEASURED


def _raw_device_fits(rows, row_index, first_bin, num_bins, max_iterations=400):
    """``rn_lineshape_fit`` itself: ``(out[F][8], status[F], iterations[F])`` in bin units."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    table = [np.ascontiguousarray(column, dtype=np.int64) for column in (row_index, first_bin, num_bins)]
    count = len(table[0])
    out = np.full((count, 8), -7.0)
    status, iterations = np.full(count, -7, dtype=np.int32), np.full(count, -7, dtype=np.int32)
    rc = _lib.load().rn_lineshape_fit(0, C.c_void_p(rows.ctypes.data), rows.shape[0], rows.shape[1],
                                      *(C.c_void_p(column.ctypes.data) for column in table), count, max_iterations,
                                      C.c_void_p(out.ctypes.data), C.c_void_p(status.ctypes.data),
                                      C.c_void_p(iterations.ctypes.data))
    assert rc == _lib.RN_OK, _lib.load().rn_lineshape_last_error()
    return out, status, iterations


@pytest.fixture(scope="module")
def noise_free():
    """Rows that are one Lorentzian each, so that every window around the peak is a noise-free fit, the distinct
    (row, first bin, bins) fits on them for the six window sizes, and the host statement of each, computed once."""
    capacity = window_capacity()
    sizes = (5, 63, 64, 65, capacity, capacity + 1)
    bins = capacity + 48
    rows, fits = [], []
    for k, n in enumerate(sizes):
        widest = max(0.6, n / 6.0)
        for j, g in enumerate((0.6, 0.5 * (0.6 + widest), widest)):
            centre = 0.5 * bins + (0.3, -0.2, 0.4)[j]
            h = 10.0 ** ((3 * k + j) % 9 - 4) * 1.37
            rows.append(lorentzian(bins, h, centre, g, (0.0, 0.1, 0.3)[j] * h))
            for offset in ((0,) if n == 5 else (-1, 0, 2)):  # overlapping windows of one row
                fits.append((len(rows) - 1, int(centre) - n // 2 + offset, n))
    rows = np.array(rows)
    host = [_fit_window(rows[r, first:first + n], 400) for r, first, n in fits]
    assert all(status == 0 for _, status, _ in host)
    return rows, np.array(fits), np.array([out for out, _, _ in host])


@pytest.mark.parametrize("count", [1, 5, 4097])
def test_noise_free_windows_against_the_host_statement(noise_free, count):
    """F = 1 and 5: fewer fits than a workgroup's waves, and a table that ends inside a workgroup (so does 4097)."""
    rows, fits, host = noise_free
    rng = np.random.default_rng(count)
    picks = np.concatenate([rng.permutation(len(fits)) for _ in range(count // len(fits) + 1)])[:count]
    if count == 5:
        picks = np.array([len(fits) - 1, 0, len(fits) - 10, 7, 20])  # the longest, the shortest, either side of capacity
    out, status, iterations = _raw_device_fits(rows, *fits[picks].T)
    np.testing.assert_array_equal(status, 0)
    assert iterations.min() >= 1
    want = host[picks]
    deviation = relative_deviation(*out[:, :4].T, *want[:, :4].T)
    print(f"noise-free, F = {count}: worst device-minus-host deviation {deviation.max():.3e}")
    assert deviation.max() <= 1e-10
    np.testing.assert_array_equal(out[:, 5], want[:, 5])            # the maximum
    np.testing.assert_allclose(out[:, 6:], want[:, 6:], rtol=1e-12)  # the moments


@pytest.fixture(scope="module")
def noisy():
    w, rows, windows, _, _ = noisy_family(210, seed=20261019)
    return w, rows, windows, fit_lorentzians_host(w, rows, windows)


def test_noisy_family_against_the_host_statement(noisy):
    w, rows, windows, host = noisy
    np.testing.assert_array_equal(host.status, 0)
    device = fit_lorentzians(w, rows, windows, device=0)
    np.testing.assert_array_equal(device.status, 0)
    deviation = fits_deviation(w, device, host)
    print(f"noisy family: worst device-minus-host deviation {deviation.max():.3e}, "
          f"99th percentile {np.percentile(deviation, 99):.3e}, most iterations {device.iterations.max()}")
    assert deviation.max() <= 1e-6, "the kernel departs from the recipe"
    assert deviation.max() <= NOISY_BOUND
    np.testing.assert_allclose(device.integral, host.integral, rtol=1e-12)
    np.testing.assert_allclose(device.centroid, host.centroid, rtol=1e-12)


def test_determinism_order_and_table_length(noisy):
    w, rows, windows, _ = noisy
    first = fit_lorentzians(w, rows, windows, device=0)
    _assert_same(fit_lorentzians(w, rows, windows, device=0), first)
    backwards = fit_lorentzians(w, rows[::-1], windows[::-1], device=0)
    prefix = fit_lorentzians(w, rows[:77], windows[:77], device=0)
    for name in FIELDS:
        np.testing.assert_array_equal(getattr(backwards, name)[::-1], getattr(first, name), err_msg=name)
        np.testing.assert_array_equal(getattr(prefix, name), getattr(first, name)[:77], err_msg=name)


@pytest.mark.parametrize("kind", ["nan", "zero", "flat"])
def test_degenerate_fits_leave_their_neighbours_alone(kind):
    """The degenerate window at every position of a four-fit workgroup (five fits: the table ends in the next one)."""
    w = axis(200)
    good = np.zeros((5, 200))
    for f in range(5):
        good[f, 20:20 + 129] = lorentzian(129, 3.0 + f, 60.3 + 2 * f, 4.0 + f, 0.2) * (1 + 0.01 * np.cos(np.arange(129)))
    one_window = window(w, 20, 129)
    clean = fit_lorentzians(w, good, one_window, device=0)
    np.testing.assert_array_equal(clean.status, 0)
    for place in range(4):
        rows = good.copy()
        if kind == "nan":
            rows[place, 20 + 70] = np.nan  # (lane 6's second bin)
        else:
            rows[place] = 0.0 if kind == "zero" else 2.5
        fits = fit_lorentzians(w, rows, one_window, device=0)
        others = np.arange(5) != place
        for name in FIELDS:
            np.testing.assert_array_equal(getattr(fits, name)[others], getattr(clean, name)[others], err_msg=name)
        for name in FIELDS[:-2]:
            assert np.isnan(getattr(fits, name)[place]), name
        assert fits.status[place] == 2 and fits.iterations[place] == 0
        np.testing.assert_array_equal(fits.status, fit_lorentzians_host(w, rows, one_window).status)


def test_iteration_limit_on_the_device():
    w, rows, windows, _, _ = noisy_family(7, seed=5)
    fits = fit_lorentzians(w, rows, windows, device=0, max_iterations=1)
    np.testing.assert_array_equal(fits.status, 1)
    np.testing.assert_array_equal(fits.iterations, 1)


def test_device_tensor_entry_is_the_host_array_entry(noisy):
    w, rows, windows, _ = noisy
    want = fit_lorentzians(w, rows, windows, device=0)
    tensor = torch.tensor(rows, device="cuda")
    _assert_same(fit_lorentzians(w, tensor, windows), want)
    _assert_same(fit_lorentzians(w, tensor, windows, device=0), want)
    peaks = fit_lorentzians(w, tensor[3], np.stack([windows[3], windows[3]]))  # (W,2) on one row of the tensor
    np.testing.assert_array_equal(peaks.position, want.position[3])
    with pytest.raises(ValueError, match="contiguous float64 CUDA tensor"):
        fit_lorentzians(w, tensor.float(), windows)
    with pytest.raises(ValueError, match="contiguous float64 CUDA tensor"):
        fit_lorentzians(w, tensor.cpu(), windows)


def test_waits_for_the_producer_stream(noisy):
    """The rows are written on a side stream behind a bounded sleep; the fit, called with that stream current, must
    see the finished rows (rows of zeros are degenerate: status 2)."""
    w, rows, windows, _ = noisy
    source = torch.tensor(rows, device="cuda")
    want = fit_lorentzians(w, source, windows)  # (also grows the workspace outside the window)
    target = torch.zeros_like(source)
    assert np.all(fit_lorentzians(w, target, windows).status == 2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit_lorentzians(w, source, windows)
    call_ms = 1e3 * (time.perf_counter() - t0)
    cycles = _sleep_cycles()
    side = torch.cuda.Stream()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        start.record()
        torch.cuda._sleep(cycles)
        end.record()
        target.copy_(source)
        got = fit_lorentzians(w, target, windows)
    torch.cuda.synchronize()
    slept = start.elapsed_time(end)
    assert slept <= 2000.0, f"the sleep held the stream {slept:.0f} ms"
    assert slept >= 10.0 * call_ms, f"the sleep held the stream {slept:.1f} ms, a call takes {call_ms:.2f} ms"
    _assert_same(got, want)


@pytest.mark.parametrize("ensemble", [False, True])
def test_fit_peaks_of_the_device_resident_classes(ensemble):
    positions, lattice, vectors, masses = small_trajectory()
    tensor = torch.tensor(positions, device="cuda")
    if ensemble:
        vdos = DeviceModeVibrationalDensityOfStatesEnsemble([tensor, tensor.flip(0).contiguous()], 2.0, lattice, vectors,
                                                            masses)
    else:
        vdos = DeviceModeVibrationalDensityOfStates(tensor, 2.0, lattice, vectors, masses)
    centres, half_width = peak_arguments(vdos.measure_segments(17)[0])
    for average in (True, False):
        w, rows = vdos.measure_segments(17, 6, "hann", average)
        got = vdos.fit_peaks(centres, half_width, segment_steps=17, hop=6, average=average)
        assert got.position.shape == rows.shape[:-1]
        windows = np.broadcast_to(mode_windows(centres, half_width), rows.shape[:-1] + (2,))
        _assert_same(got, fit_lorentzians(w, rows, windows, device=0))
        on_host = vdos.fit_peaks(centres, half_width, segment_steps=17, hop=6, average=average, host=True)
        w_host, rows_host = vdos.measure_segments(17, 6, "hann", average, host=True)
        _assert_same(on_host, fit_lorentzians_host(w_host, rows_host, windows))
