"""Multi-peak line-shape fits (``ramannoodle_amd.peakfit``): what needs no GPU.

The host statement ``fit_peaks_host`` against the truth of noise-free windows (both shapes, both baselines, one to four
peaks) and against scipy's least squares and its Jacobian on noisy ones, against the one-peak statement of ``lineshape``,
its exact scaling, shift and permutation properties, the status codes, every ``ValueError``, the C entry's refusals (they
come before the device is touched), the new symbols, and ``replicate_errors`` on a ``PeakFits``."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.optimize

from ramannoodle_amd import _lib
from ramannoodle_amd.lineshape import fit_lorentzians_host, replicate_errors, replicate_standard_error
from ramannoodle_amd.peakfit import (OUTPUTS, PeakErrors, PeakFits, _fit_window, _solve, fit_peaks_host,
                                     fit_peaks_multi)
from tests.lineshape_cases import SPACING, window
from tests.peakfit_cases import (BASELINES, axis_from, model, noise_free_family, noisy_family, num_parameters,
                                 peak_deviation, shape_values)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rn_peakfit_fit", "rn_peakfit_fit_device", "rn_peakfit_window_capacity", "rn_peakfit_last_error")
PER_PEAK = ("height", "position", "hwhm", "area", "height_error", "position_error", "hwhm_error")
PER_FIT = ("baseline", "slope", "baseline_error", "rss", "residual_variance", "integral", "centroid", "status",
           "iterations")
FIELDS = PER_PEAK + PER_FIT


def _assert_same(got, want):
    for name in FIELDS:
        np.testing.assert_array_equal(getattr(got, name), getattr(want, name), err_msg=name)


def _two_peak_row(bins=64, first=10, n=33, origin=2048.0):
    row = np.zeros(bins)
    row[first:first + n] = model(n, [(2.0, 11.3, 2.5), (1.2, 21.6, 3.0)], 0.25, 0.0)
    return axis_from(origin, bins), row, window(axis_from(origin, bins), first, n)


def _centres(w, first, in_bins):
    return w[first] + SPACING * np.asarray(in_bins, dtype=np.float64)


@pytest.mark.parametrize("baseline", BASELINES)
@pytest.mark.parametrize("shape,origin", [("lorentzian", 2048.0), ("dho", 5.0), ("dho", 40.0), ("dho", 2048.0)])
def test_noise_free_windows_recover_the_truth(shape, origin, baseline):
    """Bound 1e-10 on the relative measure per peak: the stop rule's step size, on a problem with zero residual.  One to
    four peaks, windows of p + 2, 33, 64, 65, 129 and 513 bins, 8 seeds each."""
    worst = 0.0
    for peaks in (1, 2, 3, 4):
        p = num_parameters(peaks, baseline)
        w, rows, windows, first, centres, truth, base = noise_free_family(peaks, (p + 2, 33, 64, 65, 129, 513), 8, shape,
                                                                          baseline, origin)
        fits = fit_peaks_host(w, rows, windows, centres, shape=shape, baseline=baseline)
        assert isinstance(fits, PeakFits) and fits.height.shape == (len(rows), peaks) and fits.rss.shape == (len(rows),)
        np.testing.assert_array_equal(fits.status, 0)
        deviation = peak_deviation(fits, w, first, truth)
        smallest = truth[..., 0].min(axis=1)
        n = np.repeat((p + 2, 33, 64, 65, 129, 513), 8)
        level = np.abs(fits.baseline - base[:, 0]) / smallest
        tilt = np.abs(fits.slope * SPACING - base[:, 1]) * n / smallest
        worst = max(worst, deviation.max(), level.max(), tilt.max())
        assert deviation.max() <= 1e-10 and level.max() <= 1e-10 and tilt.max() <= 1e-10, (peaks, deviation.max())
        np.testing.assert_array_equal(fits.area, np.pi * fits.height * fits.hwhm)
        np.testing.assert_allclose(fits.integral, SPACING * rows.sum(axis=1), rtol=1e-12)
        np.testing.assert_array_equal(fits.residual_variance, fits.rss / (n - p))
        assert np.all(fits.rss <= 1e-20) and fits.iterations.max() < 100
        if baseline == "constant":
            np.testing.assert_array_equal(fits.slope, 0.0)
    print(f"noise-free {shape} at origin {origin:g}, {baseline}: worst relative deviation from the truth {worst:.3e}")


def test_the_damped_oscillator_shape():
    """Height exactly h at xi0, the Lorentzian of half width g for g << xi0, and area pi h g over (0, inf)."""
    values = shape_values(200, 60.0, 3.0, "dho", 1.0e6)
    assert values[60] == 1.0
    np.testing.assert_allclose(values, shape_values(200, 60.0, 3.0, "lorentzian", 0.0), rtol=1e-3)  # (d / xi0 = 6e-5)
    xi = np.linspace(0.0, 4000.0, 4_000_001)
    wide = (2 * 7.0 * xi) ** 2 / ((30.0 ** 2 - xi ** 2) ** 2 + (2 * 7.0 * xi) ** 2)
    # (the tail beyond X is 4 g^2 / X to leading order)
    np.testing.assert_allclose(np.sum(wide) * 1e-3 + 4 * 49.0 / 4000.0, np.pi * 7.0, rtol=1e-5)
    w = axis_from(20.0, 80)
    row = 3.0 * shape_values(80, 25.4, 9.0, "dho", 20.0) + 0.2
    fits = fit_peaks_host(w, row, [w[0] - 0.1, w[-1] + 0.1], [w[24]], shape="dho")
    assert fits.status == 0 and fits.height.shape == (1,)
    np.testing.assert_allclose([fits.height[0], fits.position[0], fits.hwhm[0]], [3.0, w[0] + 25.4 * SPACING, 9.0 * SPACING],
                               rtol=1e-10)
    np.testing.assert_allclose(fits.lifetime_ps, 1.0 / (4.0 * np.pi * 2.99792458e-2 * fits.hwhm), rtol=1e-15)


@pytest.mark.parametrize("peaks", [2, 3])
def test_noisy_windows_reach_the_least_squares_minimum_and_its_curvature(peaks):
    """Every status is 0; S agrees with that of scipy's Levenberg-Marquardt, started at our parameters, to 1e-12, and
    the standard errors with ``sqrt(S / (n - p) diag (J^T J)^-1)`` of scipy's (finite-difference) Jacobian to 1e-6."""
    w, rows, windows, first, centres = noisy_family(80, peaks, seed=20261021 + peaks)
    fits = fit_peaks_host(w, rows, windows, centres)
    np.testing.assert_array_equal(fits.status, 0)
    n, p = 129, 3 * peaks + 1
    x = np.arange(n, dtype=np.float64)
    worst_s = worst_e = 0.0
    for f in range(len(rows)):
        y = rows[f, first[f]:first[f] + n]
        top = y.max()
        z = y / top

        def residuals(q):
            return z - (sum(q[3 * k] * q[3 * k + 2] ** 2 / ((x - q[3 * k + 1]) ** 2 + q[3 * k + 2] ** 2)
                            for k in range(peaks)) + q[3 * peaks])

        ours = np.empty(p)
        ours[0:3 * peaks:3] = fits.height[f] / top
        ours[1:3 * peaks:3] = (fits.position[f] - w[first[f]]) / SPACING
        ours[2:3 * peaks:3] = fits.hwhm[f] / SPACING
        ours[3 * peaks] = fits.baseline[f] / top
        theirs = scipy.optimize.least_squares(residuals, ours, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
        reference = float(np.sum(residuals(theirs.x) ** 2))
        worst_s = max(worst_s, abs(fits.rss[f] / reference - 1.0))
        covariance = reference / (n - p) * np.linalg.inv(theirs.jac.T @ theirs.jac)
        errors = np.sqrt(np.diag(covariance))
        mine = np.empty(p)
        mine[0:3 * peaks:3] = fits.height_error[f] / top
        mine[1:3 * peaks:3] = fits.position_error[f] / SPACING
        mine[2:3 * peaks:3] = fits.hwhm_error[f] / SPACING
        mine[3 * peaks] = fits.baseline_error[f] / top
        worst_e = max(worst_e, np.abs(mine / errors - 1.0).max())
    print(f"noisy, {peaks} peaks: worst |S / scipy's - 1| = {worst_s:.3e}, worst |error / scipy's - 1| = {worst_e:.3e}, "
          f"most iterations {fits.iterations.max()}")
    assert worst_s <= 1e-12
    assert worst_e <= 1e-6


def test_one_peak_agrees_with_the_one_peak_statement():
    """P = 1, constant baseline, Lorentzian, noise-free: position and width to 1e-9 of the width."""
    w, rows, windows, first, centres, truth, _ = noise_free_family(1, (6, 33, 64, 129), 8)
    many = fit_peaks_host(w, rows, windows, centres)
    one = fit_lorentzians_host(w, rows, windows)
    np.testing.assert_array_equal(one.status, 0)
    np.testing.assert_array_equal(many.status, 0)
    assert np.abs(many.position[:, 0] - one.position).max() <= 1e-9 * one.hwhm.min()
    assert (np.abs(many.hwhm[:, 0] - one.hwhm) / one.hwhm).max() <= 1e-9
    np.testing.assert_array_equal(many.integral, one.integral)
    np.testing.assert_array_equal(many.centroid, one.centroid)


def test_scaling_a_row_by_a_power_of_two_scales_the_fit_exactly():
    w, rows, windows, _, centres = noisy_family(12, 2, seed=7)
    for baseline in BASELINES:
        base = fit_peaks_host(w, rows, windows, centres, baseline=baseline)
        for k in (-20, 7):
            scaled = fit_peaks_host(w, rows * 2.0 ** k, windows, centres, baseline=baseline)
            for name in ("height", "height_error", "baseline", "baseline_error", "slope", "area", "integral"):
                np.testing.assert_array_equal(getattr(scaled, name), getattr(base, name) * 2.0 ** k, err_msg=name)
            for name in ("position", "hwhm", "position_error", "hwhm_error", "rss", "residual_variance", "centroid",
                         "status", "iterations"):
                np.testing.assert_array_equal(getattr(scaled, name), getattr(base, name), err_msg=name)


def test_moving_the_window_along_a_longer_row_moves_the_position_by_the_axis_offset():
    """(Lorentzian: the origin plays no part.  The axis is dyadic and stays inside one binade, so the sum
    ``w[b0] + x0 dw`` rounds alike at both places.)"""
    w, rows, windows, first, centres = noisy_family(8, 3, seed=11)
    base = fit_peaks_host(w, rows, windows, centres)
    long_w = axis_from(2048.0, 500)
    for shift in (1, 300):
        moved = np.zeros((len(rows), 500))
        moved_windows = []
        for f in range(len(rows)):
            moved[f, first[f] + shift:first[f] + shift + 129] = rows[f, first[f]:first[f] + 129]
            moved_windows.append(window(long_w, first[f] + shift, 129))
        fits = fit_peaks_host(long_w, moved, np.array(moved_windows), centres + shift * SPACING)
        np.testing.assert_array_equal(fits.position - base.position, shift * SPACING)
        np.testing.assert_array_equal(fits.centroid - base.centroid, shift * SPACING)
        for name in FIELDS:
            if name not in ("position", "centroid"):
                np.testing.assert_array_equal(getattr(fits, name), getattr(base, name), err_msg=name)


def test_permuting_the_centres_permutes_the_peaks():
    """The peaks come back in the order of the given centres.  A permutation changes the order of the elimination, so
    the two fits agree as two convergent fits of a noise-free window do, to 1e-9 on the relative measure, not bit for
    bit."""
    w, rows, windows, first, centres, truth, _ = noise_free_family(3, (33, 129), 4)
    base = fit_peaks_host(w, rows, windows, centres)
    order = [2, 0, 1]
    turned = fit_peaks_host(w, rows, windows, centres[:, order])
    np.testing.assert_array_equal(turned.status, 0)
    assert peak_deviation(turned, w, first, truth[:, order]).max() <= 1e-10
    for name in ("height", "position", "hwhm"):
        np.testing.assert_allclose(getattr(turned, name), getattr(base, name)[:, order], rtol=1e-9, err_msg=name)
    assert np.all(np.diff(base.position, axis=1) > 0) and not np.all(np.diff(turned.position, axis=1) > 0)


def test_status_codes():
    w, row, one_window = _two_peak_row()
    centres = _centres(w, 10, [11.0, 22.0])
    good = fit_peaks_host(w, row, one_window, centres)
    assert good.status == 0 and good.status.shape == () and good.height.shape == (2,)
    assert fit_peaks_multi(w, row, one_window, centres).iterations == good.iterations  # device=None: the host statement
    stopped = fit_peaks_host(w, row, one_window, centres, max_iterations=1)
    assert stopped.status == 1 and stopped.iterations == 1 and np.all(np.isfinite(stopped.position))
    rows = np.stack([row] * 6)
    rows[1, 20] = np.nan
    rows[2, :] = 0.0
    rows[3, :] = 4.5
    rows[4, 12] = np.inf
    fits = fit_peaks_host(w, rows, one_window, centres)
    np.testing.assert_array_equal(fits.status, [0, 2, 2, 2, 2, 0])
    bad = fits.status == 2
    for name in FIELDS[:-2]:
        assert np.all(np.isnan(getattr(fits, name)[bad])), name
        assert np.all(np.isfinite(getattr(fits, name)[~bad])), name
    np.testing.assert_array_equal(fits.iterations[bad], 0)
    for name in FIELDS:
        np.testing.assert_array_equal(getattr(fits, name)[5], getattr(fits, name)[0], err_msg=name)
    # status 3: no step is ever acceptable.  The arguments that the public entries refuse (here a width that is not a
    # number) reach the recipe itself: every step is non-finite and the damping passes 1e12 after 16 solves.
    out, status, iterations = _fit_window(row[10:43], 0.0, [11.0, 22.0], [np.nan, 3.0], False, False, 400)
    assert status == 3 and iterations == 16 and out.shape == (OUTPUTS,)
    assert np.all(np.isnan(out[14:28])) and out[29] == row.max()


def test_errors_are_nan_when_the_rows_cannot_carry_the_curvature():
    """Two peaks that start as twins on the tail of the row, 0.012 high and 1.5 bins wide: the first step (-0.15 in the
    height, -24 bins in the width) leaves the validity box and is refused, so after one solve the parameters are the
    twins still.
    Their columns of J are equal bit for bit, the elimination meets a pivot that is exactly zero, every error is NaN and
    the status is what it was."""
    w, row, one_window = _two_peak_row()
    twins = fit_peaks_host(w, row, one_window, _centres(w, 10, [31.0, 31.0]), hwhm=1.5, max_iterations=1)
    assert twins.status == 1
    np.testing.assert_array_equal(twins.position, w[10] + 31.0 * SPACING)
    for name in ("height_error", "position_error", "hwhm_error", "baseline_error"):
        assert np.all(np.isnan(getattr(twins, name))), name
    assert np.isfinite(twins.rss) and np.all(np.isfinite(twins.height))
    gram = np.array([[2.0, 2.0, 1.0, 0.3], [2.0, 2.0, 1.0, 0.3], [1.0, 1.0, 3.0, 0.1], [0.3, 0.3, 0.1, 0.5]])
    assert _solve(gram, 0.0, inverse=True) is None
    np.testing.assert_allclose(_solve(np.diag([2.0, 4.0, 8.0, 1.0]), 0.0, inverse=True), [0.5, 0.25, 0.125])
    # a window of exactly p + 2 bins carries it
    smallest = fit_peaks_host(w, row, window(w, 14, 9), _centres(w, 14, [3.0, 7.0]))
    assert smallest.status == 0 and np.all(np.isfinite(smallest.position_error))


def test_window_and_centre_shapes():
    w, row, one_window = _two_peak_row()
    centres = _centres(w, 10, [11.0, 22.0])
    one = fit_peaks_host(w, row, one_window, centres)
    several = fit_peaks_host(w, row, [one_window, window(w, 8, 37), one_window], centres)
    assert several.height.shape == (3, 2) and several.status.shape == (3,) and several.status.dtype == np.int32
    np.testing.assert_array_equal(several.position[0], one.position)
    np.testing.assert_array_equal(several.position[2], one.position)
    rows = np.stack([row, 2.0 * row, 4.0 * row]).reshape(3, 1, 64)
    every = fit_peaks_host(w, rows, one_window, centres, hwhm=2.0)
    assert every.height.shape == (3, 1, 2) and every.rss.shape == (3, 1)
    per_fit = fit_peaks_host(w, rows, one_window, np.broadcast_to(centres, (3, 1, 2)), hwhm=np.full((3, 1, 2), 2.0))
    _assert_same(per_fit, every)
    np.testing.assert_array_equal(every.position[1], every.position[0])
    single = fit_peaks_host(w, row, one_window, centres[:1])
    assert single.height.shape == (1,)


@pytest.mark.parametrize("fit", [fit_peaks_host, fit_peaks_multi])
def test_value_errors(fit):
    w, row, one_window = _two_peak_row()
    centres = _centres(w, 10, [11.0, 22.0])
    crooked = w.copy()
    crooked[30] += 1e-8 * SPACING
    with pytest.raises(ValueError, match="uniform"):
        fit(crooked, row, one_window, centres)
    with pytest.raises(ValueError, match=r"holds 8 bins .*at least p \+ 2 = 9 for 2 peaks on a constant baseline"):
        fit(w, row, window(w, 10, 8), _centres(w, 10, [2.0, 5.0]))
    with pytest.raises(ValueError, match=r"holds 9 bins .*at least p \+ 2 = 10 for 2 peaks on a linear baseline"):
        fit(w, row, window(w, 10, 9), _centres(w, 10, [2.0, 5.0]), baseline="linear")
    with pytest.raises(ValueError, match="lo >= hi"):
        fit(w, row, [w[30], w[30]], centres)
    with pytest.raises(ValueError, match="non-finite"):
        fit(w, row, [w[10], np.nan], centres)
    with pytest.raises(ValueError, match="windows has wrong shape"):
        fit(w, np.stack([row, row, row]), np.zeros((2, 2)) + one_window, centres)
    with pytest.raises(ValueError, match="rows has wrong shape"):
        fit(w, row[:60], one_window, centres)
    with pytest.raises(ValueError, match="max_iterations"):
        fit(w, row, one_window, centres, max_iterations=0)
    for outside in (w[9], w[43], w[10] - 1e-6, w[42] + 1e-6):
        with pytest.raises(ValueError, match="outside the bins of its window"):
            fit(w, row, one_window, [w[20], outside])
    fit(w, row, one_window, [w[10], w[42]], max_iterations=1)  # (the window's first and last bin are inside)
    with pytest.raises(ValueError, match="not finite"):
        fit(w, row, one_window, [w[20], np.nan])
    with pytest.raises(ValueError, match="5 peaks per window: at most 4"):
        fit(w, row, one_window, w[[12, 16, 20, 24, 28]])
    with pytest.raises(ValueError, match="trailing axis"):
        fit(w, row, one_window, w[20])
    with pytest.raises(ValueError, match="centres has wrong shape"):
        fit(w, np.stack([row, row, row]), one_window, np.zeros((2, 2)) + centres)
    with pytest.raises(ValueError, match="unknown shape: 'fano'"):
        fit(w, row, one_window, centres, shape="fano")
    with pytest.raises(ValueError, match="unknown baseline: 'quadratic'"):
        fit(w, row, one_window, centres, baseline="quadratic")
    for width in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="hwhm must be positive and finite"):
            fit(w, row, one_window, centres, hwhm=width)
    with pytest.raises(ValueError, match="hwhm has wrong shape"):
        fit(w, row, one_window, centres, hwhm=[1.0, 2.0, 3.0])
    low = axis_from(-10.0, 64)  # the window's first bin is the zero of the axis
    with pytest.raises(ValueError, match="'dho' needs a window above 0 cm\\^-1"):
        fit(low, row, window(low, 10, 33), _centres(low, 10, [11.0, 22.0]), shape="dho")
    assert fit(low, row, window(low, 11, 32), _centres(low, 11, [10.0, 21.0]), shape="dho", max_iterations=1).status == 1


def test_value_errors_come_before_device_work():
    """With a device named, the same errors are raised before the library is asked for anything."""
    w, row, one_window = _two_peak_row()
    with pytest.raises(ValueError, match="outside the bins of its window"):
        fit_peaks_multi(w, row, one_window, [w[20], w[50]], device=0)
    with pytest.raises(ValueError, match="at least p \\+ 2 = 9"):
        fit_peaks_multi(w, row, window(w, 10, 8), _centres(w, 10, [2.0, 5.0]), device=0)
    with pytest.raises(ValueError, match="unknown shape"):
        fit_peaks_multi(w, row, one_window, [w[20], w[30]], shape="voigt", device=0)


def _call(rows, row_index, first_bin, num_bins, centres, widths, origin=None, count=None, shape=0, linear=0, peaks=None,
          max_iterations=400, num_rows=None):
    lib = _lib.load()
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    table = [np.ascontiguousarray(column, dtype=np.int64) for column in (row_index, first_bin, num_bins)]
    centres, widths = np.ascontiguousarray(centres, dtype=np.float64), np.ascontiguousarray(widths, dtype=np.float64)
    length = len(table[0])
    origin = np.ascontiguousarray(np.full(length, 100.0) if origin is None else origin, dtype=np.float64)
    count = length if count is None else count
    out = np.zeros((max(count, 1), OUTPUTS))
    status, iterations = np.zeros(max(count, 1), dtype=np.int32), np.zeros(max(count, 1), dtype=np.int32)
    rc = lib.rn_peakfit_fit(0, C.c_void_p(rows.ctypes.data), rows.shape[0] if num_rows is None else num_rows,
                            rows.shape[1], *(C.c_void_p(column.ctypes.data) for column in table), count, shape, linear,
                            centres.shape[1] if peaks is None else peaks, C.c_void_p(origin.ctypes.data),
                            C.c_void_p(centres.ctypes.data), C.c_void_p(widths.ctypes.data), max_iterations,
                            C.c_void_p(out.ctypes.data), C.c_void_p(status.ctypes.data),
                            C.c_void_p(iterations.ctypes.data))
    return rc, lib.rn_peakfit_last_error().decode()


def test_the_c_entry_refuses_bad_tables_before_it_touches_the_device():
    _, row, _ = _two_peak_row()
    rows = np.stack([row, row])
    good = dict(row_index=[0, 1], first_bin=[10, 10], num_bins=[33, 33], centres=[[11.0, 22.0], [11.0, 22.0]],
                widths=[[2.0, 2.0], [2.0, 2.0]])
    refusals = [
        (dict(row_index=[0, 2]), "row 2 is outside"),
        (dict(first_bin=[10, 40]), "fit 1: bins"),
        (dict(first_bin=[-1, 10]), "fit 0: bins"),
        (dict(num_bins=[33, 8], centres=[[11.0, 22.0], [2.0, 5.0]]), "fit 1: 8 bins, a fit of 7 parameters needs at least p + 2 = 9"),
        (dict(num_bins=[33, 9], centres=[[11.0, 22.0], [2.0, 5.0]], linear=1), "needs at least p + 2 = 10"),
        (dict(count=-1), "negative"),
        (dict(max_iterations=0), "max_iterations"),
        (dict(num_rows=0), "out of range"),
        (dict(peaks=0), "P = 0 peaks is outside 1 .. 4"),
        (dict(peaks=5), "P = 5 peaks is outside 1 .. 4"),
        (dict(shape=2), "shape = 2"),
        (dict(shape=-1), "shape = -1"),
        (dict(linear=2), "linear = 2"),
        (dict(centres=[[11.0, 22.0], [11.0, 32.5]]), "fit 1: centre 1 = 32.5 is outside [0, 32]"),
        (dict(centres=[[-0.5, 22.0], [11.0, 22.0]]), "fit 0: centre 0 = -0.5 is outside"),
        (dict(centres=[[11.0, np.nan], [11.0, 22.0]]), "fit 0: centre 1 = nan is outside"),
        (dict(widths=[[2.0, 2.0], [0.0, 2.0]]), "fit 1: width 0 = 0 is not positive and finite"),
        (dict(widths=[[2.0, -1.0], [2.0, 2.0]]), "fit 0: width 1 = -1 is not positive"),
        (dict(widths=[[2.0, 2.0], [2.0, np.inf]]), "fit 1: width 1 = inf is not positive and finite"),
        (dict(widths=[[np.nan, 2.0], [2.0, 2.0]]), "fit 0: width 0 = nan"),
        (dict(origin=[100.0, np.nan]), "fit 1: the origin is not finite"),
        (dict(origin=[np.inf, 100.0], shape=1), "fit 0: the origin is not finite"),
        (dict(origin=[100.0, 0.0], shape=1), "fit 1: origin 0 is not positive"),
        (dict(origin=[-3.0, 100.0], shape=1), "fit 0: origin -3 is not positive"),
    ]
    for changes, text in refusals:
        rc, message = _call(rows, **{**good, **changes})
        assert rc == _lib.RN_ERR_INVALID_ARGUMENT, (changes, rc)
        assert text in message, (changes, message)
    assert _call(rows, **{**good, "count": 0})[0] == _lib.RN_OK  # an empty table is no work
    assert _lib.load().rn_peakfit_window_capacity() >= 64


def test_new_symbols_are_declared_listed_and_exported():
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True,
                        text=True).stdout
    exported = set(re.findall(r" T (\w+)", nm))
    with open(os.path.join(ROOT, "include", "rn_peakfit.h"), encoding="utf-8") as file:
        text = re.sub(r"/\*.*?\*/", "", file.read(), flags=re.S)
    assert set(re.findall(r"\b(rn_peakfit_\w+)\s*\(", text)) == set(ENTRIES)
    assert set(_lib.PEAKFIT_SIGNATURES) == set(ENTRIES)
    for other in (_lib.SIGNATURES, _lib.INTERP_SIGNATURES, _lib.LINESHAPE_SIGNATURES, _lib.QH_SIGNATURES,
                  _lib.HT_SIGNATURES, _lib.BM_SIGNATURES):
        assert not set(ENTRIES) & set(other)
    for name in ENTRIES:
        assert name in exported, name
    assert int(re.search(r"#define RN_PEAKFIT_OUTPUTS (\d+)", text).group(1)) == OUTPUTS
    host, device = _lib.PEAKFIT_SIGNATURES["rn_peakfit_fit"], _lib.PEAKFIT_SIGNATURES["rn_peakfit_fit_device"]
    assert device[0] == host[0] and device[1] == host[1] + [C.c_void_p]
    one_peak = _lib.LINESHAPE_SIGNATURES["rn_lineshape_fit"][1]
    assert host[1][:8] == one_peak[:8] and host[1][-4:] == one_peak[-4:]  # the lineshape arguments around the new ones


@pytest.mark.parametrize("method", ["bootstrap", "jackknife", "blocks"])
def test_replicate_errors_of_peak_fits(method):
    """Against numpy by hand; replicates whose status is not 0 are left out of every peak of their window."""
    rng = np.random.default_rng(3)
    w = axis_from(2048.0, 64)
    clean = model(33, [(2.0, 11.3, 2.5), (1.2, 21.6, 3.0)], 0.25, 0.0)
    rows = np.zeros((6, 2, 64))
    rows[:, :, 10:43] = clean * (1.0 + 0.02 * rng.normal(size=(6, 2, 33)))
    rows[2, 1, 15] = np.nan  # one replicate of window 1 is degenerate
    fits = fit_peaks_host(w, rows, window(w, 10, 33), _centres(w, 10, [11.0, 22.0]))
    np.testing.assert_array_equal(fits.status != 0, np.arange(12).reshape(6, 2) == 5)
    errors = replicate_errors(fits, method, blocks_count=4 if method == "blocks" else None)
    assert isinstance(errors, PeakErrors) and errors.position_error.shape == (2, 2)
    np.testing.assert_array_equal(errors.used, [6, 5])
    for name, values in (("position_error", fits.position), ("hwhm_error", fits.hwhm), ("height_error", fits.height),
                         ("lifetime_ps_error", fits.lifetime_ps)):
        for window_index, keep in ((0, np.arange(6)), (1, np.array([0, 1, 3, 4, 5]))):
            sample = values[keep, window_index]  # [replicates][peaks]
            count = len(keep)
            if method == "bootstrap":
                want = sample.std(axis=0, ddof=1)
            elif method == "jackknife":
                want = np.sqrt((count - 1) / count * ((sample - sample.mean(axis=0)) ** 2).sum(axis=0))
            else:
                want = sample.std(axis=0, ddof=1) / np.sqrt(4)
            np.testing.assert_allclose(getattr(errors, name)[window_index], want, rtol=1e-12, err_msg=name)
    assert np.all(errors.position_error > 0)
    # the one-peak behaviour is what it was
    one = fit_lorentzians_host(w, rows[:, 0], window(w, 10, 20))
    np.testing.assert_array_equal(replicate_errors(one, method).position_error,
                                  replicate_standard_error(one.position, method, one.status == 0)[0])
    with pytest.raises(ValueError, match="no replicate axis"):
        replicate_errors(fit_peaks_host(w, rows[0, 0], window(w, 10, 33), _centres(w, 10, [11.0, 22.0])), method)
