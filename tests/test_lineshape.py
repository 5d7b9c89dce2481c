"""Lorentzian line-shape fits (``ramannoodle_amd.lineshape``): what needs no GPU.

The host statement ``fit_lorentzians_host`` against the truth of noise-free windows and against scipy's least squares on
noisy ones, its exact scaling and shift properties, the status codes, every ``ValueError``, the C entry's refusals (they
come before the device is touched), the new symbols, and ``fit_peaks`` of the host mode-VDOS classes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.optimize

from ramannoodle_amd import _lib
from ramannoodle_amd.lineshape import (LorentzianFits, fit_lorentzians, fit_lorentzians_host, mode_windows)
from ramannoodle_amd.spectrum import ModeVibrationalDensityOfStates, ModeVibrationalDensityOfStatesEnsemble
from tests.lineshape_cases import (SPACING, axis, lorentzian, noise_free_cases, noisy_family, relative_deviation, window)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rn_lineshape_fit", "rn_lineshape_fit_device", "rn_lineshape_window_capacity", "rn_lineshape_last_error")
FIELDS = ("height", "position", "hwhm", "baseline", "area", "integral", "centroid", "rss", "status", "iterations")


def _assert_same(got, want):
    for name in FIELDS:
        np.testing.assert_array_equal(getattr(got, name), getattr(want, name), err_msg=name)


def _good_row(bins=64, first=10, n=33):
    row = np.zeros(bins)
    row[first:first + n] = lorentzian(n, 2.0, 15.3, 3.0, 0.25)
    return row


def test_noise_free_windows_recover_the_truth():
    """Bound 1e-10 on the relative measure: the stop rule's step size, on a problem with zero residual."""
    cases = noise_free_cases((5, 6, 9, 64, 513))
    w = axis(600)
    rows = np.zeros((len(cases), 600))
    windows = []
    for f, (n, h, x0, g, c) in enumerate(cases):
        first = 3 + 5 * f
        rows[f, first:first + n] = lorentzian(n, h, x0, g, c)
        windows.append(window(w, first, n))
    fits = fit_lorentzians_host(w, rows, np.array(windows))
    assert isinstance(fits, LorentzianFits) and fits.height.shape == (len(cases),)
    np.testing.assert_array_equal(fits.status, 0)
    n, h, x0, g, c = np.array(cases).T
    first = 3 + 5 * np.arange(len(cases))
    deviation = relative_deviation(fits.height, (fits.position - w[first]) / SPACING, fits.hwhm / SPACING,
                                   fits.baseline, h, x0, g, c)
    print("noise-free: worst relative deviation from the truth", deviation.max())
    assert deviation.max() <= 1e-10
    np.testing.assert_array_equal(fits.area, np.pi * fits.height * fits.hwhm)
    np.testing.assert_allclose(fits.integral, SPACING * np.array([rows[f].sum() for f in range(len(cases))]),
                               rtol=1e-12)
    light = 2.99792458e-2  # cm / ps
    np.testing.assert_allclose(fits.lifetime_ps, 1.0 / (4.0 * np.pi * light * g * SPACING), rtol=1e-9)
    assert np.all(fits.rss <= 1e-20)


def test_noisy_windows_reach_the_least_squares_minimum():
    """Precondition: every host status is 0.  Then for every fit rss <= (1 + 1e-9) x the residual sum of squares of
    scipy's Levenberg-Marquardt started from our parameters: the parameters of the two differ to first order in
    scipy's stopping precision, the costs to second order.

    The family's noise-free third has zero residual: there both sums are nothing but the rounding of the model's own
    evaluation (each residual a few ulps of z <= 1, so S of the order of 1e-31), and their ratio says nothing.  The
    bound therefore carries the floor ``n (8 eps)^2`` (3e-30 n) below which float64 cannot tell two sums apart; on
    the noisy members (S from 1e-3 to 10) it changes nothing."""
    w, rows, windows, first, truth = noisy_family(84, seed=20261019)
    fits = fit_lorentzians_host(w, rows, windows)
    np.testing.assert_array_equal(fits.status, 0)
    assert fits.iterations.max() < 400
    worst = 0.0
    for f in range(len(rows)):
        n = int(truth[f, 0])
        y = rows[f, first[f]:first[f] + n]
        z = y / y.max()
        x = np.arange(n, dtype=np.float64)

        def residuals(p):
            return z - (p[0] * p[2] ** 2 / ((x - p[1]) ** 2 + p[2] ** 2) + p[3])

        ours = np.array([fits.height[f] / y.max(), (fits.position[f] - w[first[f]]) / SPACING, fits.hwhm[f] / SPACING,
                         fits.baseline[f] / y.max()])
        theirs = scipy.optimize.least_squares(residuals, ours, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
        reference = float(np.sum(residuals(theirs.x) ** 2))
        # (rss is the sum at our parameters; `ours` carries the rounding of the position at 1024 cm^-1, 2e-13 bins)
        np.testing.assert_allclose(fits.rss[f], np.sum(residuals(ours) ** 2), rtol=1e-12, atol=1e-20)
        if f % 3:  # (the noisy members: the figure that is printed)
            worst = max(worst, fits.rss[f] / reference - 1.0)
        floor = n * (8.0 * np.finfo(np.float64).eps) ** 2
        assert fits.rss[f] <= (1.0 + 1e-9) * reference + floor, (f, fits.rss[f], reference)
    print("noisy: worst rss / scipy's - 1 =", worst)


def test_scaling_a_row_by_a_power_of_two_scales_the_fit_exactly():
    w, rows, windows, _, _ = noisy_family(21, seed=7)
    base = fit_lorentzians_host(w, rows, windows)
    for k in (-20, 7):
        scaled = fit_lorentzians_host(w, rows * 2.0 ** k, windows)
        for name in ("height", "baseline", "area", "integral"):
            np.testing.assert_array_equal(getattr(scaled, name), getattr(base, name) * 2.0 ** k, err_msg=name)
        for name in ("position", "hwhm", "status", "iterations", "rss", "centroid"):
            np.testing.assert_array_equal(getattr(scaled, name), getattr(base, name), err_msg=name)


def test_moving_the_window_along_a_longer_row_moves_the_position_by_the_axis_offset():
    """(The axis is dyadic and stays inside one binade, so the sum ``w[b0] + x0 dw`` rounds alike at both places.)"""
    w, rows, windows, first, truth = noisy_family(14, seed=11)
    base = fit_lorentzians_host(w, rows, windows)
    long_w = axis(700)
    for shift in (1, 300):
        moved = np.zeros((len(rows), 700))
        moved_windows = []
        for f in range(len(rows)):
            n = int(truth[f, 0])
            moved[f, first[f] + shift:first[f] + shift + n] = rows[f, first[f]:first[f] + n]
            moved_windows.append(window(long_w, first[f] + shift, n))
        fits = fit_lorentzians_host(long_w, moved, np.array(moved_windows))
        np.testing.assert_array_equal(fits.position - base.position, shift * SPACING)
        np.testing.assert_array_equal(fits.centroid - base.centroid, shift * SPACING)
        for name in ("height", "hwhm", "baseline", "area", "integral", "rss", "status", "iterations"):
            np.testing.assert_array_equal(getattr(fits, name), getattr(base, name), err_msg=name)


def test_degenerate_windows_have_status_two_among_good_fits():
    w = axis(64)
    rows = np.stack([_good_row() for _ in range(7)])
    rows[1, 20] = np.nan
    rows[3, :] = 0.0
    rows[5, :] = 4.5
    rows[6, 12] = np.inf
    fits = fit_lorentzians_host(w, rows, window(w, 10, 33))
    np.testing.assert_array_equal(fits.status, [0, 2, 0, 2, 0, 2, 2])
    bad = fits.status == 2
    for name in FIELDS[:-2]:
        assert np.all(np.isnan(getattr(fits, name)[bad])), name
        assert np.all(np.isfinite(getattr(fits, name)[~bad])), name
    np.testing.assert_array_equal(fits.iterations[bad], 0)
    assert np.all(np.isnan(fits.lifetime_ps[bad]))
    _assert_same(fit_lorentzians_host(w, rows[[0, 2, 4]], window(w, 10, 33)),
                 fit_lorentzians_host(w, rows[[0, 0, 0]], window(w, 10, 33)))
    negative = fit_lorentzians_host(w, -rows[0] - 1.0, window(w, 10, 33))
    assert negative.status == 2 and negative.status.shape == ()


def test_iteration_limit_gives_status_one():
    w = axis(64)
    fits = fit_lorentzians_host(w, _good_row(), window(w, 10, 33), max_iterations=1)
    assert fits.status == 1 and fits.iterations == 1 and np.isfinite(fits.position)
    assert fit_lorentzians(w, _good_row(), window(w, 10, 33)).status == 0  # device=None is the host statement


def test_window_shapes():
    w = axis(64)
    row = _good_row()
    one = fit_lorentzians_host(w, row, window(w, 10, 33))
    assert one.height.shape == () and one.status.dtype == np.int32
    peaks = fit_lorentzians_host(w, row, [window(w, 10, 33), window(w, 8, 35), window(w, 10, 33)])
    assert peaks.height.shape == (3,)
    assert peaks.position[0] == one.position == peaks.position[2]
    rows = np.stack([row, 2.0 * row, 4.0 * row]).reshape(3, 1, 64)
    every = fit_lorentzians_host(w, rows, window(w, 10, 33))
    assert every.height.shape == (3, 1)
    per_row = fit_lorentzians_host(w, rows, np.array([window(w, 10, 33), window(w, 8, 35), window(w, 10, 33)])[:, None])
    assert per_row.height.shape == (3, 1)
    np.testing.assert_array_equal(per_row.position[[0, 2], 0], every.position[[0, 2], 0])
    np.testing.assert_array_equal(per_row.hwhm[1], peaks.hwhm[1])
    windows = mode_windows([10.0, 20.0], 2.5)
    np.testing.assert_array_equal(windows, [[7.5, 12.5], [17.5, 22.5]])


@pytest.mark.parametrize("fit", [fit_lorentzians_host, fit_lorentzians])
def test_value_errors(fit):
    w = axis(64)
    row = _good_row()
    crooked = w.copy()
    crooked[30] += 1e-8 * SPACING
    with pytest.raises(ValueError, match="uniform"):
        fit(crooked, row, window(w, 10, 33))
    with pytest.raises(ValueError, match="uniform"):
        fit(w[::-1], row, window(w, 10, 33))
    with pytest.raises(ValueError, match=r"holds 4 bins .*spacing 0\.5"):
        fit(w, row, window(w, 10, 4))
    with pytest.raises(ValueError, match="holds 2 bins"):  # the window runs past the end of the axis
        fit(w, row, [w[62] - 0.1, w[63] + 50.0])
    with pytest.raises(ValueError, match="lo >= hi"):
        fit(w, row, [w[30], w[30]])
    with pytest.raises(ValueError, match="lo >= hi"):
        fit(w, row, [w[40], w[20]])
    for edge in (np.nan, np.inf):
        with pytest.raises(ValueError, match="non-finite"):
            fit(w, row, [w[10], edge])
    rows = np.stack([row, row, row])
    for bad in (np.zeros((2, 2)) + window(w, 10, 33), np.zeros(3), np.zeros((3, 3)), np.zeros((3, 1, 2)), 5.0):
        with pytest.raises(ValueError, match="windows has wrong shape"):
            fit(w, rows, bad)
    with pytest.raises(ValueError, match="rows has wrong shape"):
        fit(w, rows[:, :60], window(w, 10, 33))
    with pytest.raises(ValueError, match="max_iterations"):
        fit(w, row, window(w, 10, 33), max_iterations=0)
    with pytest.raises(ValueError):
        mode_windows([[1.0, 2.0]], 1.0)
    with pytest.raises(ValueError):
        mode_windows([1.0, 2.0], 0.0)


def test_value_errors_come_before_device_work():
    """With a device named, the same errors are raised before the library is asked for anything."""
    w = axis(64)
    with pytest.raises(ValueError, match="holds 4 bins"):
        fit_lorentzians(w, _good_row(), window(w, 10, 4), device=0)
    with pytest.raises(ValueError, match="uniform"):
        fit_lorentzians(w ** 2, _good_row(), window(w, 10, 33), device=0)


def _call(rows, row_index, first_bin, num_bins, count=None, max_iterations=400, num_rows=None):
    lib = _lib.load()
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    table = [np.ascontiguousarray(column, dtype=np.int64) for column in (row_index, first_bin, num_bins)]
    count = len(table[0]) if count is None else count
    out = np.zeros((max(count, 1), 8))
    status, iterations = np.zeros(max(count, 1), dtype=np.int32), np.zeros(max(count, 1), dtype=np.int32)
    rc = lib.rn_lineshape_fit(0, C.c_void_p(rows.ctypes.data), rows.shape[0] if num_rows is None else num_rows,
                              rows.shape[1], *(C.c_void_p(column.ctypes.data) for column in table), count,
                              max_iterations, C.c_void_p(out.ctypes.data), C.c_void_p(status.ctypes.data),
                              C.c_void_p(iterations.ctypes.data))
    return rc, lib.rn_lineshape_last_error().decode()


def test_the_c_entry_refuses_bad_tables_before_it_touches_the_device():
    rows = np.stack([_good_row(), _good_row()])
    refusals = [
        (dict(row_index=[0, 2], first_bin=[10, 10], num_bins=[33, 33]), "row 2 is outside"),
        (dict(row_index=[0, -1], first_bin=[10, 10], num_bins=[33, 33]), "row -1 is outside"),
        (dict(row_index=[0, 1], first_bin=[10, 40], num_bins=[33, 25]), "fit 1: bins"),
        (dict(row_index=[0, 1], first_bin=[-1, 10], num_bins=[33, 33]), "fit 0: bins"),
        (dict(row_index=[0, 1], first_bin=[10, 10], num_bins=[33, 4]), "at least 5"),
        (dict(row_index=[0, 1], first_bin=[10, 10], num_bins=[33, 33], count=-1), "negative"),
        (dict(row_index=[0, 1], first_bin=[10, 10], num_bins=[33, 33], max_iterations=0), "max_iterations"),
        (dict(row_index=[0, 1], first_bin=[10, 10], num_bins=[33, 33], num_rows=0), "out of range"),
    ]
    for arguments, text in refusals:
        rc, message = _call(rows, **arguments)
        assert rc == _lib.RN_ERR_INVALID_ARGUMENT, (arguments, rc)
        assert text in message, (arguments, message)
    assert _call(rows, [0], [10], [33], count=0)[0] == _lib.RN_OK  # an empty table is no work
    assert _lib.load().rn_lineshape_window_capacity() >= 64


def test_new_symbols_are_declared_listed_and_exported():
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True,
                        text=True).stdout
    exported = set(re.findall(r" T (\w+)", nm))
    with open(os.path.join(ROOT, "include", "rn_lineshape.h"), encoding="utf-8") as file:
        text = re.sub(r"/\*.*?\*/", "", file.read(), flags=re.S)
    assert set(re.findall(r"\b(rn_lineshape_\w+)\s*\(", text)) == set(ENTRIES)
    assert set(_lib.LINESHAPE_SIGNATURES) == set(ENTRIES)
    assert not set(ENTRIES) & set(_lib.SIGNATURES)
    for name in ENTRIES:
        assert name in exported, name
    host, device = _lib.LINESHAPE_SIGNATURES["rn_lineshape_fit"], _lib.LINESHAPE_SIGNATURES["rn_lineshape_fit_device"]
    assert device[0] == host[0] and device[1] == host[1] + [C.c_void_p]


def small_trajectory(frames=40, atoms=3, modes=4, seed=3):
    """``(positions[frames][atoms][3], lattice, vectors[modes][atoms][3], masses)``: plumbing only, no physics."""
    rng = np.random.default_rng(seed)
    lattice = np.array([[5.0, 0.0, 0.0], [0.3, 5.2, 0.0], [0.0, -0.2, 4.9]])
    t = np.arange(frames)[:, None, None]
    phase = rng.uniform(0, 6.0, size=(1, atoms, 3))
    positions = rng.random((1, atoms, 3)) + 0.01 * np.cos(1.3 * t + phase) + 0.002 * rng.normal(size=(frames, atoms, 3))
    return positions, lattice, rng.normal(size=(modes, atoms, 3)), 1.0 + rng.random(atoms)


def peak_arguments(wavenumbers):
    """Centres and a half width that put five bins of a seven-bin axis into each of four windows."""
    spacing = wavenumbers[1] - wavenumbers[0]
    return wavenumbers[[2, 3, 3, 4]], 2.6 * spacing


@pytest.mark.parametrize("ensemble", [False, True])
def test_fit_peaks_fits_the_rows_of_measure_segments(ensemble):
    positions, lattice, vectors, masses = small_trajectory()
    if ensemble:
        vdos = ModeVibrationalDensityOfStatesEnsemble([positions, positions[::-1]], 2.0, lattice, vectors, masses)
    else:
        vdos = ModeVibrationalDensityOfStates(positions, 2.0, lattice, vectors, masses)
    w, _ = vdos.measure_segments(17)
    assert len(w) == 7
    centres, half_width = peak_arguments(w)
    for average in (True, False):
        w, rows = vdos.measure_segments(17, 6, "hann", average)
        got = vdos.fit_peaks(centres, half_width, segment_steps=17, hop=6, average=average)
        assert got.position.shape == rows.shape[:-1]
        windows = np.broadcast_to(mode_windows(centres, half_width), rows.shape[:-1] + (2,))
        _assert_same(got, fit_lorentzians_host(w, rows, windows))
    whole_axis = vdos.measure()[0]
    whole = vdos.fit_peaks(whole_axis[[4, 5, 6, 7]], 2.6 * (whole_axis[1] - whole_axis[0]))
    assert whole.position.shape == (4,)
    with pytest.raises(ValueError, match="centres"):
        vdos.fit_peaks(centres[:3], half_width, segment_steps=17)
