"""Lorentzian line-shape fits of spectrum rows (an addition): peak positions, widths and lifetimes.

A fit is (row, first bin ``b0``, bin count ``n``) on a uniformly spaced wavenumber axis.  It works in bin units,
``x = 0 .. n-1`` from ``b0``, on the normalised values ``z = y / max(y in the window)``, with the model

    m(x) = h g^2 / ((x - x0)^2 + g^2) + c

(height ``h``, position ``x0``, half width at half maximum ``g``, baseline ``c``), all float64.

Degenerate windows (a non-finite value, ``max <= 0`` or ``max == min``) give status 2 and NaN in every output.

Start values: ``c = min z``; ``p`` the first bin that holds the maximum; ``h = z[p] - c``; ``x0 = p``;
``g = clamp(sum(z - c) / (pi h), 0.5, n / 2)``.

Levenberg-Marquardt, from ``lambda = 1e-3``.  With the residuals ``r = z - m`` and the analytic Jacobian ``J = dm/dp``
an iteration forms ``N = J^T J`` (10 unique entries), ``g = J^T r`` and ``S = sum r^2`` and solves
``(N + lambda diag N) delta = g`` by Gaussian elimination without pivoting in the order (h, x0, g, c).  The trial step
``p + delta`` is *invalid* when it is non-finite or leaves ``h > 0``, ``1/8 <= g <= 4 n`` or ``-n <= x0 <= 2 n``, and
*small* when ``max(|dh| / h, |dx0| / g, |dg| / g, |dc| / h) <= 1e-10``.  A valid step with ``S' <= S`` is accepted,
``lambda = max(lambda / 10, 1e-12)``, and the fit stops with status 0 if the step was small.  Otherwise the fit stops
with status 0 if the step was small, else ``lambda`` grows tenfold and the fit stops with status 3 once it exceeds
1e12.  After ``max_iterations`` solves the fit stops with status 1.  With status 1 or 3 the outputs are the last
accepted parameters.

``fit_lorentzians_host`` is this definition; ``rn_lineshape_fit`` (``csrc/lineshape.hip``, ``include/rn_lineshape.h``)
is the same recipe with one wave per fit, and differs from it by the order of the sums over the bins and by fused
multiply-adds only.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
from numpy.typing import NDArray

from ramannoodle_amd._source import is_tensor, source

STATUS_CONVERGED = 0
STATUS_MAX_ITERATIONS = 1
STATUS_DEGENERATE = 2
STATUS_STALLED = 3

MIN_BINS = 5  # RN_LINESHAPE_MIN_BINS
_OUTPUTS = 8  # RN_LINESHAPE_OUTPUTS: h, x0, g, c, S, max, sum z, sum x z / sum z
_STEP_TOLERANCE = 1e-10
_SPEED_OF_LIGHT = 2.99792458e-2  # cm / ps


@dataclass(frozen=True)
class LorentzianFits:
    """The fits of ``fit_lorentzians``, each field an array of the leading shape.

    ``height`` and ``baseline`` are in the row's units, ``position`` and ``hwhm`` (half width at half maximum) in
    cm^-1, ``area = pi height hwhm`` is the integral of the fitted peak without its baseline.  ``integral`` (the bin
    width times the sum of the window) and ``centroid`` (its first moment; not finite when the sum vanishes) are moments
    of the data: they need no fit and hold whenever ``status != 2``.  ``rss`` is the sum of squares of the residuals of
    the normalised window, ``iterations`` the number of solves.  ``status``: 0 converged, 1 stopped at
    ``max_iterations``, 2 a degenerate window (every output NaN), 3 no acceptable step (the damping passed 1e12).

    ``lifetime_ps = 1 / (4 pi c hwhm)`` with ``c = 2.99792458e-2 cm/ps`` is the energy lifetime: a damped oscillator
    whose energy decays as ``exp(-t / tau)`` (its amplitude as ``exp(-t / (2 tau))``) has a Lorentzian power spectrum
    of that half width at half maximum.  The amplitude lifetime is twice this number."""

    height: NDArray[np.float64]
    position: NDArray[np.float64]
    hwhm: NDArray[np.float64]
    baseline: NDArray[np.float64]
    area: NDArray[np.float64]
    integral: NDArray[np.float64]
    centroid: NDArray[np.float64]
    rss: NDArray[np.float64]
    status: NDArray[np.int32]
    iterations: NDArray[np.int32]

    @property
    def lifetime_ps(self) -> NDArray[np.float64]:
        return 1.0 / (4.0 * np.pi * _SPEED_OF_LIGHT * self.hwhm)


def mode_windows(centres, half_width) -> NDArray[np.float64]:
    """The ``(M,2)`` windows ``[centre - half_width, centre + half_width)`` of ``fit_lorentzians``."""
    centres = np.asarray(centres, dtype=np.float64)
    if centres.ndim != 1:
        raise ValueError(f"centres has wrong shape: {centres.shape} != (_,)")
    half_width = float(half_width)
    if not half_width > 0 or not np.isfinite(half_width):
        raise ValueError(f"half_width must be positive and finite: {half_width}")
    return np.stack([centres - half_width, centres + half_width], axis=1)


# ----------------------------------------------------------------------------- the definition
def _sums(z, x, h, x0, g, c):
    """The 15 sums of an iteration at (h, x0, g, c): N (10, row-major upper triangle), J^T r (4), S."""
    d = x - x0
    inverse = 1.0 / (d * d + g * g)
    lorentz = g * g * inverse
    r = z - (h * lorentz + c)
    u = (h + h) * lorentz * inverse
    jx = u * d                # dm/dx0 = 2 h g^2 d / q^2
    jg = jx * d * (1.0 / g)   # dm/dg  = 2 h g d^2 / q^2
    one = np.ones_like(z)
    columns = (lorentz, jx, jg, one)
    out = [float(np.sum(columns[a] * columns[b])) for a in range(4) for b in range(a, 4)]
    out += [float(np.sum(column * r)) for column in columns]
    out.append(float(np.sum(r * r)))
    return out


def _solve(sums, damping):
    """delta of (N + damping diag N) delta = J^T r: elimination without pivoting, rows in the order (h, x0, g, c)."""
    a = np.empty((4, 5))
    k = 0
    for i in range(4):
        for j in range(i, 4):
            a[i, j] = a[j, i] = sums[k]
            k += 1
        a[i, 4] = sums[10 + i]
    for i in range(4):
        a[i, i] = a[i, i] + damping * a[i, i]
    with np.errstate(all="ignore"):
        for i in range(4):
            for j in range(i + 1, 4):
                f = a[j, i] / a[i, i]
                for m in range(i + 1, 5):
                    a[j, m] = a[j, m] - f * a[i, m]
        delta = [0.0] * 4
        for i in (3, 2, 1, 0):
            t = a[i, 4]
            for j in range(i + 1, 4):
                t = t - a[i, j] * delta[j]
            delta[i] = float(t / a[i, i])
    return delta


def _fit_window(y: NDArray[np.float64], max_iterations: int):
    """One fit in bin units: ``(outputs[_OUTPUTS], status, iterations)``."""
    n = len(y)
    nan = [float("nan")] * _OUTPUTS
    if not np.all(np.isfinite(y)):
        return nan, STATUS_DEGENERATE, 0
    top, low = float(y.max()), float(y.min())
    if top <= 0 or top == low:
        return nan, STATUS_DEGENERATE, 0
    z = y / top
    x = np.arange(n, dtype=np.float64)
    total = float(np.sum(z))
    moment = float(np.sum(x * z))
    c = float(z.min())
    peak = int(np.argmax(z))  # the first bin that holds the maximum
    h = float(z[peak]) - c
    x0 = float(peak)
    g = min(max(float(np.sum(z - c)) / (np.pi * h), 0.5), 0.5 * n)
    damping = 1e-3
    sums = _sums(z, x, h, x0, g, c)
    status, iterations = STATUS_MAX_ITERATIONS, 0
    while iterations < max_iterations:
        iterations += 1
        dh, dx, dg, dc = _solve(sums, damping)
        finite = bool(np.isfinite(dh) and np.isfinite(dx) and np.isfinite(dg) and np.isfinite(dc))
        small = (finite and abs(dh) / h <= _STEP_TOLERANCE and abs(dx) / g <= _STEP_TOLERANCE
                 and abs(dg) / g <= _STEP_TOLERANCE and abs(dc) / h <= _STEP_TOLERANCE)
        th, tx, tg, tc = h + dh, x0 + dx, g + dg, c + dc
        accepted = False
        if finite and th > 0 and 0.125 <= tg <= 4.0 * n and -float(n) <= tx <= 2.0 * n:
            trial = _sums(z, x, th, tx, tg, tc)
            accepted = trial[14] <= sums[14]
        if accepted:
            h, x0, g, c, sums = th, tx, tg, tc, trial
            damping = max(damping / 10.0, 1e-12)
            if small:
                status = STATUS_CONVERGED
                break
        else:
            if small:
                status = STATUS_CONVERGED
                break
            damping = damping * 10.0
            if damping > 1e12:
                status = STATUS_STALLED
                break
    with np.errstate(all="ignore"):
        centre = moment / total if total != 0 else float("nan")
    return [h, x0, g, c, sums[14], top, total, centre], status, iterations


# ----------------------------------------------------------------------------- tables and results
def _axis(wavenumbers) -> tuple[NDArray[np.float64], float]:
    """The axis as float64 and its spacing; ``ValueError`` unless it ascends uniformly to 1e-9 of the spacing."""
    w = np.asarray(wavenumbers, dtype=np.float64)
    if w.ndim != 1 or len(w) < MIN_BINS:
        raise ValueError(f"wavenumbers must be one axis of at least {MIN_BINS} bins: shape {w.shape}")
    if not np.all(np.isfinite(w)):
        raise ValueError("wavenumbers has a non-finite entry")
    spacing = float((w[-1] - w[0]) / (len(w) - 1))
    if not spacing > 0 or np.abs(np.diff(w) - spacing).max() > 1e-9 * spacing:
        raise ValueError("wavenumbers must ascend with a uniform spacing (to 1e-9 of the spacing)")
    return w, spacing


def _fit_table(w, spacing: float, rows_shape, windows, min_bins: int = MIN_BINS, needs: str = str(MIN_BINS)):
    """``(row_index, first_bin, num_bins, leading shape)`` of the fits of ``windows`` on rows of shape ``rows_shape``;
    a window must hold ``min_bins`` bins, which the message spells as ``needs``."""
    windows = np.asarray(windows, dtype=np.float64)
    leading = tuple(rows_shape[:-1])
    count = int(np.prod(leading, dtype=np.int64))
    if windows.shape == (2,):
        edges = np.broadcast_to(windows, (count, 2))
        row_index = np.arange(count, dtype=np.int64)
    elif windows.shape == leading + (2,):
        edges = windows.reshape(count, 2)
        row_index = np.arange(count, dtype=np.int64)
    elif windows.ndim == 2 and windows.shape[1] == 2 and leading == ():
        edges = windows
        leading = (windows.shape[0],)
        row_index = np.zeros(windows.shape[0], dtype=np.int64)
    else:
        raise ValueError(f"windows has wrong shape: {windows.shape} is none of (2,), {leading + (2,)}, or (_,2) with "
                         "a single row")
    if not np.all(np.isfinite(edges)):
        raise ValueError("a window has a non-finite edge")
    if np.any(edges[:, 0] >= edges[:, 1]):
        bad = edges[np.flatnonzero(edges[:, 0] >= edges[:, 1])[0]]
        raise ValueError(f"window [{bad[0]:g}, {bad[1]:g}) is empty: lo >= hi")
    first = np.searchsorted(w, edges[:, 0], side="left").astype(np.int64)
    bins = np.searchsorted(w, edges[:, 1], side="left").astype(np.int64) - first
    if np.any(bins < min_bins):
        index = int(np.flatnonzero(bins < min_bins)[0])
        raise ValueError(f"window [{edges[index, 0]:g}, {edges[index, 1]:g}) holds {int(bins[index])} bins of the axis "
                         f"(spacing {spacing:g} cm^-1): a fit needs at least {needs}")
    return row_index, first, np.ascontiguousarray(bins), leading


def _results(w, spacing: float, first, leading, out, status, iterations) -> LorentzianFits:
    """Bin units and normalised values -> cm^-1 and the row's units."""
    h, x0, g, c, rss, top, total, centre = (out[:, k].reshape(leading) for k in range(_OUTPUTS))
    origin = w[first].reshape(leading)
    height, hwhm = h * top, g * spacing
    return LorentzianFits(height=height, position=origin + x0 * spacing, hwhm=hwhm, baseline=c * top,
                          area=np.pi * height * hwhm, integral=spacing * (top * total),
                          centroid=origin + centre * spacing, rss=rss.copy(),
                          status=status.reshape(leading), iterations=iterations.reshape(leading))


def _check_iterations(max_iterations) -> int:
    if int(max_iterations) != max_iterations or max_iterations < 1:
        raise ValueError(f"max_iterations must be a positive integer: {max_iterations}")
    return int(max_iterations)


def _check_rows(shape, w) -> None:
    if len(shape) < 1 or shape[-1] != len(w):
        raise ValueError(f"rows has wrong shape: {tuple(shape)} != (..., {len(w)})")


def fit_lorentzians_host(wavenumbers, rows, windows, max_iterations: int = 400) -> LorentzianFits:
    """The definition at the head of this module, one fit after the other on the host.  Arguments and result as
    ``fit_lorentzians``."""
    w, spacing = _axis(wavenumbers)
    rows = np.asarray(rows, dtype=np.float64)
    _check_rows(rows.shape, w)
    max_iterations = _check_iterations(max_iterations)
    row_index, first, bins, leading = _fit_table(w, spacing, rows.shape, windows)
    flat = rows.reshape(-1, len(w))
    count = len(row_index)
    out = np.empty((count, _OUTPUTS))
    status, iterations = np.empty(count, dtype=np.int32), np.empty(count, dtype=np.int32)
    for f in range(count):
        out[f], status[f], iterations[f] = _fit_window(flat[row_index[f], first[f]:first[f] + bins[f]], max_iterations)
    return _results(w, spacing, first, leading, out, status, iterations)


def window_capacity() -> int:
    """The longest window, in bins, that the kernel keeps on chip between iterations (``rn_lineshape_window_capacity``)."""
    from ramannoodle_amd import _lib
    return int(_lib.load().rn_lineshape_window_capacity())


def _rows_source(rows, device):
    """``source`` of the rows of a fit, with the device of the call: the tensor's GPU, which ``device`` may only
    confirm, or ``device`` for a host array."""
    pointer, index, stream, rows = source(rows, "rows must be a contiguous float64 CUDA tensor (or a host array)")
    if index is not None and device is not None and int(device) != index:
        raise ValueError(f"rows are on GPU {index}, not on device {device}")
    return pointer, int(device if index is None else index), stream, rows


def fit_lorentzians(wavenumbers, rows, windows, device=None, max_iterations: int = 400) -> LorentzianFits:
    """Fit one Lorentzian on a constant baseline to each window of ``rows`` ``(..., bins)`` on the uniform axis
    ``wavenumbers`` ``(bins,)``: the definition at the head of this module.

    ``windows`` in cm^-1 are half open, ``[lo, hi)``, and hold at least 5 bins each: ``(2,)`` is one window for every
    row, ``rows.shape[:-1] + (2,)`` one window per row, and ``(W,2)`` with a single row ``(bins,)`` W peaks of one
    spectrum.  The result's arrays have the shape ``rows.shape[:-1]``, or ``(W,)``.

    ``device=None`` fits on the host (``fit_lorentzians_host``); ``device=k`` fits on GPU k (``rn_lineshape_fit``, one
    wave per fit).  A contiguous float64 CUDA tensor for ``rows`` is read where it is, on its GPU, ordered after torch's
    current stream (``rn_lineshape_fit_device``); only the results travel to the host.  ``ValueError``, before any
    device work, for an axis that is not uniform, a window with fewer than 5 bins, ``lo >= hi``, a non-finite edge and
    a shape that fits none of the three forms."""
    if device is None and not is_tensor(rows):
        return fit_lorentzians_host(wavenumbers, rows, windows, max_iterations)
    from ramannoodle_amd import _lib
    w, spacing = _axis(wavenumbers)
    pointer, device, stream, rows = _rows_source(rows, device)
    shape = tuple(rows.shape)
    _check_rows(shape, w)
    max_iterations = _check_iterations(max_iterations)
    row_index, first, bins, leading = _fit_table(w, spacing, shape, windows)
    count = len(row_index)
    out = np.empty((count, _OUTPUTS))
    status, iterations = np.empty(count, dtype=np.int32), np.empty(count, dtype=np.int32)
    num_rows = int(np.prod(shape[:-1], dtype=np.int64))
    entry = "rn_lineshape_fit" if stream is None else "rn_lineshape_fit_device"
    tail = () if stream is None else (C.c_void_p(stream),)
    rc = getattr(_lib.load(), entry)(device, C.c_void_p(pointer), num_rows, len(w), C.c_void_p(row_index.ctypes.data),
                                     C.c_void_p(first.ctypes.data), C.c_void_p(bins.ctypes.data), count, max_iterations,
                                     C.c_void_p(out.ctypes.data), C.c_void_p(status.ctypes.data),
                                     C.c_void_p(iterations.ctypes.data), *tail)
    _lib.check_status(rc, entry, "rn_lineshape_last_error")
    return _results(w, spacing, first, leading, out, status, iterations)


# ----------------------------------------------------------------------------- error bars from replicate spectra
@dataclass(frozen=True)
class LorentzianErrors:
    """The error bars of ``replicate_errors``, each array of the fits' shape without the replicate axis: the standard
    errors of ``position`` and ``hwhm`` (cm^-1), ``lifetime_ps`` and ``area``, and ``used``, the number of replicates
    whose fit converged and went into them (fewer than two: NaN)."""

    position_error: NDArray[np.float64]
    hwhm_error: NDArray[np.float64]
    lifetime_ps_error: NDArray[np.float64]
    area_error: NDArray[np.float64]
    used: NDArray[np.int64]


REPLICATE_METHODS = ("bootstrap", "jackknife", "blocks")


def check_replicate_method(method) -> None:
    if method not in REPLICATE_METHODS:
        raise ValueError(f"unknown method: {method!r} (one of {', '.join(REPLICATE_METHODS)})")


def replicate_standard_error(replicates, method, valid=None, blocks_count=None):
    """The standard error over the replicate axis (the first) of ``replicates`` ``(R, ...)``.  ``"bootstrap"``:
    ``std(ddof=1)``; ``"jackknife"``: ``sqrt((G - 1) / G sum_r (rep_r - mean_r rep)^2)``; ``"blocks"``:
    ``std(ddof=1) / sqrt(G)``.  ``valid`` (bool, the shape of ``replicates``) leaves replicates out, entry by entry;
    ``G`` is ``blocks_count``, or the number of replicates used.  Fewer than two used: NaN.  Returns ``(error, used)``."""
    check_replicate_method(method)
    values = np.asarray(replicates, dtype=np.float64)
    valid = np.ones(values.shape, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    used = valid.sum(axis=0)
    with np.errstate(all="ignore"):
        mean = np.where(valid, values, 0.0).sum(axis=0) / used
        squares = np.where(valid, (values - mean) ** 2, 0.0).sum(axis=0)
        groups = used if blocks_count is None else blocks_count
        if method == "jackknife":
            error = np.sqrt((groups - 1) / groups * squares)
        else:
            error = np.sqrt(squares / (used - 1))
            if method == "blocks":
                error = error / np.sqrt(groups)
    return np.where(used >= 2, error, np.nan), used


def replicate_errors(fits, method: str, blocks_count=None):
    """Error bars of fitted peaks from the fits of replicate spectra: ``fits`` is
    ``fit_lorentzians(w, rows[R, ...], windows)`` on the rows of ``replicates.measure_segment_replicates`` (replicates along the
    first axis), ``method`` the one that made the replicates.  Each error is
    ``replicate_standard_error`` over the replicate axis: ``"bootstrap"`` ``std(ddof=1)``, ``"jackknife"``
    ``sqrt((G - 1) / G sum_r (x_r - mean x)^2)``, ``"blocks"`` ``std(ddof=1) / sqrt(G)``.  Replicates whose status is
    not 0 are left out, window by window; ``G`` is ``blocks_count`` or, by default, the number of replicates used.

    ``fits`` may also be the ``peakfit.PeakFits`` of ``peakfit.fit_peaks_multi`` on such rows: the result is then a
    ``peakfit.PeakErrors``, the errors of ``position``, ``hwhm``, ``height`` and ``lifetime_ps`` per peak (a replicate
    is left out of all the peaks of a window together)."""
    from ramannoodle_amd import peakfit
    status = np.asarray(fits.status)
    if status.ndim < 1:
        raise ValueError("fits has no replicate axis")
    valid = status == STATUS_CONVERGED
    used = valid.sum(axis=0).astype(np.int64)
    if isinstance(fits, peakfit.PeakFits):
        per_peak = np.broadcast_to(valid[..., None], fits.position.shape)
        errors = [replicate_standard_error(values, method, per_peak, blocks_count)[0]
                  for values in (fits.position, fits.hwhm, fits.height, fits.lifetime_ps)]
        return peakfit.PeakErrors(*errors, used=used)
    errors = [replicate_standard_error(values, method, valid, blocks_count)[0]
              for values in (fits.position, fits.hwhm, fits.lifetime_ps, fits.area)]
    return LorentzianErrors(*errors, used=used)
