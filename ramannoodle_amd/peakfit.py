"""Multi-peak line-shape fits of spectrum rows (an addition): overlapping peaks, damped-oscillator shapes, error estimates.

A fit is (row, first bin ``b0``, bin count ``n``, origin ``o``, ``P`` start centres, ``P`` start widths) on a uniformly
spaced wavenumber axis, ``P`` in 1..4.  It works in bin units, ``x = 0 .. n-1`` from ``b0``, on the normalised values
``z = y / max(y in the window)``, all float64, with the parameters in the order
``(h_1, x0_1, g_1, .., h_P, x0_P, g_P, c[, s])`` (``p = 3P + 1`` with ``baseline="constant"``, ``3P + 2`` with
``"linear"``) and the model

    m(x) = sum_k h_k l_k(x) + c + s t,    t = x - (n - 1) / 2.

``shape="lorentzian"``: ``d = x - x0``, ``l = g^2 / (d^2 + g^2)``, ``dm/dx0 = 2 h g^2 d / (d^2 + g^2)^2``,
``dm/dg = 2 h g d^2 / (d^2 + g^2)^2`` (the terms of ``lineshape._sums``).

``shape="dho"``: with ``xi = x + o`` and ``xi0 = x0 + o``, where ``o = w[b0] / dw`` is the window's first bin on the
absolute axis in bin units, ``a = xi0^2 - xi^2`` (formed as ``(xi0 - xi)(xi0 + xi)``), ``b = (2 g xi)^2`` and
``q = a^2 + b``: ``l = b / q``, the velocity power spectrum of a damped oscillator with damping ``Gamma = 2 g``.  Its
height is exactly ``h`` at ``xi0``, it tends to the Lorentzian of half width ``g`` for ``g << xi0``, and its area over
``(0, inf)`` is ``pi h g``, the Lorentzian's formula.  ``dm/dx0 = -4 h b a xi0 / q^2``, ``dm/dg = 8 h g xi^2 a^2 / q^2``.

Degenerate windows (a non-finite value, ``max <= 0`` or ``max == min``) give status 2 and NaN in every output.

Start values: ``c = min z``, ``s = 0``, ``x0_k`` the given centre, ``h_k = max(z[rint(x0_k)] - c, 1e-3)``, ``g_k`` the
given width clamped to ``[0.5, n / 2]``.  The peaks keep the order of the given centres; they are never sorted.

Levenberg-Marquardt as in ``lineshape``, from ``lambda = 1e-3``.  With ``A = [J | r]``
(``J = dm/dp``, ``r = z - m``) an iteration forms the Gram matrix ``A^T A``: ``N = J^T J``, ``J^T r`` its last column
and ``S = sum r^2`` its corner.  It solves ``(N + lambda diag N) delta = J^T r`` by Gaussian elimination without
pivoting in parameter order, the factor of row j at step i taken from the pivot row, ``N_ij / N_ii``.  The trial step is
*invalid* when it is non-finite or takes a peak out of ``h_k > 0``, ``1/8 <= g_k <= 4 n``, ``-n <= x0_k <= 2 n``, and
*small* when ``|dh_k| / h_k``, ``|dx0_k| / g_k``, ``|dg_k| / g_k``, ``|dc| / max_k h_k`` and ``|ds| n / max_k h_k`` are all
``<= 1e-10``.  A valid step with ``S' <= S`` is accepted and ``lambda = max(lambda / 10, 1e-12)``; either way the fit
stops with status 0 after a small step; a step that is not accepted grows ``lambda`` tenfold, and the fit stops with
status 3 once it exceeds 1e12.  After ``max_iterations`` solves the fit stops with status 1.  With status 1 or 3 the
outputs are the last accepted parameters.

Standard errors, after the last accepted step: ``sqrt(S / (n - p) (N^-1)_ii)`` with the undamped ``N`` at the final
parameters and ``N^-1`` from the same elimination applied to unit columns.  When a pivot is ``<= 0`` or not finite,
every error is NaN and the status stays what it was.  This is the curvature estimate for independent residuals of equal
variance.  Neighbouring bins of a windowed spectrum and overlapping segments are correlated, so it is optimistic there:
``lineshape.replicate_errors`` on the fits of replicate spectra remains the honest error bar.

A window needs ``n >= p + 2`` bins.  ``fit_peaks_host`` is this definition; ``rn_peakfit_fit`` (``csrc/peakfit.hip``,
``include/rn_peakfit.h``) is the same recipe with one wave per fit and the Gram matrix on the matrix pipe, and differs
from it by the order of the sums over the bins and by fused multiply-adds only.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
from numpy.typing import NDArray

from ramannoodle_amd._source import is_tensor
from ramannoodle_amd.lineshape import (_SPEED_OF_LIGHT, _STEP_TOLERANCE, STATUS_CONVERGED, STATUS_DEGENERATE,
                                       STATUS_MAX_ITERATIONS, STATUS_STALLED, _axis, _check_iterations, _check_rows,
                                       _fit_table, _rows_source)

MAX_PEAKS = 4       # RN_PEAKFIT_MAX_PEAKS
OUTPUTS = 32        # RN_PEAKFIT_OUTPUTS
_SLOTS = 14         # parameter (and error) slots of a fit's outputs: 3 x 4 + 2
SHAPES = ("lorentzian", "dho")
BASELINES = ("constant", "linear")


def num_parameters(peaks: int, baseline: str = "constant") -> int:
    """``p``: 3 per peak, the baseline's level and, with ``"linear"``, its slope."""
    return 3 * peaks + 1 + (baseline == "linear")


@dataclass(frozen=True)
class PeakFits:
    """The fits of ``fit_peaks_multi``.  ``height``, ``position``, ``hwhm``, ``area`` and the three ``*_error`` fields of
    the same names have the leading shape and a trailing axis of the ``P`` peaks, in the order of the given centres; the
    other fields have the leading shape.

    ``height``, ``baseline`` (the baseline at the middle of the window's bins) and their errors are in the row's units,
    ``position`` and ``hwhm`` (half width at half maximum; for ``"dho"`` half the damping) in cm^-1, ``slope`` in row
    units per cm^-1 (0 for a constant baseline).  ``area = pi height hwhm`` is the integral of a fitted peak over
    ``(0, inf)`` for both shapes.  The errors are the curvature estimates of the module's head: optimistic for correlated
    residuals.  ``rss`` is the sum of squares of the residuals of the normalised window and
    ``residual_variance = rss / (n - p)``.  ``integral``, ``centroid``, ``status`` and ``iterations`` are those of
    ``lineshape.LorentzianFits``, and ``lifetime_ps = 1 / (4 pi c hwhm)`` is its energy lifetime."""

    height: NDArray[np.float64]
    position: NDArray[np.float64]
    hwhm: NDArray[np.float64]
    area: NDArray[np.float64]
    height_error: NDArray[np.float64]
    position_error: NDArray[np.float64]
    hwhm_error: NDArray[np.float64]
    baseline: NDArray[np.float64]
    slope: NDArray[np.float64]
    baseline_error: NDArray[np.float64]
    rss: NDArray[np.float64]
    residual_variance: NDArray[np.float64]
    integral: NDArray[np.float64]
    centroid: NDArray[np.float64]
    status: NDArray[np.int32]
    iterations: NDArray[np.int32]

    @property
    def lifetime_ps(self) -> NDArray[np.float64]:
        return 1.0 / (4.0 * np.pi * _SPEED_OF_LIGHT * self.hwhm)


@dataclass(frozen=True)
class PeakErrors:
    """The error bars of ``lineshape.replicate_errors`` on a ``PeakFits``: the replicate standard errors of ``position``
    and ``hwhm`` (cm^-1), ``height`` and ``lifetime_ps``, each of the fits' shape without the replicate axis (the peak
    axis last), and ``used``, the number of replicates per fit whose status was 0 (fewer than two: NaN)."""

    position_error: NDArray[np.float64]
    hwhm_error: NDArray[np.float64]
    height_error: NDArray[np.float64]
    lifetime_ps_error: NDArray[np.float64]
    used: NDArray[np.int64]


# ----------------------------------------------------------------------------- the definition
def _gram(z, x, params, peaks: int, dho: bool, linear: bool, origin: float):
    """``A^T A`` of ``A = [J | r]`` at ``params``, symmetric: ``N`` in ``[:p, :p]``, ``J^T r`` in ``[:p, p]``, ``S`` in
    ``[p, p]``."""
    columns = []
    model = 0.0
    for k in range(peaks):
        h, x0, g = params[3 * k], params[3 * k + 1], params[3 * k + 2]
        if dho:
            xi, xi0 = x + origin, x0 + origin
            a = (xi0 - xi) * (xi0 + xi)
            twice = (g + g) * xi
            b = twice * twice
            inverse = 1.0 / (a * a + b)
            shape = b * inverse
            u = (4.0 * h) * shape * inverse * a
            jx = -(u * xi0)
            jg = u * a * (0.5 / g)
        else:
            d = x - x0
            g2 = g * g
            inverse = 1.0 / (d * d + g2)
            shape = g2 * inverse
            u = (h + h) * shape * inverse
            jx = u * d
            jg = jx * d * (1.0 / g)
        model = model + h * shape
        columns += [shape, jx, jg]
    model = model + params[3 * peaks]
    columns.append(np.ones_like(z))
    if linear:
        t = x - 0.5 * (len(z) - 1)
        model = model + params[3 * peaks + 1] * t
        columns.append(t)
    columns.append(z - model)
    a = np.stack(columns, axis=1)
    gram = a.T @ a
    return np.triu(gram) + np.triu(gram, 1).T


def _solve(gram, damping: float, inverse: bool = False):
    """Gaussian elimination without pivoting, rows in parameter order, on ``(N + damping diag N | J^T r | I)``.
    Returns ``delta``, or with ``inverse`` the diagonal of ``N^-1`` (None when a pivot is ``<= 0`` or not finite)."""
    p = len(gram) - 1
    m = np.concatenate([gram[:p, :p + 1], np.eye(p)], axis=1)
    index = np.arange(p)
    m[index, index] = m[index, index] + damping * m[index, index]
    with np.errstate(all="ignore"):
        for i in range(p - 1):
            factors = m[i, i + 1:p] / m[i, i]
            m[i + 1:, i + 1:] = m[i + 1:, i + 1:] - factors[:, None] * m[i, i + 1:]
        pivots = m[index, index].copy()
        solution = np.empty((p, p + 1))
        for i in range(p - 1, -1, -1):
            t = m[i, p:].copy()
            for j in range(i + 1, p):
                t = t - m[i, j] * solution[j]
            solution[i] = t / m[i, i]
    if not inverse:
        return solution[:, 0]
    if not np.all(np.isfinite(pivots)) or np.any(pivots <= 0):
        return None
    return solution[index, 1 + index]


def _fit_window(y, origin: float, centres, widths, dho: bool, linear: bool, max_iterations: int):
    """One fit in bin units: ``(outputs[OUTPUTS], status, iterations)``."""
    n, peaks = len(y), len(centres)
    p = 3 * peaks + 1 + int(linear)
    out = np.full(OUTPUTS, np.nan)
    if not np.all(np.isfinite(y)):
        return out, STATUS_DEGENERATE, 0
    top, low = float(y.max()), float(y.min())
    if top <= 0 or top == low:
        return out, STATUS_DEGENERATE, 0
    z = y / top
    x = np.arange(n, dtype=np.float64)
    total = float(np.sum(z))
    moment = float(np.sum(x * z))
    params = np.zeros(p)
    params[3 * peaks] = float(z.min())
    for k in range(peaks):
        params[3 * k] = max(float(z[int(np.rint(centres[k]))]) - params[3 * peaks], 1e-3)
        params[3 * k + 1] = centres[k]
        params[3 * k + 2] = min(max(float(widths[k]), 0.5), 0.5 * n)
    heights, positions, hwhms = slice(0, 3 * peaks, 3), slice(1, 3 * peaks, 3), slice(2, 3 * peaks, 3)
    damping = 1e-3
    gram = _gram(z, x, params, peaks, dho, linear, origin)
    status, iterations = STATUS_MAX_ITERATIONS, 0
    while iterations < max_iterations:
        iterations += 1
        delta = _solve(gram, damping)
        finite = bool(np.all(np.isfinite(delta)))
        small = False
        if finite:
            tallest = params[heights].max()
            scaled = [np.abs(delta[heights]) / params[heights], np.abs(delta[positions]) / params[hwhms],
                      np.abs(delta[hwhms]) / params[hwhms], [abs(delta[3 * peaks]) / tallest]]
            if linear:
                scaled.append([abs(delta[3 * peaks + 1]) * n / tallest])
            small = bool(np.concatenate(scaled).max() <= _STEP_TOLERANCE)
        trial = params + delta
        accepted = False
        if (finite and np.all(trial[heights] > 0) and np.all(trial[hwhms] >= 0.125) and np.all(trial[hwhms] <= 4.0 * n)
                and np.all(trial[positions] >= -float(n)) and np.all(trial[positions] <= 2.0 * n)):
            trial_gram = _gram(z, x, trial, peaks, dho, linear, origin)
            accepted = trial_gram[p, p] <= gram[p, p]
        if accepted:
            params, gram = trial, trial_gram
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
    out[:p] = params
    rss = float(gram[p, p])
    diagonal = _solve(gram, 0.0, inverse=True)
    if diagonal is not None:
        with np.errstate(all="ignore"):
            out[_SLOTS:_SLOTS + p] = np.sqrt(rss / (n - p) * diagonal)
    with np.errstate(all="ignore"):
        centre = moment / total if total != 0 else float("nan")
    out[28:] = rss, top, total, centre
    return out, status, iterations


# ----------------------------------------------------------------------------- tables and results
def _check_model(shape, baseline) -> tuple[bool, bool]:
    if shape not in SHAPES:
        raise ValueError(f"unknown shape: {shape!r} (one of {', '.join(SHAPES)})")
    if baseline not in BASELINES:
        raise ValueError(f"unknown baseline: {baseline!r} (one of {', '.join(BASELINES)})")
    return shape == "dho", baseline == "linear"


def _peak_table(w, spacing: float, rows_shape, windows, centres, hwhm, shape, baseline):
    """The fit table of ``fit_peaks_multi``: ``(row_index, first_bin, num_bins, origin[F], centres[F][P], widths[F][P],
    leading shape, dho, linear)``, the last three columns in bin units."""
    dho, linear = _check_model(shape, baseline)
    centres = np.asarray(centres, dtype=np.float64)
    if centres.ndim < 1 or centres.shape[-1] < 1:
        raise ValueError(f"centres needs a trailing axis of 1 to {MAX_PEAKS} peaks: shape {centres.shape}")
    peaks = centres.shape[-1]
    if peaks > MAX_PEAKS:
        raise ValueError(f"centres holds {peaks} peaks per window: at most {MAX_PEAKS} are fitted together")
    p = num_parameters(peaks, baseline)
    row_index, first, bins, leading = _fit_table(w, spacing, rows_shape, windows, min_bins=p + 2,
                                                 needs=f"p + 2 = {p + 2} for {peaks} peaks on a {baseline} baseline")
    count = len(row_index)
    try:
        centres = np.broadcast_to(centres, leading + (peaks,)).reshape(count, peaks)
    except ValueError:
        raise ValueError(f"centres has wrong shape: {centres.shape} does not broadcast to {leading + (peaks,)}") from None
    if not np.all(np.isfinite(centres)):
        raise ValueError("a centre is not finite")
    start = w[first]
    in_bins = (centres - start[:, None]) / spacing
    outside = (in_bins < 0) | (in_bins > (bins - 1)[:, None])
    if np.any(outside):
        f, k = (int(i[0]) for i in np.nonzero(outside))
        raise ValueError(f"centre {centres[f, k]:g} cm^-1 is outside the bins of its window, "
                         f"[{start[f]:g}, {w[first[f] + bins[f] - 1]:g}] cm^-1")
    if hwhm is None:
        widths = np.repeat((bins / (8.0 * peaks))[:, None], peaks, axis=1)
    else:
        hwhm = np.asarray(hwhm, dtype=np.float64)
        try:
            widths = np.broadcast_to(hwhm, leading + (peaks,)).reshape(count, peaks) / spacing
        except ValueError:
            raise ValueError(f"hwhm has wrong shape: {hwhm.shape} is neither a scalar nor that of centres") from None
        if not np.all(np.isfinite(widths)) or np.any(widths <= 0):
            raise ValueError("hwhm must be positive and finite")
    origin = start / spacing
    if dho and np.any(start <= 0):
        f = int(np.flatnonzero(start <= 0)[0])
        raise ValueError(f"shape 'dho' needs a window above 0 cm^-1: the first bin of a window is at {start[f]:g} cm^-1")
    return (row_index, first, bins, np.ascontiguousarray(origin), np.ascontiguousarray(in_bins),
            np.ascontiguousarray(widths), leading, dho, linear)


def _results(w, spacing: float, first, bins, leading, peaks: int, linear: bool, out, status, iterations) -> PeakFits:
    """Bin units and normalised values -> cm^-1 and the row's units."""
    p = 3 * peaks + 1 + int(linear)
    top = out[:, 29]
    start = w[first]

    def per_peak(values):
        return values.reshape(leading + (peaks,))

    h, x0, g = (out[:, k:3 * peaks:3] for k in range(3))
    eh, ex0, eg = (out[:, _SLOTS + k:_SLOTS + 3 * peaks:3] for k in range(3))
    height, hwhm = h * top[:, None], g * spacing
    slope = out[:, 3 * peaks + 1] * top / spacing if linear else np.where(np.isnan(top), np.nan, 0.0)
    with np.errstate(all="ignore"):
        variance = out[:, 28] / (bins - p)
    return PeakFits(height=per_peak(height), position=per_peak(start[:, None] + x0 * spacing), hwhm=per_peak(hwhm),
                    area=per_peak(np.pi * height * hwhm), height_error=per_peak(eh * top[:, None]),
                    position_error=per_peak(ex0 * spacing), hwhm_error=per_peak(eg * spacing),
                    baseline=(out[:, 3 * peaks] * top).reshape(leading), slope=slope.reshape(leading),
                    baseline_error=(out[:, _SLOTS + 3 * peaks] * top).reshape(leading),
                    rss=out[:, 28].reshape(leading).copy(), residual_variance=variance.reshape(leading),
                    integral=(spacing * (top * out[:, 30])).reshape(leading),
                    centroid=(start + out[:, 31] * spacing).reshape(leading),
                    status=status.reshape(leading), iterations=iterations.reshape(leading))


def fit_peaks_host(wavenumbers, rows, windows, centres, hwhm=None, shape: str = "lorentzian", baseline: str = "constant",
                   max_iterations: int = 400) -> PeakFits:
    """The definition at the head of this module, one fit after the other on the host.  Arguments and result as
    ``fit_peaks_multi``."""
    w, spacing = _axis(wavenumbers)
    rows = np.asarray(rows, dtype=np.float64)
    _check_rows(rows.shape, w)
    max_iterations = _check_iterations(max_iterations)
    row_index, first, bins, origin, centres, widths, leading, dho, linear = _peak_table(
        w, spacing, rows.shape, windows, centres, hwhm, shape, baseline)
    flat = rows.reshape(-1, len(w))
    count = len(row_index)
    out = np.empty((count, OUTPUTS))
    status, iterations = np.empty(count, dtype=np.int32), np.empty(count, dtype=np.int32)
    for f in range(count):
        out[f], status[f], iterations[f] = _fit_window(flat[row_index[f], first[f]:first[f] + bins[f]], float(origin[f]),
                                                       centres[f], widths[f], dho, linear, max_iterations)
    return _results(w, spacing, first, bins, leading, centres.shape[1], linear, out, status, iterations)


def window_capacity() -> int:
    """The longest window, in bins, that the kernel keeps in registers between iterations
    (``rn_peakfit_window_capacity``)."""
    from ramannoodle_amd import _lib
    return int(_lib.load().rn_peakfit_window_capacity())


def fit_peaks_multi(wavenumbers, rows, windows, centres, hwhm=None, shape: str = "lorentzian",
                    baseline: str = "constant", device=None, max_iterations: int = 400) -> PeakFits:
    """Fit ``P`` peaks on a constant or linear baseline to each window of ``rows`` ``(..., bins)`` on the uniform axis
    ``wavenumbers`` ``(bins,)``: the definition at the head of this module.

    ``rows`` and ``windows`` are those of ``lineshape.fit_lorentzians``: half-open windows ``[lo, hi)`` in cm^-1 of shape
    ``(2,)``, ``rows.shape[:-1] + (2,)``, or ``(W,2)`` with a single row.  ``centres`` in cm^-1 has a trailing axis of the
    ``P`` start positions (1 to 4) and broadcasts against the windows; each lies within the bins of its window.  ``hwhm``
    in cm^-1, the start widths, is a scalar or has the shape of ``centres``; by default the window's width / (8 P).
    ``shape`` is ``"lorentzian"`` or ``"dho"`` (the velocity power spectrum of a damped oscillator: windows above
    0 cm^-1 only), ``baseline`` ``"constant"`` or ``"linear"``.  A window holds at least ``p + 2`` bins.

    ``device=None`` fits on the host (``fit_peaks_host``); ``device=k`` fits on GPU k (``rn_peakfit_fit``, one wave per
    fit).  A contiguous float64 CUDA tensor for ``rows`` is read where it is, ordered after torch's current stream
    (``rn_peakfit_fit_device``); only the results travel to the host.  ``ValueError``, before any device work, for what
    ``fit_lorentzians`` refuses, a centre outside its window, more than 4 peaks, fewer than ``p + 2`` bins, an unknown
    shape or baseline, and ``"dho"`` on a window whose first bin is at or below 0 cm^-1."""
    if device is None and not is_tensor(rows):
        return fit_peaks_host(wavenumbers, rows, windows, centres, hwhm, shape, baseline, max_iterations)
    from ramannoodle_amd import _lib
    w, spacing = _axis(wavenumbers)
    pointer, device, stream, rows = _rows_source(rows, device)
    shape_of_rows = tuple(rows.shape)
    _check_rows(shape_of_rows, w)
    max_iterations = _check_iterations(max_iterations)
    row_index, first, bins, origin, centres, widths, leading, dho, linear = _peak_table(
        w, spacing, shape_of_rows, windows, centres, hwhm, shape, baseline)
    count, peaks = centres.shape
    out = np.empty((count, OUTPUTS))
    status, iterations = np.empty(count, dtype=np.int32), np.empty(count, dtype=np.int32)
    num_rows = int(np.prod(shape_of_rows[:-1], dtype=np.int64))
    entry = "rn_peakfit_fit" if stream is None else "rn_peakfit_fit_device"
    tail = () if stream is None else (C.c_void_p(stream),)
    rc = getattr(_lib.load(), entry)(device, C.c_void_p(pointer), num_rows, len(w), C.c_void_p(row_index.ctypes.data),
                                     C.c_void_p(first.ctypes.data), C.c_void_p(bins.ctypes.data), count, int(dho),
                                     int(linear), peaks, C.c_void_p(origin.ctypes.data), C.c_void_p(centres.ctypes.data),
                                     C.c_void_p(widths.ctypes.data), max_iterations, C.c_void_p(out.ctypes.data),
                                     C.c_void_p(status.ctypes.data), C.c_void_p(iterations.ctypes.data), *tail)
    _lib.check_status(rc, entry, "rn_peakfit_last_error")
    return _results(w, spacing, first, bins, leading, peaks, linear, out, status, iterations)
