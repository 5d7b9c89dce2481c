"""Seeded windows for the multi-peak fit tests (``test_peakfit.py``, ``test_peakfit_gpu.py``)."""
import numpy as np

from tests.lineshape_cases import SPACING, window

SHAPES = ("lorentzian", "dho")
BASELINES = ("constant", "linear")


def axis_from(origin, bins):
    """A dyadic axis whose first bin is ``origin`` bins above 0 cm^-1."""
    return SPACING * (origin + np.arange(bins))


def shape_values(n, x0, g, shape, origin):
    x = np.arange(n, dtype=np.float64)
    if shape == "dho":
        xi, xi0 = x + origin, x0 + origin
        b = (2.0 * g * xi) ** 2
        return b / ((xi0 - xi) ** 2 * (xi0 + xi) ** 2 + b)
    return g * g / ((x - x0) ** 2 + g * g)


def model(n, peaks, c, s, shape="lorentzian", origin=0.0):
    """``sum_k h_k l_k(x) + c + s (x - (n - 1) / 2)`` on ``x = 0 .. n-1``; ``peaks`` is ``[(h, x0, g), ..]``."""
    y = c + s * (np.arange(n, dtype=np.float64) - 0.5 * (n - 1))
    for h, x0, g in peaks:
        y = y + h * shape_values(n, x0, g, shape, origin)
    return y


def num_parameters(peaks, baseline):
    return 3 * peaks + 1 + (baseline == "linear")


def peak_deviation(fits, w, first, truth, top=1.0):
    """``lineshape_cases.relative_deviation`` per peak: heights and the baseline over the peak's height, position and
    width over its width.  ``fits`` a ``PeakFits`` of leading shape ``(F,)``, ``truth[F][P][3]`` in bin units and row
    units, ``first[F]`` the windows' first bins.  Returns ``[F][P]``."""
    truth = np.asarray(truth, dtype=np.float64)
    h, x0, g = truth[..., 0], truth[..., 1], truth[..., 2]
    position = (fits.position - w[np.asarray(first)][:, None]) / SPACING
    return np.max([np.abs(fits.height - h) / h, np.abs(position - x0) / g, np.abs(fits.hwhm / SPACING - g) / g], axis=0)


def fits_deviation(fits, reference):
    """The same measure between two ``PeakFits``, the baseline and the slope (over a window of ``n`` bins; here as the
    change of the baseline per bin) included, against the smallest height of the fit.  Returns ``[F]``."""
    per_peak = np.max([np.abs(fits.height - reference.height) / reference.height,
                       np.abs(fits.position - reference.position) / reference.hwhm,
                       np.abs(fits.hwhm - reference.hwhm) / reference.hwhm], axis=0).max(axis=-1)
    smallest = reference.height.min(axis=-1)
    return np.max([per_peak, np.abs(fits.baseline - reference.baseline) / smallest,
                   np.abs(fits.slope - reference.slope) * SPACING / smallest], axis=0)


def errors_deviation(fits, reference):
    """The standard errors of one ``PeakFits`` against another's, relative to themselves.  Returns ``[F]``."""
    names = ("height_error", "position_error", "hwhm_error")
    per_peak = np.max([np.abs(getattr(fits, name) - getattr(reference, name)) / getattr(reference, name)
                       for name in names], axis=0).max(axis=-1)
    return np.maximum(per_peak, np.abs(fits.baseline_error - reference.baseline_error) / reference.baseline_error)


def noise_free_family(peaks, sizes, seeds, shape="lorentzian", baseline="constant", origin=2048.0, bins=None):
    """The issue's noise-free family: per size and seed ``peaks`` peaks with centres spread evenly over the window,
    ``g`` in ``[0.08, 0.2] n / P`` and at least 0.6 bins, heights in [0.3, 1.3] x a scale over nine decades, a baseline
    up to 0.3 of the scale (and a slope that moves it by up to 20 % across the window); the start centres within
    +-0.5 g of the truth (and inside the window), the start widths ``n / (8 P)``.  One fit per row at a varying offset.
    Returns ``(w, rows[F][bins], windows[F][2], first[F], centres[F][P] in cm^-1, truth[F][P][3], base[F][2])``."""
    rng = np.random.default_rng(1000 * peaks + 7)
    bins = max(sizes) + 16 if bins is None else bins
    w = axis_from(origin, bins)
    rows, windows, firsts, centres, truth, base = [], [], [], [], [], []
    for n in sizes:
        for seed in range(seeds):
            scale = 10.0 ** ((seed + n) % 9 - 4) * 1.37
            triplets = []
            for k in range(peaks):
                g = max(rng.uniform(0.08, 0.2) * n / peaks, 0.6)
                x0 = (k + 0.5) * n / peaks - 0.5 + rng.uniform(-0.2, 0.2)
                triplets.append((scale * rng.uniform(0.3, 1.3), x0, g))
            c = 0.3 * rng.random() * scale
            s = 0.2 * c / n * rng.uniform(-1, 1) if baseline == "linear" else 0.0
            first = int(rng.integers(0, bins - n + 1))
            row = np.zeros(bins)
            row[first:first + n] = model(n, triplets, c, s, shape, origin + first)
            start = [min(max(x0 + rng.uniform(-0.5, 0.5) * g, 0.0), n - 1.0) for _, x0, g in triplets]
            rows.append(row)
            windows.append(window(w, first, n))
            firsts.append(first)
            centres.append(w[first] + SPACING * np.array(start))
            truth.append(triplets)
            base.append((c, s))
    return (w, np.array(rows), np.array(windows), np.array(firsts), np.array(centres), np.array(truth), np.array(base))


def noisy_family(count, peaks, seed, n=129, bins=160, origin=2048.0):
    """The issue's noisy family: ``n = 129``, ``peaks`` overlapping Lorentzians (neighbours 1 to 3 x the sum of their
    widths apart) on a constant baseline, every row multiplied by 5 % Gaussian noise.  Returns ``(w, rows, windows,
    first, centres in cm^-1)``; the start centres are the true ones moved by up to +-0.3 g."""
    rng = np.random.default_rng(seed)
    w = axis_from(origin, bins)
    rows, windows, firsts, centres = np.zeros((count, bins)), [], [], []
    for f in range(count):
        scale = 10.0 ** rng.uniform(-4.5, 4.5)
        g = rng.uniform(3.0, 7.0, peaks) * 2.0 / peaks
        gaps = rng.uniform(1.0, 3.0, peaks - 1) * (g[:-1] + g[1:])
        x0 = np.concatenate([[0.0], np.cumsum(gaps)])
        x0 = x0 + 0.5 * (n - 1) - 0.5 * x0[-1] + rng.uniform(-2, 2)
        triplets = [(scale * rng.uniform(0.5, 1.0), x0[k], g[k]) for k in range(peaks)]
        y = model(n, triplets, 0.1 * rng.random() * scale, 0.0) * (1.0 + 0.05 * rng.normal(size=n))
        first = int(rng.integers(0, bins - n + 1))
        rows[f, first:first + n] = y
        windows.append(window(w, first, n))
        firsts.append(first)
        centres.append(w[first] + SPACING * (x0 + rng.uniform(-0.3, 0.3, peaks) * g))
    return w, rows, np.array(windows), np.array(firsts), np.array(centres)
