"""Seeded windows for the Lorentzian-fit tests (``test_lineshape.py``, ``test_lineshape_gpu.py``)."""
import numpy as np

SPACING = 0.5   # cm^-1 per bin; the axes are dyadic so that offsets along them are exact
ORIGIN = 1024.0


def axis(bins):
    return ORIGIN + SPACING * np.arange(bins)


def lorentzian(n, h, x0, g, c):
    x = np.arange(n, dtype=np.float64)
    return h * g * g / ((x - x0) ** 2 + g * g) + c


def window(w, first, n):
    """The half-open window in cm^-1 that holds exactly bins ``first .. first + n - 1`` of ``w``."""
    return [w[first] - 0.25 * SPACING, w[first] + (n - 0.25) * SPACING]


def relative_deviation(h, x0, g, c, h_ref, x0_ref, g_ref, c_ref):
    """The measure of every bound here: height and baseline over the height, position and width over the width."""
    h, x0, g, c, h_ref, x0_ref, g_ref, c_ref = np.broadcast_arrays(h, x0, g, c, h_ref, x0_ref, g_ref, c_ref)
    return np.max([np.abs(h - h_ref) / h_ref, np.abs(c - c_ref) / h_ref, np.abs(x0 - x0_ref) / g_ref,
                   np.abs(g - g_ref) / g_ref], axis=0)


def fits_deviation(w, fits, reference):
    """``relative_deviation`` of one ``LorentzianFits`` from another, fit for fit."""
    return relative_deviation(fits.height, fits.position, fits.hwhm, fits.baseline, reference.height,
                              reference.position, reference.hwhm, reference.baseline)


def noise_free_cases(sizes):
    """``(n, h, x0, g, c)``: per size three widths from 0.6 bins to ``max(0.6, n / 6)``, the centre off the bins and
    inside the middle of the window, heights over nine decades."""
    cases = []
    for k, n in enumerate(sizes):
        widest = max(0.6, n / 6.0)
        for j, g in enumerate((0.6, 0.5 * (0.6 + widest), widest)):
            x0 = 0.5 * (n - 1) + (0.3, -0.2, 0.4)[j] * min(1.0, n / 10.0)
            h = 10.0 ** ((3 * k + j) % 9 - 4) * 1.37
            cases.append((n, h, x0, g, (0.0, 0.1, 0.3)[j] * h))
    return cases


def noisy_family(count, seed, bins=256):
    """The issue's family: ``n`` in {16, 33, 63, 64, 65, 129, 200}, ``g`` in [1, n/6] bins, the centre in the middle
    40 % of the window, heights over nine decades, a baseline up to 0.3 h; one third noise-free, the rest multiplied by
    chi^2(2Q)/(2Q) noise with Q = 16 or 64.  Returns ``(w, rows[count][bins], windows[count][2], first[count],
    truth[count][5])``, one fit per row at a varying offset."""
    rng = np.random.default_rng(seed)
    sizes = (16, 33, 63, 64, 65, 129, 200)
    w = axis(bins)
    rows = np.zeros((count, bins))
    windows, firsts, truth = [], [], []
    for f in range(count):
        n = sizes[f % len(sizes)]
        g = 1.0 + (n / 6.0 - 1.0) * rng.random()
        x0 = n * (0.3 + 0.4 * rng.random())
        h = 10.0 ** rng.uniform(-4.5, 4.5)
        c = 0.3 * rng.random() * h
        y = lorentzian(n, h, x0, g, c)
        kind = f % 3
        if kind:
            q = (16, 64)[kind - 1]
            y = y * rng.chisquare(2 * q, n) / (2 * q)
        first = int(rng.integers(0, bins - n + 1))
        rows[f, first:first + n] = y
        windows.append(window(w, first, n))
        firsts.append(first)
        truth.append((n, h, x0, g, c))
    return w, rows, np.array(windows), np.array(firsts), np.array(truth)
