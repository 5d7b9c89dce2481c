#!/usr/bin/env python3
"""Timing record of the multi-peak fits (profiles/peak_fits.txt): 769 channels x 100 segments, one window of 129 bins per
row with P = 1, 2 and 4 overlapping Lorentzians, the shape of profiles/lineshape_fit.txt.

Per P: ``fit_peaks_multi`` on GPU 0 from a CUDA tensor (only the table and the results travel) and from host rows (the
upload of the rows included), each as the median and range of ``--repeats`` whole calls after a warm-up, and the host
statement, timed on ``--host-fits`` fits and scaled to all of them.  For P = 1 also ``fit_lorentzians`` on the same
windows.  The rows carry chi^2(2Q)/(2Q) noise with Q = 100 (a 100-segment average); the start centres are the true ones
moved by up to 0.3 of the width.  The lines go to standard output and to ``--output``.

    python tools/peakfit_timing.py [--channels 769] [--segments 100] [--bins 256] [--window 129] [--repeats 7]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ramannoodle_amd.lineshape import fit_lorentzians  # noqa: E402
from ramannoodle_amd.peakfit import fit_peaks_host, fit_peaks_multi  # noqa: E402


def make_rows(segments, channels, bins, window, peaks, seed=0):
    """``(w, rows[segments][channels][bins], windows[..][2], centres[..][peaks])``: the peaks 1 to 3 x the sum of their
    widths apart, around the middle of the window."""
    rng = np.random.default_rng(seed + peaks)
    w = 2.0 * np.arange(1, bins + 1)
    shape = (segments, channels)
    first = rng.integers(0, bins - window + 1, size=shape)
    x = np.arange(bins)[None, None, :] - first[:, :, None]
    width = rng.uniform(3.0, 7.0, size=shape + (peaks,)) * 2.0 / peaks
    gaps = rng.uniform(1.0, 3.0, size=shape + (peaks - 1,)) * (width[..., :-1] + width[..., 1:])
    centre = np.concatenate([np.zeros(shape + (1,)), np.cumsum(gaps, axis=-1)], axis=-1)
    centre += 0.5 * (window - 1) - 0.5 * centre[..., -1:] + rng.uniform(-2, 2, size=shape + (1,))
    scale = 10.0 ** rng.uniform(-3, 3, size=shape + (1,))
    rows = 0.2 * rng.random(shape + (1,)) * np.ones(bins)
    for k in range(peaks):
        g, x0 = width[..., k:k + 1], centre[..., k:k + 1]
        rows += rng.uniform(0.5, 1.0, size=shape + (1,)) * g ** 2 / ((x - x0) ** 2 + g ** 2)
    rows *= scale
    rows *= rng.chisquare(200, size=rows.shape) / 200.0
    windows = np.stack([w[first] - 0.5, w[first] + 2.0 * window - 0.5], axis=-1)
    starts = w[first][..., None] + 2.0 * (centre + rng.uniform(-0.3, 0.3, size=centre.shape) * width)
    return w, rows, windows, starts


def timed(call, repeats):
    """``(median, min, max)`` in seconds of ``repeats`` calls after one warm-up call (every call ends in a device
    synchronise: the results are on the host when it returns), and the last result."""
    result = call()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        result = call()
        times.append(time.perf_counter() - t0)
    return (float(np.median(times)), min(times), max(times)), result


def line(name, times, fits, repeats):
    median, low, high = (1e3 * t for t in times)
    return (f"{name:<26}{median:9.2f} ms [{low:.2f} .. {high:.2f}]  ({1e3 * median / fits:.3f} us per fit), median "
            f"[min .. max] of {repeats} calls after a warm-up")


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--channels", type=int, default=769)
    parser.add_argument("--segments", type=int, default=100)
    parser.add_argument("--bins", type=int, default=256)
    parser.add_argument("--window", type=int, default=129)
    parser.add_argument("--repeats", type=int, default=7)
    parser.add_argument("--host-fits", type=int, default=300)
    parser.add_argument("--peaks", type=int, nargs="+", default=[1, 2, 4])
    parser.add_argument("--output", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                         "profiles", "peak_fits.txt"))
    args = parser.parse_args()
    import torch

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    fits = args.segments * args.channels
    say("# python tools/peakfit_timing.py; records, not gates")
    say(f"{fits} fits ({args.segments} segments x {args.channels} channels), windows of {args.window} bins, rows of "
        f"{args.bins} bins; {torch.cuda.get_device_name(0)}; torch {torch.__version__}; float64")
    for peaks in args.peaks:
        w, rows, windows, centres = make_rows(args.segments, args.channels, args.bins, args.window, peaks)
        say(f"## P = {peaks}, Lorentzians on a constant baseline")
        fit_peaks_multi(w, rows[:1], windows[:1], centres[:1], device=0)  # loads the library and the kernel
        tensor = torch.tensor(rows, device="cuda")
        torch.cuda.synchronize()
        times, from_tensor = timed(lambda: fit_peaks_multi(w, tensor, windows, centres), args.repeats)
        say(line("device, device tensor:", times, fits, args.repeats))
        times, from_host = timed(lambda: fit_peaks_multi(w, rows, windows, centres, device=0), args.repeats)
        say(line("device, host rows:", times, fits, args.repeats))
        assert np.array_equal(from_host.position, from_tensor.position)
        if peaks == 1:
            times, one = timed(lambda: fit_lorentzians(w, tensor, windows), args.repeats)
            say(line("fit_lorentzians, tensor:", times, fits, args.repeats))
            both = (one.status == 0) & (from_tensor.status == 0)
            worst = (np.abs(one.position - from_tensor.position[..., 0]) / one.hwhm)[both].max()
            say(f"fit_lorentzians against P = 1 where both converged ({int(both.sum())} fits): positions agree to "
                f"{worst:.1e} of the width")
        count = min(args.host_fits, args.channels)
        t0 = time.perf_counter()
        on_host = fit_peaks_host(w, rows[0, :count], windows[0, :count], centres[0, :count])
        seconds = time.perf_counter() - t0
        say(f"{'host statement:':<26}{1e3 * seconds * fits / count:9.0f} ms  ({1e6 * seconds / count:.0f} us per fit), one "
            f"call of {count} fits, scaled")
        status = from_host.status
        say(f"status 0 / 1 / 2 / 3: {[int((status == k).sum()) for k in range(4)]}; iterations: mean "
            f"{from_host.iterations.mean():.1f}, most {from_host.iterations.max()}")
        same = (from_host.status[0, :count] == 0) & (on_host.status == 0)
        worst = max((np.abs(from_host.position[0, :count] - on_host.position) / on_host.hwhm)[same].max(),
                    (np.abs(from_host.hwhm[0, :count] - on_host.hwhm) / on_host.hwhm)[same].max())
        say(f"device against host on those {count} fits ({int(same.sum())} converged on both): position and width agree "
            f"to {worst:.1e} of the width")
    # the timing lines replace the head of the record; what follows them there (the notes, the compiler's figures and
    # the deviations of the tests, written by hand from the first "(" line on) stays
    kept = ""
    if os.path.exists(args.output):
        with open(args.output, encoding="utf-8") as file:
            old = file.read()
        if "\n(" in old:
            kept = old[old.index("\n(") + 1:]
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w", encoding="utf-8") as file:
        file.write("\n".join(lines) + "\n" + kept)


if __name__ == "__main__":
    main()
