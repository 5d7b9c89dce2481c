#!/usr/bin/env python3
"""Timing record of the Lorentzian fits (profiles/lineshape_fit.txt): 769 channels x 100 segments, one window of 129 bins
per row, as a time-resolved mode-projected VDOS would bring them.

Three figures: ``fit_lorentzians`` on GPU 0 from host rows (the upload of the rows included), the same from a CUDA tensor
(only the table and the results travel), and the host statement, timed on ``--host-fits`` fits and scaled to all of them.
The rows are Lorentzians of random position and width under chi^2(2Q)/(2Q) noise with Q = 100 (a 100-segment average).

    python tools/lineshape_timing.py [--channels 769] [--segments 100] [--bins 256] [--window 129] [--repeats 7]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ramannoodle_amd.lineshape import fit_lorentzians, fit_lorentzians_host  # noqa: E402


def make_rows(segments, channels, bins, window, seed=0):
    rng = np.random.default_rng(seed)
    w = 2.0 * np.arange(1, bins + 1)
    first = rng.integers(0, bins - window + 1, size=(segments, channels))
    x = np.arange(bins)[None, None, :] - first[:, :, None]
    centre = window * rng.uniform(0.3, 0.7, size=(segments, channels, 1))
    width = rng.uniform(1.0, window / 6.0, size=(segments, channels, 1))
    height = 10.0 ** rng.uniform(-3, 3, size=(segments, channels, 1))
    rows = height * (width ** 2 / ((x - centre) ** 2 + width ** 2) + 0.2 * rng.random((segments, channels, 1)))
    rows *= rng.chisquare(200, size=rows.shape) / 200.0
    windows = np.stack([w[first] - 0.5, w[first] + 2.0 * window - 0.5], axis=-1)
    return w, rows, windows


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
    return (f"{name:<23}{median:9.2f} ms [{low:.2f} .. {high:.2f}]  ({1e3 * median / fits:.3f} us per fit), median "
            f"[min .. max] of {repeats} calls after a warm-up")


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--channels", type=int, default=769)
    parser.add_argument("--segments", type=int, default=100)
    parser.add_argument("--bins", type=int, default=256)
    parser.add_argument("--window", type=int, default=129)
    parser.add_argument("--repeats", type=int, default=7)
    parser.add_argument("--host-fits", type=int, default=769)
    args = parser.parse_args()
    import torch

    w, rows, windows = make_rows(args.segments, args.channels, args.bins, args.window)
    fits = args.segments * args.channels
    print(f"{fits} fits ({args.segments} segments x {args.channels} channels), windows of {args.window} bins, rows of "
          f"{args.bins} bins ({rows.nbytes / 2 ** 20:.0f} MiB); {torch.cuda.get_device_name(0)}")
    fit_lorentzians(w, rows[:1], windows[:1], device=0)  # loads the library and the kernel
    times, from_host = timed(lambda: fit_lorentzians(w, rows, windows, device=0), args.repeats)
    print(line("device, host rows:", times, fits, args.repeats))
    tensor = torch.tensor(rows, device="cuda")
    torch.cuda.synchronize()
    times, from_tensor = timed(lambda: fit_lorentzians(w, tensor, windows), args.repeats)
    print(line("device, device tensor:", times, fits, args.repeats))
    assert np.array_equal(from_host.position, from_tensor.position)
    count = min(args.host_fits, args.channels)
    t0 = time.perf_counter()
    on_host = fit_lorentzians_host(w, rows[0, :count], windows[0, :count])
    seconds = time.perf_counter() - t0
    print(f"{'host statement:':<23}{1e3 * seconds * fits / count:9.0f} ms  ({1e6 * seconds / count:.0f} us per fit), "
          f"one call of {count} fits, scaled")
    status = from_host.status
    print(f"status 0 / 1 / 2 / 3: {[int((status == k).sum()) for k in range(4)]}; iterations: mean "
          f"{from_host.iterations.mean():.1f}, most {from_host.iterations.max()}")
    worst = max((np.abs(from_host.position[0, :count] - on_host.position) / on_host.hwhm).max(),
                (np.abs(from_host.hwhm[0, :count] - on_host.hwhm) / on_host.hwhm).max())
    print(f"device against host on those {count} fits: position and width agree to {worst:.1e} of the width")


if __name__ == "__main__":
    main()
