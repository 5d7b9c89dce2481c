#!/usr/bin/env python3
"""Segment-averaged MD Raman spectra on the GPU against the loop a caller had before them
(profiles/segment_spectra.txt).  A random symmetric alpha(t) of S = 200 001 steps in HBM, segments of W steps at 50 %
overlap (Q segments), K random configurations, the Hann taper for the new entry:
  (a) averaged    rn_md_raman_segments_device, average = 1: K rows reach the host
  (b) rows        rn_md_raman_segments_device, average = 0: Q * K rows reach the host (pageable memory)
  (c) loop        Q calls of rn_md_raman_polarized_device on slices of the same tensor (no taper: it has none), the
                  Q * K rows averaged on the host
One warm-up call of each path per case (plans, buffers); a device synchronise precedes every clock read; the median of
--reps timed calls.  The last column compares (a) with the boxcar taper against (c): they compute the same mean.

--paths a (or c) runs one path alone, for a kernel trace of a single row:
  rocprofv3 --kernel-trace --stats -- python tools/time_segment_spectra.py --widths 16385 --configs 720 --paths a --out ""

Usage: python tools/time_segment_spectra.py [--steps 200001] [--widths 1025,4097,16385] [--configs 1,720] [--reps 5]
                                            [--paths a,b,c] [--out profiles/segment_spectra.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch  # before the HIP library: one HIP runtime per process (torch's)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scipy.spatial.transform import Rotation  # noqa: E402

from ramannoodle_amd.spectrum import (_md_polarized_on_device, _md_segments_on_device, polarized_weights,  # noqa: E402
                                      segment_plan)


def timed(fn, reps):
    out = fn()  # warm-up
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200_001)
    ap.add_argument("--widths", default="1025,4097,16385")
    ap.add_argument("--configs", default="1,720")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--paths", default="a,b,c")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_spectra.txt"))
    args = ap.parse_args()
    paths = set(args.paths.split(","))
    if not paths or paths - {"a", "b", "c"}:
        ap.error("--paths takes a, b and c")
    torch.cuda.init()
    rng = np.random.default_rng(0)
    a = rng.normal(size=(args.steps, 3, 3))
    alpha = torch.tensor(a + np.swapaxes(a, 1, 2), device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"device: {torch.cuda.get_device_name(0)}; ROCm {torch.version.hip}; float64; S = {args.steps}, 50 % overlap; "
             f"medians of {args.reps} calls after a warm-up"]
    print(lines[0], flush=True)
    slower = []
    for width in (int(w) for w in args.widths.split(",")):
        _, hop, tau = segment_plan(args.steps, width, None, "hann")
        starts = np.arange((args.steps - width) // hop + 1) * hop
        for k in (int(c) for c in args.configs.split(",")):
            weights, _ = polarized_weights(rng.normal(size=(k, 3)), rng.normal(size=(k, 3)),
                                           Rotation.random(k, random_state=k).as_matrix())

            def segments(average, taper=tau):
                return _md_segments_on_device(alpha, 1.0, weights, width, hop, taper, average, 0, stream=stream)[1]

            def loop():
                total = np.zeros((k, (width - 1 + 1) // 2 - 1))
                for first in starts:
                    total += _md_polarized_on_device(alpha[first:first + width], 1.0, weights, 0, stream=stream)[1]
                return total / len(starts)

            line = f"W = {width:6d}  Q = {len(starts):4d}  K = {k:4d}:"
            if "a" in paths:
                _, t_mean = timed(lambda: segments(True), args.reps)
                line += f" (a) averaged {t_mean * 1e3:9.2f} ms  "
            if "b" in paths:
                _, t_rows = timed(lambda: segments(False), args.reps)
                line += f" (b) rows {t_rows * 1e3:9.2f} ms  "
            if "c" in paths:
                want, t_loop = timed(loop, args.reps)
                line += f" (c) loop of {len(starts)} calls {t_loop * 1e3:9.2f} ms  "
            if {"a", "c"} <= paths:
                got = segments(True, np.ones(width - 1))
                diff = np.abs(got - want).max() / np.abs(want).max()
                line += f" (c)/(a) {t_loop / t_mean:7.1f}x   max rel diff (a, boxcar) - (c) {diff:.1e}"
                if not t_mean < t_loop:
                    slower.append(line)
            print(line, flush=True)
            lines.append(line)
    if {"a", "c"} <= paths:
        lines.append("(a) is faster than (c) in every row" if not slower else
                     f"(a) is NOT faster than (c) in {len(slower)} row(s)")
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
