#!/usr/bin/env python3
"""MD Raman spectra averaged over several runs, whole and by atom group, against what a caller had before them
(profiles/ensemble_spectra.txt).  R runs of S steps in HBM, joined end to end, segments of W steps at 50 % overlap within
each run (Q segments in all), the Hann taper.
Whole spectra, K random configurations:
  (a) table     one rn_md_raman_segments_at_device call over all runs, average = 1
  (b) per run   R calls of rn_md_raman_segments_device (one per run, average = 1), the mean taken on the host with each
                run's segment count as its weight
Partial spectra, G groups, K = 1:
  (c) table     one rn_md_raman_partial_segments_device call over all runs, average = 1
  (d) loop      Q calls of rn_md_raman_partial_device on the segments' slices (no taper: it has none), averaged on the host
One warm-up call of each path per case (plans, buffers); a device synchronise precedes every clock read; the median and
the range of --reps timed calls.  (a) and (b) compute the same mean; (c) with the boxcar taper computes (d)'s.

Usage: python tools/time_ensemble_spectra.py [--runs 8] [--steps 25001] [--width 4097] [--configs 7,720] [--groups 3,16]
                                             [--reps 5] [--paths a,b,c,d] [--out profiles/ensemble_spectra.txt]
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

from ramannoodle_amd.spectrum import (_md_partial_on_device, _md_partial_segments_on_device,  # noqa: E402
                                      _md_segments_at_on_device, _md_segments_on_device, _measure_weights,
                                      ensemble_segment_starts, polarized_weights, segment_plan)


def timed(fn, reps):
    out = fn()  # warm-up
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return out, float(np.median(times)), f"{np.median(times):9.2f} ms [{min(times):.2f} .. {max(times):.2f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=25_001)
    ap.add_argument("--width", type=int, default=4097)
    ap.add_argument("--configs", default="7,720")
    ap.add_argument("--groups", default="3,16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--paths", default="a,b,c,d")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_spectra.txt"))
    args = ap.parse_args()
    paths = set(args.paths.split(","))
    if not paths or paths - set("abcd"):
        ap.error("--paths takes a, b, c and d")
    torch.cuda.init()
    rng = np.random.default_rng(0)
    lengths = [args.steps] * args.runs
    width, hop, tau = segment_plan(args.steps, args.width, None, "hann")
    starts, run_index = ensemble_segment_starts(lengths, width, hop)
    per_run = int(np.sum(run_index == 0))
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"device: {torch.cuda.get_device_name(0)}; ROCm {torch.version.hip}; float64; R = {args.runs} runs of "
             f"S = {args.steps}, W = {width}, 50 % overlap, Q = {len(starts)}; median [min .. max] of {args.reps} calls "
             "after a warm-up"]
    print(lines[0], flush=True)
    if paths & {"a", "b"}:
        a = rng.normal(size=(args.runs * args.steps, 3, 3))
        alpha = torch.tensor(a + np.swapaxes(a, 1, 2), device="cuda")
        for k in (int(c) for c in args.configs.split(",")):
            weights, _ = polarized_weights(rng.normal(size=(k, 3)), rng.normal(size=(k, 3)),
                                           Rotation.random(k, random_state=k).as_matrix())

            def table():
                return _md_segments_at_on_device(alpha, 1.0, weights, width, starts, tau, True, 0, stream=stream)[1]

            def runs():
                total = 0.0
                for r in range(args.runs):
                    run = alpha[r * args.steps:(r + 1) * args.steps]
                    total = total + per_run * _md_segments_on_device(run, 1.0, weights, width, hop, tau, True, 0,
                                                                     stream=stream)[1]
                return total / len(starts)

            line = f"whole    K = {k:4d}:"
            if "a" in paths:
                got, t_table, text = timed(table, args.reps)
                line += f" (a) table {text}  "
            if "b" in paths:
                want, t_runs, text = timed(runs, args.reps)
                line += f" (b) {args.runs} calls {text}  "
            if {"a", "b"} <= paths:
                line += f" (b)/(a) {t_runs / t_table:6.2f}x   max rel diff {np.abs(got - want).max() / np.abs(want).max():.1e}"
            print(line, flush=True)
            lines.append(line)
        del alpha
    if paths & {"c", "d"}:
        weights = _measure_weights()
        for groups in (int(g) for g in args.groups.split(",")):
            d = rng.normal(size=(args.runs * args.steps - 1, groups, 3, 3))
            incr = torch.tensor(d + np.swapaxes(d, 2, 3), device="cuda")

            def table(taper=tau):
                return _md_partial_segments_on_device(incr, 1.0, weights, width, starts, taper, True, 0, stream=stream)[1]

            def loop():
                total = 0.0
                for first in starts:
                    total = total + _md_partial_on_device(incr[first:first + width - 1], 1.0, weights, 0, stream=stream)[1]
                return total / len(starts)

            line = f"partial  G = {groups:4d}:"
            if "c" in paths:
                _, t_table, text = timed(table, args.reps)
                line += f" (c) table {text}  "
            if "d" in paths:
                want, t_loop, text = timed(loop, args.reps)
                line += f" (d) {len(starts)} calls {text}  "
            if {"c", "d"} <= paths:
                got = table(np.ones(width - 1))
                line += (f" (d)/(c) {t_loop / t_table:6.2f}x   max rel diff (c, boxcar) - (d) "
                         f"{np.abs(got - want).max() / np.abs(want).max():.1e}")
            print(line, flush=True)
            lines.append(line)
            del incr
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
