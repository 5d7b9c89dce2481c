#!/usr/bin/env python3
"""Replicate spectra of the segment mean against what a caller had before them (profiles/replicate_spectra.txt).
R_runs runs of S steps in HBM, joined end to end, segments of W steps at 50 % overlap within each run (Q segments in
all), the Hann taper, K random configurations, R replicates: the jackknife over the runs (R = G = the number of runs)
and a bootstrap over the runs (R = 200).
  (a) replicates  one rn_md_raman_segment_replicates_device call: 6 Q + 2 R K transforms, R K rows to the host
  (b) rows        one rn_md_raman_segments_at_device call with average = 0 (Q (6 + 2 K) transforms, Q K rows to the
                  host), then numpy V @ rows
One warm-up call of each path per case (plans, buffers); a device synchronise precedes every clock read; the median and
the range of --reps timed calls.  Then, with rn_md_raman_segment_replicates_set_profiling(1), the HIP-event times of the
four phases of --reps more calls of (a) (the median of each phase).  The lines are appended to --out.

Usage: python tools/time_replicate_spectra.py [--runs 8] [--steps 25001] [--width 4097] [--configs 1,7]
                                              [--bootstrap 200] [--reps 5] [--out profiles/replicate_spectra.txt]
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

from ramannoodle_amd import _lib  # noqa: E402
from ramannoodle_amd.replicates import _md_segment_replicates_on_device, replicate_weights  # noqa: E402
from ramannoodle_amd.spectrum import (_md_segments_at_on_device, ensemble_segment_starts,  # noqa: E402
                                      polarized_weights, segment_plan)

PHASES = ("builder", "forward FFTs", "product kernel", "back half")


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


def phase_times(fn, reps):
    lib = _lib.load()
    lib.rn_md_raman_segment_replicates_set_profiling(1)
    rows = []
    try:
        for _ in range(reps):
            fn()
            millis = np.zeros(4)
            lib.rn_md_raman_segment_replicates_phase_times(millis.ctypes.data)
            rows.append(millis)
    finally:
        lib.rn_md_raman_segment_replicates_set_profiling(0)
    return np.median(rows, axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=25_001)
    ap.add_argument("--width", type=int, default=4097)
    ap.add_argument("--configs", default="1,7")
    ap.add_argument("--bootstrap", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replicate_spectra.txt"))
    args = ap.parse_args()
    torch.cuda.init()
    rng = np.random.default_rng(0)
    lengths = [args.steps] * args.runs
    width, hop, tau = segment_plan(args.steps, args.width, None, "hann")
    starts, run_index = ensemble_segment_starts(lengths, width, hop)
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"device: {torch.cuda.get_device_name(0)}; ROCm {torch.version.hip}; float64; {args.runs} runs of "
             f"S = {args.steps}, W = {width}, 50 % overlap, Q = {len(starts)}; median [min .. max] of {args.reps} calls "
             "after a warm-up"]
    print(lines[0], flush=True)
    a = rng.normal(size=(args.runs * args.steps, 3, 3))
    alpha = torch.tensor(a + np.swapaxes(a, 1, 2), device="cuda")
    tables = [("jackknife", replicate_weights(run_index, "jackknife")),
              ("bootstrap", replicate_weights(run_index, "bootstrap", args.bootstrap, seed=0))]
    for k in (int(c) for c in args.configs.split(",")):
        weights, _ = polarized_weights(rng.normal(size=(k, 3)), rng.normal(size=(k, 3)),
                                       Rotation.random(k, random_state=k).as_matrix())
        for name, table in tables:
            def replicates(table=table):
                return _md_segment_replicates_on_device(alpha, 1.0, weights, width, starts, tau, table, 0, stream=stream)[1]

            def rows(table=table):
                segment_rows = _md_segments_at_on_device(alpha, 1.0, weights, width, starts, tau, False, 0, stream=stream)[1]
                return np.einsum("rq,qkb->rkb", table, segment_rows)

            got, t_new, text_new = timed(replicates, args.reps)
            want, t_old, text_old = timed(rows, args.reps)
            line = (f"K = {k:2d}  R = {len(table):3d} ({name}): (a) replicates {text_new}   (b) rows, V @ rows {text_old}   "
                    f"(b)/(a) {t_old / t_new:6.2f}x   max rel diff {np.abs(got - want).max() / np.abs(want).max():.1e}")
            print(line, flush=True)
            lines.append(line)
            phases = phase_times(replicates, args.reps)
            line = "    phases of (a): " + ", ".join(f"{label} {ms:.3f} ms" for label, ms in zip(PHASES, phases))
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
