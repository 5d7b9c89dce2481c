#!/usr/bin/env python3
"""The band moments on the GPU (profiles/band_modes.txt).  First the device - host differences of the shapes of
tests/test_band_modes_gpu.py, which its tolerance comes from.  Then two shapes, float64, with alpha (K' = 3N + 6 columns)
and 16 weight rows [bw; bw nu] of 8 bands of --band-bins bins:
  whole     N atoms x T frames, the whole run as one boxcar segment                      (--atoms 256 --frames 25001)
  runs      8 runs of W = 4097 frames of the same atoms, each one boxcar segment         (--runs 8 --width 4097)
For each:
  (a) HBM     band_moments_device() of tensors already in HBM (rn_bm_moments_device)
  (b) host    band_moments_device() of host arrays (rn_bm_moments: positions and alpha are copied to the device first)
  (c) numpy   band_moments_host() on --threads threads (one FFT per segment, two products per weight row)
One warm-up call of each device path (buffers); a device synchronise precedes every clock read; the median and the range
of --reps timed calls (numpy: --host-reps).  Then, with rn_bm_set_profiling(1), the HIP-event times of the four phases of
--reps more calls of (a) (median of each phase) and the flops of the two products, computed from the shapes, not counted
by the hardware, padding included (the matrix pipe does that work):
  transform  2 x Rp x Kp x 16 ceil(n / 16) per segment          (Rp, Kp: 2 U rows and K' columns padded to 64)
  update     2 x 64 x 64 x (segments x Rp) per pair of 64-column tiles of the lower triangle and weight row
over the phase time (the update's phase holds the sums over the chunks as well), against the float64 matrix peak
csrc/kernels_gemm.hip quotes (78 TFLOP/s).  The useful flops, 2 x 2 U x K' x n and 2 x B x 2 U x K'^2 / 2 per segment, are
given beside them.
The share of the transform spent making its first operand: the transform's phase time of a build variant whose operand
is a constant,
  RN_BUILD_TAG=bmconst RN_EXTRA_FLAGS=-DRN_BM_CONSTANT_OPERAND ramannoodle_amd/csrc/build.sh
measured by this tool in a child process of its own (--phases-only, RN_POTGNN_LIB=the variant); without that library the
line says so.

Usage: python tools/band_modes_timing.py [--atoms 256] [--frames 25001] [--runs 8] [--width 4097] [--band-bins 25]
                                         [--reps 7] [--host-reps 1] [--threads 16] [--no-host] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch  # before the HIP library: one HIP runtime per process (torch's)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ramannoodle_amd import _lib  # noqa: E402
from ramannoodle_amd.bandmodes import band_moments_device, band_moments_host  # noqa: E402

F64_MATRIX_PEAK = 78.0e12  # flop/s (csrc/kernels_gemm.hip)
TILE, K_TILE = 64, 16
VARIANT = os.path.join(ROOT, "ramannoodle_amd", "librn_potgnn_bmconst.so")
LATTICE = np.array([[15.6, 0.0, 0.0], [0.4, 15.2, 0.0], [-0.3, 0.2, 16.1]])


def timed(fn, reps, warm=True):
    out = fn() if warm else None
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return out, f"{np.median(times):9.2f} ms [{min(times):.2f} .. {max(times):.2f}]"


def phases(fn, reps):
    lib = _lib.load()
    lib.rn_bm_set_profiling(1)
    rows = []
    try:
        for _ in range(reps):
            fn()
            millis = (C.c_double * 4)()
            lib.rn_bm_phase_times(millis)
            rows.append(list(millis))
    finally:
        lib.rn_bm_set_profiling(0)
    return np.median(np.array(rows), axis=0)


def test_shape_differences(lines):
    from tests import test_band_modes_gpu as tests
    from tests.band_modes_cases import CASES, PHASE_CASE, LATTICE as cell, device_case, host_moments, moment_error, weight_sets
    worst = 0.0
    for name in CASES:
        positions, masses, alpha, width, starts, taper = device_case(name)
        for with_alpha in (False, True):
            for weights_name, weights in weight_sets(tests._bins(width)).items():
                got = band_moments_device(positions, cell, masses, alpha if with_alpha else None, width, starts, taper,
                                          weights)
                error = moment_error(got, host_moments(name, with_alpha, weights_name))
                worst = max(worst, error)
                lines.append(f"  {name:34s} alpha {int(with_alpha)}  {weights_name:24s} {error:.3e}")
    positions, masses, alpha, width, starts, taper = device_case(PHASE_CASE)
    bins = tests._bins(width)
    weights = np.zeros((2, bins))
    weights[0, [0, 4999]] = 1.0
    weights[1, [4999, bins - 1]] = (0.5, 1.5)
    for with_alpha in (False, True):
        arguments = (positions, cell, masses, alpha if with_alpha else None, width, starts, taper, weights)
        error = moment_error(band_moments_device(*arguments), band_moments_host(*arguments))
        worst = max(worst, error)
        lines.append(f"  {PHASE_CASE:34s} alpha {int(with_alpha)}  {'bins 1, 5000, 10000':24s} {error:.3e}")
    lines.append(f"  worst: {worst:.3e} (the test tolerance is 20 x this)")


def shape(tag, positions, alpha, masses, width, starts, band_bins, args, lines):
    steps = width - 1
    bins = (steps + 1) // 2 - 1
    taper = np.ones(steps)
    axis = np.arange(1, bins + 1) * (33356.40951981521 / steps)
    plain = np.zeros((8, bins))
    for b in range(8):
        first = (b + 1) * bins // 10
        plain[b, first:first + band_bins] = 1.0
    weights = np.concatenate([plain, plain * axis[None, :]])
    active = int((weights != 0).any(axis=0).sum())
    columns = positions.shape[1] * 3 + 6
    segments = len(starts)
    d_positions = torch.tensor(positions, dtype=torch.float64, device="cuda")
    d_alpha = torch.tensor(alpha, dtype=torch.float64, device="cuda")
    call = lambda p, a: band_moments_device(p, LATTICE, masses, a, width, starts, taper, weights)  # noqa: E731
    if args.phases_only:
        call(d_positions, d_alpha)
        return [float(v) for v in phases(lambda: call(d_positions, d_alpha), args.reps)]
    lines.append(f"{tag}: {positions.shape[1]} atoms, {len(positions)} frames, {segments} segment(s) of W = {width}, K' = "
                 f"{columns} columns, 8 bands of {band_bins} bins (U = {active} bins, {2 * active} rows), 16 weight rows")
    got, text = timed(lambda: call(d_positions, d_alpha), args.reps)
    lines.append(f"  device, positions and alpha in HBM   {text}")
    print("\n".join(lines[-2:]), flush=True)
    same, text = timed(lambda: call(positions, alpha), args.reps)
    lines.append(f"  device, positions and alpha on host  {text}   bit-identical to the HBM entry: {np.array_equal(got, same)}")
    print(lines[-1], flush=True)
    ms = phases(lambda: call(d_positions, d_alpha), args.reps)
    padded_rows, padded_columns = -(-2 * active // TILE) * TILE, -(-columns // TILE) * TILE
    tiles = padded_columns // TILE
    transform = 2.0 * padded_rows * padded_columns * K_TILE * -(-steps // K_TILE) * segments
    update = 2.0 * TILE * TILE * segments * padded_rows * (tiles * (tiles + 1) // 2) * len(weights)
    useful = (2.0 * 2 * active * columns * steps * segments, 2.0 * len(weights) * 2 * active * columns * columns / 2 * segments)
    lines.append(f"  phases of the HBM entry (HIP events, median): copies in and phase table {ms[0]:.3f} ms, transform "
                 f"{ms[1]:.3f} ms, update and sums over the chunks {ms[2]:.3f} ms, copy out {ms[3]:.3f} ms")
    for name, issued, good, span in (("transform", transform, useful[0], ms[1]), ("update", update, useful[1], ms[2])):
        rate = issued / (1e-3 * span)
        lines.append(f"  {name:9s} {issued / 1e9:9.2f} GFLOP issued (computed; {good / 1e9:.2f} GFLOP useful) in {span:.3f} ms = "
                     f"{rate / 1e12:.2f} TFLOP/s = {100.0 * rate / F64_MATRIX_PEAK:.1f} % of the 78 TFLOP/s float64 matrix peak")
    print("\n".join(lines[-3:]), flush=True)
    constant = args.constant.get(tag)
    if constant is None:
        lines.append("  transform with a constant first operand: not measured (no librn_potgnn_bmconst.so)")
    else:
        lines.append(f"  transform with a constant first operand (the variant build, a process of its own): {constant[1]:.3f} ms "
                     f"against {ms[1]:.3f} ms: making the operand costs {100.0 * (1.0 - constant[1] / ms[1]):.0f} % of the "
                     "transform")
    print(lines[-1], flush=True)
    if not args.no_host:
        want, text = timed(lambda: band_moments_host(positions, LATTICE, masses, alpha, width, starts, taper, weights),
                           args.host_reps, warm=False)
        from tests.band_modes_cases import moment_error
        lines.append(f"  numpy ({args.threads} threads)                   {text}   device - host, each entry relative to "
                     f"sqrt(want_jj want_ll): {moment_error(got, want):.1e}")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=256)
    ap.add_argument("--frames", type=int, default=25_001)
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--width", type=int, default=4097)
    ap.add_argument("--band-bins", type=int, default=25)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-shapes", action="store_true", help="skip the differences of the test shapes")
    ap.add_argument("--phases-only", action="store_true", help="print the phase times of both shapes as JSON and stop")
    ap.add_argument("--out", default="", help="also write the lines to this file (profiles/band_modes.txt quotes them)")
    args = ap.parse_args()
    torch.set_num_threads(args.threads)
    torch.cuda.init()
    lines = [f"device: {torch.cuda.get_device_name(0)}; ROCm {torch.version.hip}; float64; median [min .. max] of {args.reps} "
             f"calls after a warm-up (numpy: {args.host_reps} call(s), no warm-up)"]
    print(lines[-1], flush=True)
    if not args.no_shapes and not args.phases_only:
        lines.append("device - host differences of the shapes of tests/test_band_modes_gpu.py (each entry relative to "
                     "sqrt(want_jj want_ll)):")
        test_shape_differences(lines)
        print("\n".join(lines[-120:]), flush=True)
    rng = np.random.default_rng(0)
    atoms = args.atoms
    masses = rng.uniform(1.0, 100.0, atoms)

    def run(frames):
        positions = (rng.random((1, atoms, 3)) + 0.01 * rng.normal(size=(frames, atoms, 3))) % 1.0
        return positions, np.cumsum(0.01 * rng.normal(size=(frames, 3, 3)), axis=0)

    args.constant = {}
    if not args.phases_only and os.path.exists(VARIANT):
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--phases-only", "--atoms", str(atoms), "--frames",
                                str(args.frames), "--runs", str(args.runs), "--width", str(args.width), "--band-bins",
                                str(args.band_bins), "--reps", str(args.reps)],
                               env={**os.environ, "RN_POTGNN_LIB": VARIANT}, capture_output=True, text=True)
        found = re.search(r"PHASES (\{.*\})", child.stdout)
        if found:
            args.constant = json.loads(found.group(1))
    positions, alpha = run(args.frames)
    whole = shape("whole", positions, alpha, masses, args.frames, np.array([0], dtype=np.int64), args.band_bins, args, lines)
    positions, alpha = run(args.runs * args.width)
    starts = np.arange(args.runs, dtype=np.int64) * args.width
    runs = shape("runs", positions, alpha, masses, args.width, starts, args.band_bins, args, lines)
    if args.phases_only:
        print("PHASES " + json.dumps({"whole": whole, "runs": runs}), flush=True)
        return
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
