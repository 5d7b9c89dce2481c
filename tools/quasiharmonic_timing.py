#!/usr/bin/env python3
"""The covariance moments of quasi-harmonic mode analysis on the GPU (profiles/quasiharmonic_modes.txt): N atoms x T
frames of positions (a jitter about random sites, so that the minimum image acts at the cell faces), for each of
--blocks:
  (a) HBM     moments_device() of a tensor already in HBM (rn_qh_moments_device)
  (b) host    moments_device() of a host array (rn_qh_moments: the positions are copied to the device first)
  (c) numpy   moments_host() on --threads threads (two BLAS rank-updates per block)
One warm-up call of each path (buffers); a device synchronise precedes every clock read; the median and the range of
--reps timed calls.  Then, with rn_qh_set_profiling(1), the HIP-event times of the four phases of --reps more calls of (a)
(median of each phase) and the flops of the two rank updates, computed from the shapes, not counted by the hardware:
  2 series x 2 x 64 x 64 flops per frame of a k-tile of 16 frames, for each pair of 64-column tiles of the lower triangle
  and each k-tile of every chunk (the padding of the last k-tile of a chunk and of the last tile of 3N is counted: the
  matrix pipe does that work), over the phase time, against the float64 matrix peak csrc/kernels_gemm.hip quotes
  (78 TFLOP/s).  The useful flops, 2 series x 2 x 3N x 3N x T of the full matrices, are given beside them.
Then numpy.linalg.eigh of a 3N x 3N covariance (the host half of modes_from_moments), and the device - host differences
of the test shapes of tests/test_quasiharmonic_gpu.py, which its tolerances come from.

Usage: python tools/quasiharmonic_timing.py [--atoms 256] [--frames 10000] [--blocks 1 8] [--reps 7] [--threads 16]
                                            [--no-host] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch  # before the HIP library: one HIP runtime per process (torch's)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ramannoodle_amd import _lib  # noqa: E402
from ramannoodle_amd.quasiharmonic import (chunk_frames, modes_from_moments, moments_device, moments_host,  # noqa: E402
                                           pool_moments, run_blocks)

F64_MATRIX_PEAK = 78.0e12  # flop/s (csrc/kernels_gemm.hip)
TILE, K_TILE = 64, 16


def timed(fn, reps):
    out = fn()  # warm-up
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
    lib.rn_qh_set_profiling(1)
    rows = []
    try:
        for _ in range(reps):
            fn()
            millis = (C.c_double * 4)()
            lib.rn_qh_phase_times(millis)
            rows.append(list(millis))
    finally:
        lib.rn_qh_set_profiling(0)
    return np.median(np.array(rows), axis=0)


def issued_flops(columns, bounds):
    tiles = -(-columns // TILE)
    pairs = tiles * (tiles + 1) // 2
    chunk = chunk_frames()
    k_tiles = 0
    for lo, hi in zip(bounds, bounds[1:]):
        frames = int(hi - lo)
        k_tiles += (frames // chunk) * (chunk // K_TILE) + -(-(frames % chunk) // K_TILE)
    return 2.0 * 2.0 * TILE * TILE * K_TILE * k_tiles * pairs


def test_shape_differences(lines):
    from tests.quasiharmonic_cases import moment_differences
    from tests import test_quasiharmonic_gpu as cases
    worst = [0.0, 0.0]
    for name in cases.CASES:
        positions, anchor, bounds, joined, want = cases._case(name)
        first, second = moment_differences(moments_device(positions, anchor, bounds, joined), want)
        worst = [max(worst[0], first), max(worst[1], second)]
        lines.append(f"  {name:48s} first {first:.3e}   second {second:.3e}")
    positions, anchor, bounds, joined, want = cases._case("a chunk and a frame")
    frames = bounds[-1]
    pooled_want = [array[None] for array in pool_moments(*want)]
    for cut in ([0, frames], [0, 100, 300, frames], [0, 1, frames - 1, frames], [0, 16, 32, 48, frames]):
        flags = [1] * (len(cut) - 2) + [0]
        pooled = [array[None] for array in pool_moments(*moments_device(positions, anchor, cut, flags))]
        first, second = moment_differences(pooled, pooled_want)
        worst = [max(worst[0], first), max(worst[1], second)]
        lines.append(f"  {'pooled, blocks ' + str(cut):48s} first {first:.3e}   second {second:.3e}")
    lines.append(f"  worst: first {worst[0]:.3e}, second {worst[1]:.3e} (the test tolerances are 20 x these)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=256)
    ap.add_argument("--frames", type=int, default=10_000)
    ap.add_argument("--blocks", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default="", help="also write the lines to this file (profiles/quasiharmonic_modes.txt quotes them)")
    args = ap.parse_args()
    torch.set_num_threads(args.threads)
    torch.cuda.init()
    rng = np.random.default_rng(0)
    atoms, frames = args.atoms, args.frames
    columns = 3 * atoms
    positions = (rng.random((1, atoms, 3)) + 0.01 * rng.normal(size=(frames, atoms, 3))) % 1.0
    anchor = positions[0]
    tensor = torch.tensor(positions, dtype=torch.float64, device="cuda")
    lattice = np.array([[15.6, 0.0, 0.0], [0.4, 15.2, 0.0], [-0.3, 0.2, 16.1]])
    masses = rng.uniform(1.0, 100.0, atoms)
    lines = [f"device: {torch.cuda.get_device_name(0)}; ROCm {torch.version.hip}; float64; N = {atoms} atoms (3N = {columns}), "
             f"T = {frames} frames; chunks of {chunk_frames()} frames; median [min .. max] of {args.reps} calls after a "
             "warm-up"]
    print(lines[-1], flush=True)
    got = None
    for blocks in args.blocks:
        bounds, joined = run_blocks([frames], blocks)
        tag = f"blocks = {blocks}"
        got, text = timed(lambda: moments_device(tensor, anchor, bounds, joined), args.reps)
        lines.append(f"{tag:11s} device, positions in HBM   {text}")
        print(lines[-1], flush=True)
        same, text = timed(lambda: moments_device(positions, anchor, bounds, joined), args.reps)
        identical = all(np.array_equal(a, b) for a, b in zip(got, same))
        lines.append(f"{tag:11s} device, positions on host  {text}   bit-identical to the HBM entry: {identical}")
        print(lines[-1], flush=True)
        ms = phases(lambda: moments_device(tensor, anchor, bounds, joined), args.reps)
        issued, useful = issued_flops(columns, bounds), 2.0 * 2.0 * columns * columns * frames
        rate = issued / (1e-3 * ms[1])
        lines.append(f"{tag:11s} phases of the HBM entry (HIP events, median): copies in {ms[0]:.3f} ms, rank updates "
                     f"{ms[1]:.3f} ms, sums over the chunks {ms[2]:.3f} ms, copies out {ms[3]:.3f} ms")
        lines.append(f"{tag:11s} rank updates {issued / 1e9:9.2f} GFLOP issued (computed; {useful / 1e9:.2f} GFLOP of the full "
                     f"matrices) in {ms[1]:.3f} ms = {rate / 1e12:.2f} TFLOP/s = {100.0 * rate / F64_MATRIX_PEAK:.1f} % of the "
                     "78 TFLOP/s float64 matrix peak")
        print("\n".join(lines[-2:]), flush=True)
        if not args.no_host:
            want, text = timed(lambda: moments_host(positions, anchor, bounds, joined), args.reps)
            second = max(np.abs(got[1][b, s] - want[1][b, s]).max() / np.abs(want[1][b, s]).max()
                         for b in range(blocks) for s in range(2))
            lines.append(f"{tag:11s} numpy ({args.threads} threads)         {text}   max rel diff of a second matrix device - "
                         f"host {second:.1e}")
            print(lines[-1], flush=True)
    first, second, counts = pool_moments(*got)
    covariance = second[0] / counts[0] - np.outer(first, first) / counts[0] ** 2
    _, text = timed(lambda: np.linalg.eigh(covariance), args.reps)
    lines.append(f"numpy.linalg.eigh of {columns} x {columns} ({args.threads} threads) {text}")
    _, text = timed(lambda: modes_from_moments(*got, lattice, masses, 1.0), args.reps)
    lines.append(f"modes_from_moments of the last moments (host: metric, eigh, per-block quotients) {text}")
    print("\n".join(lines[-2:]), flush=True)
    lines.append("device - host differences of the shapes of tests/test_quasiharmonic_gpu.py (first: relative to sqrt(frames x "
                 "largest displacement-matrix entry); second: each matrix relative to its largest entry):")
    test_shape_differences(lines)
    print("\n".join(lines[-20:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
