#!/usr/bin/env python3
"""The mode-by-mode interference matrix of MD Raman bands on the GPU (profiles/mode_matrix.txt): C = 3N + 1 channels of
increments in HBM for the benchmark's 256-atom cell (768 modes and the rest), segments of W = 4097 frames, B = 3 bands,
K = 1 configuration (measure_interference).  The increments are seeded random numbers made on the device: the
reducer's arithmetic does not depend on the values, and 4097 frames through the model would take a minute.
  (a) matrix    DeviceModeMDRamanSpectrum.measure_interference: the call, and the HIP-event times of its phases
                (rn_md_raman_mode_matrix_phase_times).  The product's flops are computed from the shapes (the tile
                pairs of the upper triangle, 64 x 64 x 12 x 2 per frequency of the padded half-spectrum, per segment,
                band and configuration; the kernel runs a few more when the channels go through in blocks), not
                counted by the hardware, against the float64 matrix peak csrc/kernels_gemm.hip quotes
  (b) select    the only other route to the same numbers: select() of 15 channels and the atom-group pair reducer's
                segment mean (DevicePartialMDRamanSpectrum.measure_segments), timed, and multiplied by the least number
                of such calls that could cover all pairs of channels, ceil(C (C - 1) / 2 / 105): a figure computed from
                one call, not a measurement of them all
One warm-up call of each path; a device synchronise precedes every clock read; the median and the range of --reps calls.

Usage: python tools/mode_matrix_timing.py [--atoms 256] [--width 4097] [--segments 1] [--reps 5] [--out FILE]
"""
import argparse
import ctypes as C
import math
import os
import sys
import time

import numpy as np
import torch  # before the HIP library: one HIP runtime per process (torch's)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ramannoodle_amd import _lib  # noqa: E402
from ramannoodle_amd.spectrum import MAX_SELECTED, DeviceModeMDRamanSpectrum  # noqa: E402

F64_MATRIX_PEAK = 78.0e12  # flop/s (csrc/kernels_gemm.hip)
TILE, FREQS = 64, 4        # csrc/spectrum_mode_matrix.hip


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


def phases(fn, reps):
    lib = _lib.load()
    lib.rn_md_raman_mode_matrix_set_profiling(1)
    rows = []
    try:
        for _ in range(reps):
            fn()
            millis = (C.c_double * 4)()
            lib.rn_md_raman_mode_matrix_phase_times(millis)
            rows.append(list(millis))
    finally:
        lib.rn_md_raman_mode_matrix_set_profiling(0)
    return np.median(np.array(rows), axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=256)
    ap.add_argument("--width", type=int, default=4097)
    ap.add_argument("--segments", type=int, default=1, help="segments, half a segment apart")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="", help="also write the lines to this file (profiles/mode_matrix.txt quotes them)")
    args = ap.parse_args()
    torch.cuda.init()
    channels, width, hop = 3 * args.atoms + 1, args.width, args.width // 2
    steps = width - 1 + hop * (args.segments - 1)
    generator = torch.Generator(device="cuda:0").manual_seed(0)
    increments = torch.randn((steps, channels, 3, 3), dtype=torch.float64, device="cuda:0", generator=generator)
    spectrum = DeviceModeMDRamanSpectrum(increments, 1.0)
    wavenumbers, _ = DeviceModeMDRamanSpectrum(increments[:, :1].contiguous(), 1.0).measure_segments(width, hop)
    third = len(wavenumbers) // 3
    bands = np.array([[wavenumbers[0], wavenumbers[third]], [wavenumbers[third], wavenumbers[2 * third]],
                      [wavenumbers[2 * third], 2 * wavenumbers[-1]]])
    lines = [f"device: {torch.cuda.get_device_name(0)}; ROCm {torch.version.hip}; float64; N = {args.atoms} atoms, C = "
             f"{channels} channels, {args.segments} segment(s) of W = {width} frames (L = {2 * (width - 1)}), B = 3 bands of "
             f"about {third} bins, K = 1; median [min .. max] of {args.reps} calls after a warm-up"]

    def matrix():
        return spectrum.measure_interference(bands, width, hop)[1]

    out, call_ms, text = timed(matrix, args.reps)
    ms = phases(matrix, args.reps)
    lines.append(f"measure_interference -> A{list(out.shape)} {text}")
    lines.append(f"phases (HIP events, median): builder {ms[0]:.3f} ms, forward FFTs {ms[1]:.3f} ms, product "
                 f"{ms[2]:.3f} ms, copies {ms[3]:.3f} ms; the rest of the call is the host's (the frequency weights, the "
                 "uploads, the mirror)")
    tiles = -(-channels // TILE)
    length = 1 << math.ceil(math.log2(2 * (width - 1) - 1))
    padded = -(-(length // 2 + 1) // FREQS) * FREQS
    flops = 3.0 * (tiles * (tiles + 1) // 2) * TILE * TILE * 12 * 2 * padded * args.segments
    rate = flops / (1e-3 * ms[2])
    lines.append(f"product {flops / 1e9:.2f} GFLOP (computed: {tiles * (tiles + 1) // 2} tile pairs) = {rate / 1e12:.2f} "
                 f"TFLOP/s = {100.0 * rate / F64_MATRIX_PEAK:.1f} % of the 78 TFLOP/s float64 matrix peak")
    print("\n".join(lines), flush=True)

    def select():
        return spectrum.select(np.arange(MAX_SELECTED)).measure_segments(width, hop)[1]

    _, select_ms, text = timed(select, args.reps)
    pairs_per_call = MAX_SELECTED * (MAX_SELECTED - 1) // 2
    calls = -(-(channels * (channels - 1) // 2) // pairs_per_call)
    lines.append(f"select({MAX_SELECTED} channels) + the pair reducer's segment mean, one call {text}")
    lines.append(f"all pairs that way: at least {calls} calls ({pairs_per_call} pairs a call) x {select_ms:.2f} ms = "
                 f"{1e-3 * calls * select_ms:.1f} s (computed from the one call), {calls * select_ms / call_ms:.0f} x the "
                 "matrix call; and it would return every bin, which the matrix sums")
    print("\n".join(lines[-2:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
