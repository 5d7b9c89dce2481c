#!/usr/bin/env python3
"""The mode-projected VDOS of an MD run on the GPU (profiles/mode_vdos.txt): N atoms x S frames of positions in HBM,
M projection vectors (a random orthonormal set).
  (a) whole    DeviceModeVibrationalDensityOfStates.measure(): one boxcar segment of S frames
  (b) Welch    measure_segments(W, hop = W // 2, "hann", average=True)
  (c) host     the numpy path of (a) and (b) on --threads threads (the projection is a BLAS product and uses them; scipy
               / numpy FFTs are single-threaded)
One warm-up call of each path (plans, buffers); a device synchronise precedes every clock read; the median and the range
of --reps timed calls.  Then, with rn_md_mode_vdos_set_profiling(1), the HIP-event times of the phases of --reps more
calls (median of each phase) and the flops of the projection, computed from the shapes, not counted by the hardware:
  projection   2 n 3N M per segment (the product steps x 3N by 3N x M; the minimum image and the lattice are not counted)
over the phase time, against the float64 matrix peak csrc/kernels_gemm.hip quotes (78 TFLOP/s).  The FFT phase is
hipFFT's.  The shared driver launches the transforms and the back half itself, so a phase lasts from its first launch to
the next phase's: event times include the launch gaps inside a phase.

Usage: python tools/mode_vdos_timing.py [--atoms 256] [--steps 10000] [--modes 768] [--width 2048] [--reps 7]
                                        [--threads 16] [--no-host] [--out FILE]
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
from ramannoodle_amd.spectrum import DeviceModeVibrationalDensityOfStates, segment_plan  # noqa: E402

F64_MATRIX_PEAK = 78.0e12  # flop/s (csrc/kernels_gemm.hip)


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
    lib.rn_md_mode_vdos_set_profiling(1)
    rows = []
    try:
        for _ in range(reps):
            fn()
            millis = (C.c_double * 4)()
            lib.rn_md_mode_vdos_phase_times(millis)
            rows.append(list(millis))
    finally:
        lib.rn_md_mode_vdos_set_profiling(0)
    return np.median(np.array(rows), axis=0)


def padded_length(n):
    length = 1
    while length < 2 * n - 1:
        length <<= 1
    return length


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10_000)
    ap.add_argument("--modes", type=int, default=768)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default="", help="also write the lines to this file (profiles/mode_vdos.txt quotes them)")
    args = ap.parse_args()
    torch.set_num_threads(args.threads)
    torch.cuda.init()
    rng = np.random.default_rng(0)
    atoms, steps, modes = args.atoms, args.steps, args.modes
    walk = np.cumsum(0.01 * rng.normal(size=(steps, atoms, 3)), axis=0)
    positions = (rng.random((atoms, 3)) + walk) % 1.0
    lattice = np.array([[15.6, 0.0, 0.0], [0.4, 15.2, 0.0], [-0.3, 0.2, 16.1]])
    masses = rng.uniform(1.0, 100.0, atoms)
    basis, _ = np.linalg.qr(rng.normal(size=(3 * atoms, 3 * atoms)))
    vectors = np.ascontiguousarray(basis.T[:modes].reshape(modes, atoms, 3))
    vdos = DeviceModeVibrationalDensityOfStates(torch.tensor(positions, device="cuda"), 1.0, lattice, vectors, masses)
    width, hop, _ = segment_plan(steps, args.width, None, "hann")
    segments = (steps - width) // hop + 1
    lines = [f"device: {torch.cuda.get_device_name(0)}; ROCm {torch.version.hip}; float64; N = {atoms} atoms, S = {steps} "
             f"frames, M = {modes}; Welch W = {width}, hop {hop}, Q = {segments}; median [min .. max] of {args.reps} "
             "calls after a warm-up"]
    cases = (("whole", lambda **kw: vdos.measure(**kw)[1], steps, 1),
             ("Welch", lambda **kw: vdos.measure_segments(width, hop, "hann", True, **kw)[1], width, segments))
    for name, call, frames, count in cases:
        n = frames - 1
        length = padded_length(n)
        got, text = timed(call, args.reps)
        lines.append(f"{name:5s} device {text}   (L = {length})")
        print(lines[-1], flush=True)
        ms = phases(call, args.reps)
        flops = 2.0 * n * 3 * atoms * modes * count
        rate = flops / (1e-3 * ms[0])
        lines.append(f"{name:5s} phases (HIP events, median): projection {ms[0]:.3f} ms, forward FFTs {ms[1]:.3f} ms, power "
                     f"{ms[2]:.3f} ms, back half and copies {ms[3]:.3f} ms")
        lines.append(f"{name:5s} projection {flops / 1e9:9.2f} GFLOP (computed) in {ms[0]:.3f} ms = {rate / 1e12:.2f} TFLOP/s "
                     f"= {100.0 * rate / F64_MATRIX_PEAK:.1f} % of the 78 TFLOP/s float64 matrix peak")
        print("\n".join(lines[-2:]), flush=True)
        if not args.no_host:
            want, text = timed(lambda: call(host=True), max(1, args.reps // 3))
            error = (np.abs(got - want).max(axis=-1) / np.abs(want).max(axis=-1)).max()
            lines.append(f"{name:5s} host ({args.threads} threads) {text}   max rel diff of a row device - host {error:.1e}")
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
