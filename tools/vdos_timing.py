#!/usr/bin/env python3
"""The vibrational density of states of an MD run on the GPU (profiles/vdos.txt): N atoms x S frames of positions in
HBM, G groups.
  (a) whole    DeviceVibrationalDensityOfStates.measure(): one boxcar segment of S frames
  (b) Welch    measure_segments(W, hop = W // 2, "hann", average=True)
  (c) host     the numpy path of (a) and (b) on --threads threads (scipy / numpy FFTs are single-threaded: the thread
               count bounds the BLAS and OpenMP pools only, as it would for a user)
One warm-up call of each path (plans, buffers); a device synchronise precedes every clock read; the median and the range
of --reps timed calls.  Then, with rn_md_vdos_set_profiling(1), the HIP-event times of the phases of --reps more calls
(median of each phase) and the bytes each kernel must move, computed from the shapes:
  builder   24 N (n + 1) Q read (every frame of every segment once) + 16 * 3 N L Q written
  power     16 * 3 N L Q read + 16 G L written per launch that owns the rows
over the phase time, against the HBM peak BASELINE.md assumes (8 TB/s).  The FFT phase is hipFFT's; its bytes are not
modelled.  Event times include the launch gaps inside a phase when a call needs many blocks.

Usage: python tools/vdos_timing.py [--atoms 256] [--steps 10000] [--groups 3] [--width 2048] [--reps 7] [--threads 16]
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
from ramannoodle_amd.spectrum import DeviceVibrationalDensityOfStates, segment_plan  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s


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
    lib.rn_md_vdos_set_profiling(1)
    rows = []
    try:
        for _ in range(reps):
            fn()
            millis = (C.c_double * 4)()
            lib.rn_md_vdos_phase_times(millis)
            rows.append(list(millis))
    finally:
        lib.rn_md_vdos_set_profiling(0)
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
    ap.add_argument("--groups", type=int, default=3)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default="", help="also write the lines to this file (profiles/vdos.txt quotes them)")
    args = ap.parse_args()
    torch.set_num_threads(args.threads)
    torch.cuda.init()
    rng = np.random.default_rng(0)
    atoms, steps, groups = args.atoms, args.steps, args.groups
    walk = np.cumsum(0.01 * rng.normal(size=(steps, atoms, 3)), axis=0)
    positions = (rng.random((atoms, 3)) + walk) % 1.0
    lattice = np.array([[15.6, 0.0, 0.0], [0.4, 15.2, 0.0], [-0.3, 0.2, 16.1]])
    masses = rng.uniform(1.0, 100.0, atoms)
    labels = np.arange(atoms) % groups
    vdos = DeviceVibrationalDensityOfStates(torch.tensor(positions, device="cuda"), 1.0, lattice, masses, labels, groups)
    width, hop, _ = segment_plan(steps, args.width, None, "hann")
    segments = (steps - width) // hop + 1
    lines = [f"device: {torch.cuda.get_device_name(0)}; ROCm {torch.version.hip}; float64; N = {atoms} atoms, S = {steps} "
             f"frames, G = {groups}; Welch W = {width}, hop {hop}, Q = {segments}; median [min .. max] of {args.reps} "
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
        series = 16.0 * 3 * atoms * length * count
        moved = {"builder": 24.0 * atoms * (n + 1) * count + series, "power": series + 16.0 * groups * length}
        lines.append(f"{name:5s} phases (HIP events, median): builder {ms[0]:.3f} ms, forward FFTs {ms[1]:.3f} ms, power "
                     f"{ms[2]:.3f} ms, back half and copies {ms[3]:.3f} ms")
        for kernel, index in (("builder", 0), ("power", 2)):
            rate = moved[kernel] / (1e-3 * ms[index])
            lines.append(f"{name:5s} {kernel:7s} {moved[kernel] / 1e6:9.1f} MB in {ms[index]:.3f} ms = {rate / 1e12:.3f} TB/s "
                         f"= {100.0 * rate / HBM_PEAK:.1f} % of the 8 TB/s HBM peak")
        print("\n".join(lines[-3:]), flush=True)
        if not args.no_host:
            want, text = timed(lambda: call(host=True), max(1, args.reps // 3))
            lines.append(f"{name:5s} host ({args.threads} threads) {text}   max rel diff device - host "
                         f"{np.abs(got - want).max() / np.abs(want).max():.1e}")
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
