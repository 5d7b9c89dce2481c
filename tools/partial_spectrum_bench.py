#!/usr/bin/env python3
"""Atom-group decomposition costs (profiles/partial_spectra.txt):
  increments  PotGNN.calc_group_increments_device on config 3's structure (rocksalt, 256 atoms, P = 4) at
              Fn = Fe = 64 and at the documented 5 / 14, float32 and float64, groups = "species"; frames / s
  spectra     DevicePartialMDRamanSpectrum.measure_polarized (rn_md_raman_partial_device, the intensities copied to
              pageable host memory and unpacked to [K,G,G,bins]) on random increments in HBM, G in {2, 4, 16},
              K in {1, 64}
One warm-up call per case; a device synchronise precedes every clock read; the best of --reps calls.

Usage: python tools/partial_spectrum_bench.py [--frames 256] [--steps 1000000] [--reps 3] [--out profiles/partial_spectra.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch  # before the HIP library: one HIP runtime per process (torch's)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import make_workload  # noqa: E402
from ramannoodle_amd.spectrum import DevicePartialMDRamanSpectrum  # noqa: E402


def best_of(fn, reps):
    fn()
    best = float("inf")
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partial_spectra.txt"))
    args = ap.parse_args()
    torch.cuda.init()
    lines = [f"# device: {torch.cuda.get_device_name(0)}; best of {args.reps} calls after one warm-up"]

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    for hparams, label in (("perf", "Fn = Fe = 64"), ("parity", "Fn = 5, Fe = 14")):
        wl = make_workload(num_cells=(4, 4, 2), frames=args.frames, hparams=hparams)
        model = wl["model"](device=0).eval()
        positions = torch.tensor(wl["positions"], dtype=torch.float64, device="cuda:0")
        for float64 in (False, True):
            out = model.calc_group_increments_device(positions, "species", float64=float64)
            seconds = best_of(lambda: model.calc_group_increments_device(positions, "species", float64=float64,
                                                                         out=out), args.reps)
            emit(f"increments  {wl['num_atoms']} atoms  {label:16s} {'float64' if float64 else 'float32'}  "
                 f"{args.frames} frames: {seconds * 1e3:8.1f} ms  {args.frames / seconds:8.0f} frames/s  "
                 f"({seconds / args.frames * 1e3:.3f} ms/frame)")
        del model, positions

    rng = np.random.default_rng(0)
    e_i = np.eye(3)[rng.integers(0, 3, size=64)] + 0.1
    e_s = np.eye(3)[rng.integers(0, 3, size=64)] - 0.1
    for groups in (2, 4, 16):
        for k in (1, 64):
            steps = args.steps
            # the output is K G (G+1) / 2 bins doubles (packed) plus K G^2 bins (unpacked): keep it below ~8 GB
            while k * groups * groups * (steps // 2) * 8 > 8e9:
                steps //= 10
            incr = torch.randn((steps - 1, groups, 3, 3), dtype=torch.float64, device="cuda:0")
            incr = incr + incr.transpose(2, 3)
            spectrum = DevicePartialMDRamanSpectrum(incr.contiguous(), 1.0)
            try:
                seconds = best_of(lambda: spectrum.measure_polarized(e_i[:k], e_s[:k]),
                                  1 if k * groups > 64 else args.reps)
            except MemoryError as exc:
                emit(f"spectrum    S = {steps:8d}  G = {groups:2d}  K = {k:2d}: does not fit the default 4 GiB "
                     f"workspace ({exc})")
                continue
            emit(f"spectrum    S = {steps:8d}  G = {groups:2d}  K = {k:2d}: {seconds * 1e3:9.1f} ms  "
                 f"({k * groups * (groups + 1) // 2} rows of {steps // 2 - 1} bins)")
            del spectrum, incr
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
