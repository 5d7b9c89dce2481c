#!/usr/bin/env python3
"""Harmonic trajectories on the GPU (profiles/harmonic_trajectory.txt): N atoms, M = 3N modes, T frames, for each of
--runs:
  (a) HBM       synthesize_device(): the inputs uploaded, the kernel, the tensor left in HBM (rn_ht_synthesize_device)
  (b) download  synthesize_download(): the same and the positions copied into a host array (rn_ht_synthesize)
  (c) numpy     synthesize_host() on --threads threads
One warm-up call of each path; a device synchronise precedes every clock read; the median and the range of --reps timed
calls.  Then, with rn_ht_set_profiling(1), the HIP-event times of the phases of --reps more calls of (a) (median of each
phase) and the flops of the product, computed from the shapes, not counted by the hardware: 2 x 64 x 128 x 16 per k-tile
of 16 modes of a workgroup's 64 frames x 128 columns, padding included (the matrix pipe does that work), over the kernel
time, against the float64 matrix peak csrc/kernels_gemm.hip quotes (78 TFLOP/s).
The share of the kernel spent producing cosines: the kernel time of a build variant whose cosine is a constant,
  RN_BUILD_TAG=htconst RN_EXTRA_FLAGS=-DRN_HT_CONSTANT_COSINE ramannoodle_amd/csrc/build.sh
measured by this tool in a child process of its own (--kernel-only, RN_POTGNN_LIB=the variant); without that library the
line says so.  Then the device - host differences of the cases of tests/test_harmonic_trajectory_gpu.py next to their
bounds, the kernel's resources from the compiler (when hipcc is there), the ratio of the 2 omega line to the omega line
of the single-mode run of that file's last test at --temperatures, and one bench.py run (--bench).

Usage: python tools/harmonic_trajectory_timing.py [--atoms 256] [--frames 10000] [--runs 1 8] [--reps 7] [--threads 16]
                                                  [--no-host] [--bench] [--overtone-only] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys
import time

import numpy as np
import torch  # before the HIP library: one HIP runtime per process (torch's)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ramannoodle_amd import _lib, harmonic  # noqa: E402

F64_MATRIX_PEAK = 78.0e12  # flop/s (csrc/kernels_gemm.hip)
FRAMES, COLUMNS, MODES = 64, 128, 16  # a workgroup's tile and the k-tile of csrc/kernels_harmonic.hip
VARIANT = os.path.join(ROOT, "ramannoodle_amd", "librn_potgnn_htconst.so")


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
    lib.rn_ht_set_profiling(1)
    rows = []
    try:
        for _ in range(reps):
            fn()
            millis = (C.c_double * 3)()
            lib.rn_ht_phase_times(millis)
            rows.append(list(millis))
    finally:
        lib.rn_ht_set_profiling(0)
    return np.median(np.array(rows), axis=0)


def inputs(atoms, runs, seed=0):
    """Random sites, a random orthonormal basis of 3N modes scaled to a reach of 0.05, angles per frame in (0.01, 3)."""
    rng = np.random.default_rng(seed)
    columns = 3 * atoms
    ref = rng.random((atoms, 3))
    D, _ = np.linalg.qr(rng.normal(size=(columns, columns)))
    amp = rng.uniform(0.2, 1.0, size=(runs, columns))
    D *= 0.05 / (np.abs(amp)[:, :, None] * np.abs(D)[None]).sum(axis=1).max()
    return ref, np.ascontiguousarray(D), rng.uniform(0.01, 3.0, columns), amp, rng.uniform(0, 2 * np.pi, size=(runs, columns))


def issued_flops(columns, modes, frames, runs):
    tiles = -(-columns // COLUMNS) * -(-frames // FRAMES) * runs
    return 2.0 * FRAMES * COLUMNS * MODES * -(-modes // MODES) * tiles


def kernel_only(atoms, frames, runs, reps):
    """The median kernel time in ms of each of ``runs`` (the child process of the cosine-share measurement)."""
    torch.cuda.init()
    out = {}
    for count in runs:
        arguments = inputs(atoms, count)
        tensor = torch.empty((count, frames, atoms, 3), dtype=torch.float64, device="cuda")
        call = lambda: harmonic.synthesize_device(*arguments, frames, out=tensor)  # noqa: E731
        call()
        out[str(count)] = float(phases(call, reps)[1])
    print("KERNEL_MS " + json.dumps(out), flush=True)


def case_differences(lines):
    from tests.harmonic_cases import DEVICE_CASES, device_case, difference_bound, minimum_image
    for name in DEVICE_CASES:
        (ref, D, omega_dt, amp, phase), frames, first = device_case(name)
        want = harmonic.synthesize_host(ref, D, omega_dt, amp, phase, frames, first)
        got = harmonic.synthesize_device(ref, D, omega_dt, amp, phase, frames, first).cpu().numpy()
        difference = np.abs(minimum_image(got - want)).reshape(len(amp), frames, -1).max(axis=(0, 1))
        bound = difference_bound(amp, D)
        worst = int(np.argmax(difference / bound))
        lines.append(f"  {name:48s} difference {difference[worst]:.3e}   bound {bound[worst]:.3e}   ratio "
                     f"{difference[worst] / bound[worst]:.3f}")


def kernel_resources(lines):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    source = os.path.join(ROOT, "ramannoodle_amd", "csrc", "kernels_harmonic.hip")
    if not os.path.exists(hipcc):
        lines.append("  not taken: no hipcc here")
        return
    result = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c", source, "-o",
                             os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    found = dict(re.findall(r"remark:\s+([A-Za-z \[\]/]+): (\S+) \[-Rpass", result.stderr))
    if "VGPRs" not in found:
        lines.append(f"  not taken: hipcc gave no remarks (exit {result.returncode})")
        return
    lines.append(f"  harmonic_synthesis_kernel: {found['VGPRs']} VGPRs, {found['AGPRs']} AGPRs, {found['TotalSGPRs']} SGPRs, "
                 f"{found['ScratchSize [bytes/lane]']} B scratch per lane, {found['LDS Size [bytes/block]']} B LDS, "
                 f"{found['Occupancy [waves/SIMD]']} waves per SIMD")


def overtone_ratios(lines, temperatures, frames=1024):
    """The single-mode run of tests/test_harmonic_trajectory_gpu.py's last test: the strongest bin within one bin of
    2 omega over that of omega.  The wavenumbers make whole cycles in 1024 timesteps: with 1025 frames the 1024
    differences the spectrum is made of hold whole cycles, with the test's 1024 frames they do not."""
    from ramannoodle_amd.dynamics import Phonons
    from ramannoodle_amd.spectrum import _PER_FS_TO_CM1, DeviceMDRamanSpectrum
    from tests.conftest import load_golden
    from tests.harmonic_cases import mode_basis
    from tests.helpers import product_model_from_golden
    g = load_golden("triclinic20")
    model = product_model_from_golden(g).eval()
    lattice = np.asarray(g["lattice"], dtype=np.float64).reshape(3, 3)
    sites = np.asarray(g["positions"], dtype=np.float64)
    atoms, timestep = len(sites), 1.0
    rng = np.random.default_rng(8)
    masses = rng.uniform(1.0, 4.0, atoms)
    columns = 3 * atoms
    translations = np.sqrt(masses / masses.sum())[None, :, None] * np.eye(3)[:, None, :]
    vectors = np.concatenate([translations, mode_basis(masses, columns - 3, rng)])
    cycles = np.concatenate([[0, 0, 0], 30 + 5 * np.arange(columns - 3)])
    wavenumbers = cycles / (1024 * timestep) * _PER_FS_TO_CM1
    phonons = Phonons(sites, wavenumbers, np.ascontiguousarray((vectors / np.sqrt(masses)[None, :, None]) @ np.linalg.inv(lattice)))
    tensors = phonons.get_raman_spectrum(model).raman_tensors
    mode = int(np.argmax((tensors[3:] ** 2).sum(axis=(1, 2)))) + 3
    ref, D, omega_dt, selected, _ = harmonic.phonon_arguments(phonons, lattice, timestep, masses, modes=[mode])
    previous = None
    for temperature in temperatures:
        amp, phase = harmonic.draw(selected, temperature, "classical", "mean", 1, seed=0)
        tensor = harmonic.synthesize_device(ref, D, omega_dt, amp, phase, frames, device=model.device_index)[0]
        axis, intensities = DeviceMDRamanSpectrum(model.calc_polarizabilities_device(tensor), timestep).measure()
        width = axis[1] - axis[0]
        line = lambda w: intensities[np.abs(axis - w) <= width].max()  # noqa: E731
        ratio = line(2.0 * wavenumbers[mode]) / line(wavenumbers[mode])
        growth = "" if previous is None else f"   x {ratio / previous[1]:.2f} for T x {temperature / previous[0]:.0f}"
        lines.append(f"  {frames} frames, mode {mode} ({wavenumbers[mode]:.1f} 1/cm), {temperature:6.1f} K: I(2 omega) / I(omega) = {ratio:.4e}{growth}")
        previous = (temperature, ratio)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=256)
    ap.add_argument("--frames", type=int, default=10_000)
    ap.add_argument("--runs", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--temperatures", type=float, nargs="+", default=[10.0, 40.0, 160.0])
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--bench", action="store_true", help="also run python bench.py --gpus 1 --steps 3 --warmup 1")
    ap.add_argument("--overtone-only", action="store_true", help="the overtone ratios alone, at 1024 and 1025 frames")
    ap.add_argument("--kernel-only", action="store_true", help="print the kernel times alone (the variant's child process)")
    ap.add_argument("--out", default="", help="also write the lines to this file (profiles/harmonic_trajectory.txt quotes them)")
    args = ap.parse_args()
    torch.set_num_threads(args.threads)
    if args.kernel_only:
        kernel_only(args.atoms, args.frames, args.runs, args.reps)
        return
    torch.cuda.init()
    if args.overtone_only:
        lines = []
        for count in (1024, 1025):
            overtone_ratios(lines, args.temperatures, count)
        print("\n".join(lines), flush=True)
        return
    atoms, frames = args.atoms, args.frames
    columns = modes = 3 * atoms
    lines = [f"device: {torch.cuda.get_device_name(0)}; ROCm {torch.version.hip}; float64; N = {atoms} atoms (3N = {columns}), "
             f"M = {modes} modes, T = {frames} frames; median [min .. max] of {args.reps} calls after a warm-up"]
    print(lines[-1], flush=True)
    kernel_ms = {}
    for runs in args.runs:
        arguments = inputs(atoms, runs)
        tag = f"runs = {runs}"
        megabytes = runs * frames * columns * 8 / 1e6
        tensor = torch.empty((runs, frames, atoms, 3), dtype=torch.float64, device="cuda")
        call = lambda: harmonic.synthesize_device(*arguments, frames, out=tensor)  # noqa: E731
        _, text = timed(call, args.reps)
        lines.append(f"{tag:9s} device, left in HBM ({megabytes:.0f} MB)   {text}")
        print(lines[-1], flush=True)
        got = tensor.cpu().numpy()
        same, text = timed(lambda: harmonic.synthesize_download(*arguments, frames), args.reps)
        lines.append(f"{tag:9s} device, copied to the host    {text}   bit-identical to the HBM entry: {np.array_equal(got, same)}")
        print(lines[-1], flush=True)
        ms = phases(call, args.reps)
        kernel_ms[str(runs)] = float(ms[1])
        issued, useful = issued_flops(columns, modes, frames, runs), 2.0 * columns * modes * frames * runs
        rate = issued / (1e-3 * ms[1])
        lines.append(f"{tag:9s} phases of the HBM entry (HIP events, median): copies in {ms[0]:.3f} ms, kernel {ms[1]:.3f} ms "
                     f"({megabytes / ms[1]:.0f} GB/s of positions written)")
        lines.append(f"{tag:9s} kernel {issued / 1e9:9.2f} GFLOP issued (computed; {useful / 1e9:.2f} GFLOP without padding) in "
                     f"{ms[1]:.3f} ms = {rate / 1e12:.2f} TFLOP/s = {100.0 * rate / F64_MATRIX_PEAK:.1f} % of the 78 TFLOP/s "
                     "float64 matrix peak")
        print("\n".join(lines[-2:]), flush=True)
        if not args.no_host:
            want, text = timed(lambda: harmonic.synthesize_host(*arguments, frames), max(2, args.reps // 2))
            difference = np.abs(got - want)
            difference = np.minimum(difference, 1.0 - difference).max()
            lines.append(f"{tag:9s} numpy ({args.threads} threads)            {text}   max difference device - host {difference:.1e}")
            print(lines[-1], flush=True)
            del want
        del tensor, got, same
    if os.path.exists(VARIANT):
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernel-only", "--atoms", str(atoms), "--frames",
                                str(frames), "--reps", str(args.reps), "--runs", *map(str, args.runs)],
                               env={**os.environ, "RN_POTGNN_LIB": VARIANT}, capture_output=True, text=True)
        found = re.search(r"KERNEL_MS (\{.*\})", child.stdout)
        if found:
            for runs, constant in json.loads(found.group(1)).items():
                lines.append(f"runs = {runs}: kernel with a constant for the cosine {constant:.3f} ms against {kernel_ms[runs]:.3f} ms: "
                             f"the cosines take {100.0 * (1.0 - constant / kernel_ms[runs]):.0f} % of the kernel")
        else:
            lines.append(f"cosine share: not taken, the child process failed ({child.returncode}): {child.stderr[-300:]}")
    else:
        lines.append("cosine share: not taken, the constant-cosine variant librn_potgnn_htconst.so is not built")
    print("\n".join(lines[-len(args.runs):]), flush=True)
    lines.append("device - host differences of the cases of tests/test_harmonic_trajectory_gpu.py, after the minimum image, at "
                 "the column with the largest ratio to its bound 2 (M + 8) 2^-52 s_j + 2^-50:")
    start = len(lines)
    case_differences(lines)
    lines.append("the kernel, from the compiler (-Rpass-analysis=kernel-resource-usage):")
    kernel_resources(lines)
    lines.append("the single-mode run of the last test of tests/test_harmonic_trajectory_gpu.py (1024 frames of 1 fs, classical, "
                 "mean): proportionality of the ratio to T is expected; recorded, not asserted:")
    overtone_ratios(lines, args.temperatures)
    print("\n".join(lines[start - 1:]), flush=True)
    if args.bench:
        bench = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"],
                               capture_output=True, text=True, cwd=ROOT)
        rows = [row for row in bench.stdout.splitlines() if row.startswith("{")]
        lines.append("python bench.py --gpus 1 --steps 3 --warmup 1: " + (rows[-1] if rows else f"failed ({bench.returncode})"))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
