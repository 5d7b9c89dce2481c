#!/usr/bin/env python3
"""The phonon-mode projection of an MD Raman spectrum on the GPU (profiles/mode_raman.txt): the benchmark's rocksalt cell
(4 x 4 x 2: 256 atoms, the perf hyper-parameters), S frames of positions in HBM, M = 3N modes of a random orthonormal
mass-weighted basis.
  (a) increments   PotGNN.calc_mode_increments_device (M modes and the rest) next to calc_group_increments_device (one
                   group) on the same frames, float64: both run the same taped forwards and reverse passes of six
                   cotangent rows per frame and differ in the contraction alone
  (b) contraction  rn_potgnn_mode_contract_device alone on Jacobian rows of the same shape (random: the arithmetic does
                   not depend on the values), between HIP events on the call's stream.  Its share is this time over the
                   device time of (a)'s mode call; the flops are computed from the shapes (14 * 3N * M a step: seven
                   products), not counted by the hardware, against the float64 matrix peak csrc/kernels_gemm.hip quotes
  (c) reducer      DeviceModeMDRamanSpectrum.measure() and measure_segments(W, hop = W // 2) of (a)'s increments, and
                   the HIP-event times of their phases (rn_md_raman_modes_phase_times)
One warm-up call of each path; a device synchronise precedes every clock read; the median and the range of --reps calls.

Usage: python tools/mode_raman_timing.py [--frames 129] [--width 33] [--reps 5] [--out FILE]
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
from bench import make_workload  # noqa: E402
from ramannoodle_amd import _lib  # noqa: E402
from ramannoodle_amd.spectrum import DeviceModeMDRamanSpectrum, mode_projectors  # noqa: E402

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
    return out, float(np.median(times)), f"{np.median(times):9.2f} ms [{min(times):.2f} .. {max(times):.2f}]"


def phases(fn, reps):
    lib = _lib.load()
    lib.rn_md_raman_modes_set_profiling(1)
    rows = []
    try:
        for _ in range(reps):
            fn()
            millis = (C.c_double * 4)()
            lib.rn_md_raman_modes_phase_times(millis)
            rows.append(list(millis))
    finally:
        lib.rn_md_raman_modes_set_profiling(0)
    return np.median(np.array(rows), axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=129)
    ap.add_argument("--width", type=int, default=33)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="", help="also write the lines to this file (profiles/mode_raman.txt quotes them)")
    args = ap.parse_args()
    torch.cuda.init()
    wl = make_workload(num_cells=(4, 4, 2), frames=args.frames, hparams="perf")
    model = wl["model"](device=0).eval()
    atoms, frames = wl["num_atoms"], args.frames
    modes = 3 * atoms
    rng = np.random.default_rng(0)
    basis = np.linalg.qr(rng.normal(size=(modes, modes)))[0].T.reshape(modes, atoms, 3)
    masses = rng.uniform(1.0, 100.0, atoms)
    fractional = (basis / np.sqrt(masses)[None, :, None]) @ np.linalg.inv(wl["lattice"])
    disp, proj = mode_projectors(fractional, wl["lattice"], masses)
    positions = torch.tensor(wl["positions"], dtype=torch.float64, device="cuda:0")
    one_group = np.zeros(atoms, dtype=np.int32)
    lines = [f"device: {torch.cuda.get_device_name(0)}; ROCm {torch.version.hip}; float64; N = {atoms} atoms (Fn, Fe, passes = "
             f"{wl['hparams']}), S = {frames} frames, M = {modes} modes and the rest; median [min .. max] of {args.reps} "
             "calls after a warm-up"]

    group, _, text = timed(lambda: model.calc_group_increments_device(positions, one_group), args.reps)
    lines.append(f"calc_group_increments_device (one group) {text}")
    increments, mode_ms, text = timed(lambda: model.calc_mode_increments_device(positions, disp, proj), args.reps)
    lines.append(f"calc_mode_increments_device  (M + rest)  {text}")
    total = group[:, 0].cpu().numpy()
    closure = np.abs(increments.sum(dim=1).cpu().numpy() - total).max() / np.abs(total).max()
    lines.append(f"sum over the channels - the one group: {closure:.1e} of the largest entry")
    print("\n".join(lines), flush=True)

    jac = torch.tensor(rng.normal(size=(frames, 6, atoms, 3)), device="cuda:0")
    d_disp, d_proj = torch.tensor(disp, device="cuda:0"), torch.tensor(proj, device="cuda:0")
    out = torch.empty((frames - 1, modes + 1, 9), dtype=torch.float64, device="cuda:0")
    sigma = np.ones(9)
    stream = torch.cuda.current_stream()

    def contract():
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        rc = _lib.load().rn_potgnn_mode_contract_device(
            C.c_void_p(jac.data_ptr()), frames, C.c_void_p(positions.data_ptr()), atoms, C.c_void_p(d_disp.data_ptr()),
            C.c_void_p(d_proj.data_ptr()), modes, C.c_void_p(sigma.ctypes.data), 1, modes + 1,
            C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream))
        end.record()
        assert rc == _lib.RN_OK
        torch.cuda.synchronize()
        return start.elapsed_time(end)

    contract()
    events = [contract() for _ in range(args.reps)]
    contract_ms = float(np.median(events))
    flops = 14.0 * 3 * atoms * modes * (frames - 1)
    rate = flops / (1e-3 * contract_ms)
    share = contract_ms / mode_ms
    lines.append(f"contraction alone (both kernels, sigma's copy included; HIP events) {contract_ms:.3f} ms "
                 f"[{min(events):.3f} .. {max(events):.3f}] = {100.0 * share:.2f} % of the mode call")
    lines.append(f"contraction {flops / 1e9:.2f} GFLOP (computed) = {rate / 1e12:.2f} TFLOP/s = "
                 f"{100.0 * rate / F64_MATRIX_PEAK:.1f} % of the 78 TFLOP/s float64 matrix peak")
    if share > 0.1:
        lines.append("the share exceeds a tenth: see the note at the end of profiles/mode_raman.txt")
    print("\n".join(lines[-2:]), flush=True)

    spectrum = DeviceModeMDRamanSpectrum(increments, 1.0)
    for name, call in (("whole", lambda: spectrum.measure()[1]),
                       ("Welch", lambda: spectrum.measure_segments(args.width, args.width // 2)[1])):
        _, _, text = timed(call, args.reps)
        ms = phases(call, args.reps)
        lines.append(f"{name:5s} reducer, C + 1 = {modes + 2} rows {text}")
        lines.append(f"{name:5s} phases (HIP events, median): builder {ms[0]:.3f} ms, forward FFTs {ms[1]:.3f} ms, power "
                     f"{ms[2]:.3f} ms, back half and copies {ms[3]:.3f} ms")
        print("\n".join(lines[-2:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
