#!/usr/bin/env python3
"""Times of the model-domain check on the GPU (profiles/model_domain.txt), on the benchmark's config 3 (256 atoms,
10 000 frames, the "perf" widths):
  (a) calc_polarizabilities_device and calc_descriptors_device(..., alpha_out=...) of the same frames in HBM: what the
      pooling kernel adds to an evaluation.  --polarizabilities-only times the first alone, so that the same line can be
      taken with another build of the library (RN_POTGNN_LIB, e.g. the parent commit's);
  (b) nearest() of all descriptors against those of the first --training frames, and select_farthest() of --picks frames
      seeded with them, descriptors in HBM: wall time and, with rn_select_set_profiling(1), the HIP-event times of the
      four phases (copies in, search, picks, copies out);
  (c) DomainCheck end to end on tensors in HBM.
One warm-up call of each; a device synchronise precedes every clock read; the median and the range of --reps calls.

Usage: python tools/model_domain_timing.py [--frames 10000] [--training 1000] [--picks 100] [--reps 7]
                                           [--polarizabilities-only] [--out FILE]
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
from bench import CONFIGS, make_workload  # noqa: E402
from ramannoodle_amd import _lib  # noqa: E402


def timed(fn, reps):
    out = fn()  # warm-up
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return out, f"{np.median(times):9.3f} ms [{min(times):.3f} .. {max(times):.3f}]"


def phases(fn, reps):
    lib = _lib.load()
    lib.rn_select_set_profiling(1)
    rows = []
    try:
        for _ in range(reps):
            fn()
            millis = (C.c_double * 4)()
            lib.rn_select_phase_times(millis)
            rows.append(list(millis))
    finally:
        lib.rn_select_set_profiling(0)
    ms = np.median(np.array(rows), axis=0)
    return f"copies in {ms[0]:.3f} ms, search {ms[1]:.3f} ms, picks {ms[2]:.3f} ms, copies out {ms[3]:.3f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=CONFIGS[3]["frames"])
    ap.add_argument("--training", type=int, default=1000)
    ap.add_argument("--picks", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--polarizabilities-only", action="store_true")
    ap.add_argument("--out", default="", help="append the lines to this file")
    args = ap.parse_args()
    if args.polarizabilities_only:  # a library of an earlier commit lacks the newer entries: leave them out of this run's tables
        library = C.CDLL(_lib.library_path())
        for table in (_lib.SIGNATURES, _lib.SELECT_SIGNATURES):
            for name in [name for name in table if not hasattr(library, name)]:
                del table[name]
    torch.cuda.init()
    config = CONFIGS[3]
    wl = make_workload(num_cells=config["cells"], frames=args.frames, hparams="perf", seed=config["seed"])
    model = wl["model"](device=0)
    positions = torch.tensor(wl["positions"], dtype=torch.float64, device="cuda:0")
    frames = positions.shape[0]
    lines = [f"device: {torch.cuda.get_device_name(0)}; ROCm {torch.version.hip}; library {os.path.basename(_lib.library_path())}; "
             f"config 3: {wl['num_atoms']} atoms, {frames} frames, (Fn, Fe, passes) = {wl['hparams']}; median [min .. max] of "
             f"{args.reps} calls after a warm-up"]
    alpha = torch.empty((frames, 3, 3), dtype=torch.float64, device="cuda:0")
    _, text = timed(lambda: model.calc_polarizabilities_device(positions, out=alpha), args.reps)
    lines.append(f"calc_polarizabilities_device                      {text}")
    if not args.polarizabilities_only:
        from ramannoodle_amd.selection import DomainCheck, nearest, select_farthest
        alpha_too = torch.empty_like(alpha)
        desc, text = timed(lambda: model.calc_descriptors_device(positions, alpha_out=alpha_too), args.reps)
        lines.append(f"calc_descriptors_device(..., alpha_out=...)       {text}   alpha bit-identical: "
                     f"{bool(torch.equal(alpha, alpha_too))}")
        _, text = timed(lambda: model.calc_descriptors_device(positions), args.reps)
        lines.append(f"calc_descriptors_device, descriptors alone        {text}")
        training = desc[:args.training].contiguous()
        center = training.mean(dim=0).cpu().numpy()
        scale = 1.0 / training.std(dim=0, unbiased=False).cpu().numpy()
        shape = f"S = {frames}, M = {args.training}, D = {desc.shape[1]}"
        _, text = timed(lambda: nearest(desc, training, center, scale), args.reps)
        lines.append(f"nearest, {shape:34s}       {text}")
        lines.append(f"  phases (HIP events, median): {phases(lambda: nearest(desc, training, center, scale), args.reps)}")
        _, text = timed(lambda: select_farthest(desc, args.picks, training, center=center, scale=scale), args.reps)
        lines.append(f"select_farthest, {args.picks} picks, seeded, {shape:20s} {text}")
        lines.append("  phases (HIP events, median): "
                     + phases(lambda: select_farthest(desc, args.picks, training, center=center, scale=scale), args.reps))
        _, text = timed(lambda: select_farthest(desc, args.picks, scale=scale), args.reps)
        lines.append(f"select_farthest, {args.picks} picks, no reference            {text}")
        check, text = timed(lambda: DomainCheck(model, positions[:args.training]), args.reps)
        lines.append(f"DomainCheck of the first {args.training} frames (descriptors, leave-one-out search) {text}   unit "
                     f"{check.unit:.4f}")
        novelty, text = timed(lambda: check.novelty(positions), args.reps)
        lines.append(f"DomainCheck.novelty of {frames} frames (descriptors + search)   {text}   median novelty "
                     f"{np.median(novelty):.3f}, outside {100.0 * np.mean(novelty > 1.0):.1f} %")
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
