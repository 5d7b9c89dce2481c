#!/usr/bin/env python3
"""Variable-cell costs (profiles/variable_cell.txt):
  evaluation  PotGNN.calc_polarizabilities_device on bench.py's config 3 frames (rocksalt, 256 atoms, Fn = Fe = 64,
              P = 4, 10 000 frames), fixed cell and with a lattice per frame, L_t = L0 (I + eps_t) with the strain of
              tests/test_variable_cell_gpu.py (t = frame index in fs); structures/s, the calls alternated
  increments  PotGNN.calc_group_increments_device on the same structure, groups = "species", float32 and float64,
              without and with lattices (the reverse pass then writes dlat too, and the cell channel is one more launch
              per chunk); ms per step
One warm-up call per case; a device synchronise precedes every clock read; the best of --reps calls.
--fixed-only measures the fixed-cell lines alone and touches nothing the parent commit lacks (for A/B against it).

Usage: python tools/variable_cell_bench.py [--frames 10000] [--steps 256] [--reps 5] [--fixed-only] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch  # before the HIP library: one HIP runtime per process (torch's)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import CONFIGS, make_workload  # noqa: E402

AMP = np.array([[.010, .004, -.003], [.004, -.008, .005], [-.003, .005, .006]])
PER = np.array([[310., 470., 390.], [470., 260., 530.], [390., 530., 350.]])


def strained(lattice, frames, dt=1.0):
    t = (np.arange(frames) * dt)[:, None, None]
    return lattice[None] @ (np.eye(3)[None] + AMP[None] * np.sin(2 * np.pi * t / PER[None] + 0.3))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=CONFIGS[3]["frames"])
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fixed-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variable_cell.txt"))
    args = ap.parse_args()
    torch.cuda.init()
    lines = [f"# device: {torch.cuda.get_device_name(0)}; best of {args.reps} calls after one warm-up"
             + ("; fixed cell only" if args.fixed_only else "")]

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    cfg = CONFIGS[3]
    wl = make_workload(num_cells=cfg["cells"], frames=args.frames, seed=cfg["seed"])
    model = wl["model"](device=0).eval()
    positions = torch.tensor(wl["positions"], dtype=torch.float64, device="cuda:0")
    out = torch.empty((args.frames, 3, 3), dtype=torch.float64, device="cuda:0")
    cases = {"fixed cell": {}}
    if not args.fixed_only:
        cases["lattice per frame"] = {"lattices": torch.tensor(strained(wl["lattice"], args.frames), dtype=torch.float64,
                                                               device="cuda:0")}
    best = {name: float("inf") for name in cases}
    for name, kw in cases.items():
        model.calc_polarizabilities_device(positions, out, synchronize=True, **kw)
    for _ in range(args.reps):
        for name, kw in cases.items():  # alternated: a drifting clock hits both
            best[name] = min(best[name], timed(lambda: model.calc_polarizabilities_device(positions, out, synchronize=True, **kw)))
    for name in cases:
        emit(f"evaluation  {wl['num_atoms']} atoms  {args.frames} frames  {name:18s}: {best[name] * 1e3:8.2f} ms  "
             f"{args.frames / best[name]:9.0f} structures/s")
    if not args.fixed_only:
        emit(f"evaluation  lattice per frame / fixed cell: {best['fixed cell'] / best['lattice per frame']:.4f} of the rate")

    steps = args.steps
    frames = positions[:steps + 1].contiguous()
    cases = {"atoms only": {}}
    if not args.fixed_only:
        cases["atoms + cell"] = {"lattices": torch.tensor(strained(wl["lattice"], steps + 1), dtype=torch.float64, device="cuda:0")}
    for float64 in (False, True):
        best = {name: float("inf") for name in cases}
        for name, kw in cases.items():
            model.calc_group_increments_device(frames, "species", float64=float64, **kw)
        for _ in range(max(2, args.reps // 2)):
            for name, kw in cases.items():
                best[name] = min(best[name], timed(lambda: model.calc_group_increments_device(frames, "species", float64=float64, **kw)))
        for name in cases:
            emit(f"increments  {wl['num_atoms']} atoms  {steps} steps  {'float64' if float64 else 'float32'}  {name:13s}: "
                 f"{best[name] * 1e3:8.1f} ms  {best[name] / steps * 1e3:.4f} ms/step")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
