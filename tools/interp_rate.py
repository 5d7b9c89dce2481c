#!/usr/bin/env python3
"""The interpolation model on the GPU (profiles/interpolation_model.txt): 256 atoms, 768 DOFs of a seeded orthonormal
basis, cubic splines through 7 points, S frames (10 000 and 2 000).
  (a) frames/s   InterpolationModel.calc_polarizabilities_device on frames in HBM, and calc_polarizabilities from a
                 host array (staging copies included); a host clock around calls that end in a device synchronise
  (b) kernels    the forward launch (interp_alpha_kernel) and the Jacobian's two launches (interp_alpha_kernel with the
                 derivative epilogue, interp_rows_kernel) between HIP events on the call's stream; the events bracket
                 nothing but the launches of one entry
                 the forward launch again for a model of the same shape whose splines are order 1 with one piece: the
                 same product with next to no epilogue, so the difference is what the cubic epilogue costs
  (c) bound      the time the float64 products alone would take at the matrix-pipe rate (2 S 3N J flop for the
                 amplitudes, 2 (6 S) J 3N more for the Jacobian rows), computed from the shapes, and the bytes each
                 kernel must move at the HBM rate
  (d) host       evaluate_host (numpy) on the same frames, for comparison
One warm-up call of each path; a device synchronise precedes every clock read; the median and the range of --reps calls.

Usage: python tools/interp_rate.py [--frames 10000 2000] [--reps 7] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch  # before the HIP library: one HIP runtime per process (torch's)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scipy.interpolate import make_interp_spline  # noqa: E402

from ramannoodle_amd.pmodel import InterpolationModel  # noqa: E402
from ramannoodle_amd.structure import ReferenceStructure  # noqa: E402

F64_MATRIX_PEAK = 78.0e12  # flop/s, the figure csrc/kernels_gemm.hip quotes (the public 78.6 TFLOP/s of the part)
HBM_PEAK = 8.0e12  # byte/s (MI355X_MICROARCH: 8 TB/s)


def make_model(atoms: int, dofs: int, seed: int = 0, linear: bool = False):
    """The workload's model; ``linear``: the same basis with order-1 splines through two points (one piece, no search,
    one Horner step), so that its forward launch is the product with next to no epilogue."""
    rng = np.random.default_rng(seed)
    lattice = np.diag([17.0, 17.5, 18.0]) + rng.uniform(-0.5, 0.5, size=(3, 3))
    ref = rng.uniform(0.02, 0.98, size=(atoms, 3))
    basis = np.linalg.qr(rng.normal(size=(3 * atoms, 3 * atoms)))[0].T[:dofs].reshape(dofs, atoms, 3)
    x = np.array([-0.3, 0.3]) if linear else np.array([-0.3, -0.2, -0.1, 0.0, 0.1, 0.2, 0.3])
    splines = []
    for _ in range(dofs):
        y = rng.normal(size=(len(x), 3, 3)) * x[:, None, None]
        splines.append(make_interp_spline(x, (y + y.transpose(0, 2, 1)) / 2, k=1 if linear else 3))
    alpha_ref = np.diag([40.0, 41.0, 39.0])
    structure = ReferenceStructure([8] * atoms, lattice, ref)
    return InterpolationModel(structure, alpha_ref, list(basis), splines), ref


def timed(fn, reps):
    fn()  # warm-up
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(times)), f"{np.median(times):9.3f} ms [{min(times):.3f} .. {max(times):.3f}]"


def events(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end))
    return float(np.median(times)), f"{np.median(times):9.3f} ms [{min(times):.3f} .. {max(times):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[10000, 2000])
    ap.add_argument("--atoms", type=int, default=256)
    ap.add_argument("--dofs", type=int, default=768)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="", help="also write the lines to this file (profiles/interpolation_model.txt quotes them)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/interp_rate.py measures on a GPU: none found")
    torch.cuda.init()
    model, ref = make_model(args.atoms, args.dofs)
    linear, _ = make_model(args.atoms, args.dofs, linear=True)
    atoms, dofs, k3 = args.atoms, args.dofs, 3 * args.atoms
    lines = [f"device: {torch.cuda.get_device_name(0)}; ROCm {torch.version.hip}; float64; N = {atoms} atoms, J = {dofs} DOFs, "
             f"cubic splines through 7 points (4 pieces); median [min .. max] of {args.reps} calls after a warm-up"]
    for frames in args.frames:
        rng = np.random.default_rng(frames)
        host = ref + rng.normal(size=(frames, atoms, 3)) * 0.004
        host -= np.floor(host)
        positions = torch.tensor(host, dtype=torch.float64, device="cuda:0")
        out = torch.empty((frames, 3, 3), dtype=torch.float64, device="cuda:0")
        jac = torch.empty((frames, 6, atoms, 3), dtype=torch.float64, device="cuda:0")
        lines.append(f"--- S = {frames} frames")
        ms, text = timed(lambda: model.calc_polarizabilities_device(positions, out=out), args.reps)
        lines.append(f"calc_polarizabilities_device (frames in HBM) {text} = {frames / (1e-3 * ms):12.0f} frames/s")
        ms, text = timed(lambda: model.calc_polarizabilities(host), args.reps)
        lines.append(f"calc_polarizabilities (host array in, out)   {text} = {frames / (1e-3 * ms):12.0f} frames/s")
        fwd_ms, text = events(lambda: model.calc_polarizabilities_device(positions, out=out), args.reps)
        lines.append(f"forward launch (HIP events)                  {text}")
        lin_ms, text = events(lambda: linear.calc_polarizabilities_device(positions), args.reps)
        lines.append(f"forward launch, order 1 and one piece        {text}   (the same product, next to no epilogue)")
        jac_ms, text = events(lambda: model.calc_jacobian_device(positions, out=jac), args.reps)
        lines.append(f"Jacobian, two launches (HIP events)          {text}")
        flops = 2.0 * frames * k3 * dofs
        product_ms = 1e3 * flops / F64_MATRIX_PEAK
        lines.append(f"amplitude product {flops / 1e9:.2f} GFLOP (computed) = {product_ms:.3f} ms at the 78 TFLOP/s float64 matrix "
                     f"rate; the forward launch is {fwd_ms / product_ms:.1f} x that = "
                     f"{flops / (1e-3 * fwd_ms) / 1e12:.2f} TFLOP/s of product")
        read_ms = 1e3 * (frames * k3 * 8.0) / HBM_PEAK
        lines.append(f"forward reads {frames * k3 * 8 / 1e6:.1f} MB of frames once = {read_ms:.3f} ms at 8 TB/s")
        jflops = flops + 2.0 * 6 * frames * dofs * k3
        jbytes = frames * 6 * k3 * 8.0 + 2 * frames * 6 * dofs * 8.0 + frames * k3 * 8.0
        lines.append(f"Jacobian products {jflops / 1e9:.2f} GFLOP (computed) = {1e3 * jflops / F64_MATRIX_PEAK:.3f} ms at that rate; "
                     f"rows written, derivatives written and read, frames read: {jbytes / 1e6:.1f} MB = "
                     f"{1e3 * jbytes / HBM_PEAK:.3f} ms at 8 TB/s; measured {jac_ms:.3f} ms")
        print("\n".join(lines[-9:]), flush=True)
        if frames == min(args.frames):
            threads = torch.get_num_threads()
            t0 = time.perf_counter()
            want = model.evaluate_host(host)
            host_ms = 1e3 * (time.perf_counter() - t0)
            error = np.abs(out.cpu().numpy() - want).max() / np.abs(want).max()
            lines.append(f"evaluate_host (numpy, OMP_NUM_THREADS = {os.environ.get('OMP_NUM_THREADS', 'unset')}, torch threads "
                         f"{threads}), one call: {host_ms:.1f} ms = {frames / (1e-3 * host_ms):.0f} frames/s; device - host "
                         f"{error:.1e} of the largest entry")
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
