#!/usr/bin/env python3
"""A/B of the entries of the five analysis modules (line-shape fits, multi-peak fits, covariance moments, harmonic
trajectories, band moments) between two builds of the library (profiles/analysis_entries_ab.txt), modelled on
tools/api_split_ab.py.  RN_POTGNN_LIB selects the library.

  --measure           one process, one JSON line.  "hashes": the SHA-256 of the results of every call below, made once, in
                      a fixed order; "seconds": the wall time of one call, a device synchronise before each clock read,
                      the median of --small-calls calls after --small-warmup for the small shapes and of --calls calls
                      after one for the timing shapes.
                      The calls, each through the host entry and the _device entry (inputs already in HBM):
                        the shapes of tests/test_analysis_entries_gpu.py (tests/analysis_entries_cases.py): per module
                        small, larger, small again;
                        lineshape   76 900 fits of 129 bins in rows of 256 (tools/lineshape_timing.py, profiles/lineshape_fit.txt)
                        peakfit     the same table, P = 1, 2, 4 (tools/peakfit_timing.py, profiles/peak_fits.txt; P = 2 timed)
                        qh          256 atoms x 10 000 frames, 1 and 8 blocks (tools/quasiharmonic_timing.py; 1 block timed)
                        ht          256 atoms, 768 modes, 10 000 frames, 1 and 8 runs (tools/harmonic_trajectory_timing.py)
                        bm          256 atoms, 16 weight rows, with alpha: 25 001 frames as one segment, and 8 segments of
                                    4097 frames ("whole" and "runs" of tools/band_modes_timing.py)
  --drive PARENT NEW  every process fresh, parent and new interleaved: --measure six times per library, bench.py --gpus 1
                      --steps 10 --warmup 3 three times per library; then the report.  Stops at the first child that fails.
                      --only measure|bench runs one part.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _digest(arrays):
    sha = hashlib.sha256()
    for array in arrays:
        array = np.ascontiguousarray(array)
        sha.update(f"{array.dtype}{array.shape}".encode())
        sha.update(array.tobytes())
    return sha.hexdigest()[:16]


def timing_calls():
    """name -> call, at the shapes of the timing tools; a call returns a tuple of host arrays."""
    import torch
    from band_modes_timing import LATTICE as BM_LATTICE
    from harmonic_trajectory_timing import inputs as ht_inputs
    from lineshape_timing import make_rows as lineshape_rows
    from peakfit_timing import make_rows as peakfit_rows
    from ramannoodle_amd import harmonic
    from ramannoodle_amd.bandmodes import band_moments_device
    from ramannoodle_amd.lineshape import fit_lorentzians
    from ramannoodle_amd.peakfit import fit_peaks_multi
    from ramannoodle_amd.quasiharmonic import moments_device, run_blocks
    from tests.analysis_entries_cases import fields, on_gpu
    calls = {}

    def both(name, call, host, *rest):
        device = on_gpu(host)
        calls[f"{name} host"] = lambda: call(host, *rest)
        calls[f"{name} device"] = lambda: call(device, *rest)

    w, rows, windows = lineshape_rows(100, 769, 256, 129)
    both("lineshape 76900 fits", lambda r, *a: fields(fit_lorentzians(a[0], r, a[1], device=0)), rows, w, windows)
    for peaks in (1, 2, 4):
        w, rows, windows, centres = peakfit_rows(100, 769, 256, 129, peaks)
        both(f"peakfit 76900 fits P = {peaks}", lambda r, *a: fields(fit_peaks_multi(a[0], r, a[1], a[2], device=0)), rows,
             w, windows, centres)
    rng = np.random.default_rng(0)
    atoms, frames = 256, 10_000
    positions = (rng.random((1, atoms, 3)) + 0.01 * rng.normal(size=(frames, atoms, 3))) % 1.0
    for blocks in (1, 8):
        bounds, joined = run_blocks([frames], blocks)
        both(f"qh 256 x 10000, {blocks} block(s)", lambda p, *a: tuple(moments_device(p, *a, device=0)), positions,
             positions[0], bounds, joined)
    for runs in (1, 8):
        name = f"ht 256 x 768 x 10000, {runs} run(s)"
        inputs = ht_inputs(256, runs)
        out = torch.empty((runs, 10_000, 256, 3), dtype=torch.float64, device="cuda:0")
        calls[f"{name} host"] = lambda inputs=inputs: (harmonic.synthesize_download(*inputs, 10_000, device=0),)
        calls[f"{name} device"] = lambda inputs=inputs, out=out: (
            harmonic.synthesize_device(*inputs, 10_000, out=out).cpu().numpy(),)

        def left_in_hbm(inputs=inputs, out=out):  # (the device entry alone: it does not wait for its kernel, the clock does)
            harmonic.synthesize_device(*inputs, 10_000, out=out)
            return ()

        calls[f"{name} device, left in HBM"] = left_in_hbm
    # the two shapes of tools/band_modes_timing.py, drawn as it draws them: "whole", then "runs" from the same generator
    rng = np.random.default_rng(0)
    masses = rng.uniform(1.0, 100.0, atoms)
    for name, width, starts in (("bm 256 x 25001, 1 segment", 25_001, np.array([0], dtype=np.int64)),
                                ("bm 256 x 32776, 8 segments of 4097", 4097, np.arange(8, dtype=np.int64) * 4097)):
        frames = width * len(starts)
        positions = (rng.random((1, atoms, 3)) + 0.01 * rng.normal(size=(frames, atoms, 3))) % 1.0
        alpha = np.cumsum(0.01 * rng.normal(size=(frames, 3, 3)), axis=0)
        steps = width - 1
        bins = (steps + 1) // 2 - 1
        plain = np.zeros((8, bins))
        for b in range(8):
            plain[b, (b + 1) * bins // 10:(b + 1) * bins // 10 + 25] = 1.0
        weights = np.concatenate([plain, plain * (np.arange(1, bins + 1) * (33356.40951981521 / steps))[None, :]])
        rest = (width, starts, np.ones(steps), weights)
        for entry, p, a in (("host", positions, alpha), ("device", on_gpu(positions), on_gpu(alpha))):
            calls[f"{name} {entry}"] = lambda p=p, a=a, rest=rest: (band_moments_device(p, BM_LATTICE, masses, a, *rest),)
    return calls


TIMED = ("lineshape 76900 fits", "peakfit 76900 fits P = 2", "qh 256 x 10000, 1 block", "ht 256", "bm 256")  # prefixes


def measure(small_calls, small_warmup, calls):
    import torch
    from tests.analysis_entries_cases import CALLS
    hashes, seconds = {}, {}

    def clock(call, count, warmup):
        samples = []
        for index in range(warmup + count):
            torch.cuda.synchronize()
            start = time.perf_counter()
            call()
            torch.cuda.synchronize()
            if index >= warmup:
                samples.append(time.perf_counter() - start)
        return statistics.median(samples)

    for module, sizes in CALLS.items():
        for step, size in enumerate(("small", "larger", "small")):
            for entry, call in sizes[size].items():
                hashes[f"{module} {size} {entry}" + (" again" if step == 2 else "")] = _digest(call())
        for entry, call in sizes["small"].items():
            seconds[f"{module} small {entry}"] = clock(call, small_calls, small_warmup)
    for name, call in timing_calls().items():
        results = call()
        if results:
            hashes[name] = _digest(results)
        if name.startswith(TIMED):
            seconds[name] = clock(call, calls, 1)
    print(json.dumps({"hashes": hashes, "seconds": seconds}), flush=True)


# ----------------------------------------------------------------------------- the driver
def _child(lib, args, limit):
    """A fresh process on library ``lib``; its last output line.  A failure ends the whole run."""
    env = dict(os.environ, RN_POTGNN_LIB=os.path.abspath(lib))
    done = subprocess.run([sys.executable] + args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=limit,
                          check=False)
    if done.returncode != 0:
        sys.exit(f"{' '.join(args)} on {lib}: exit {done.returncode}\n{done.stdout[-2000:]}\n{done.stderr[-2000:]}")
    print(".", end="", file=sys.stderr, flush=True)
    lines = done.stdout.strip().splitlines()
    return lines[-1] if lines else ""


def report_outputs(parent, new):
    ok = True
    names = list(parent[0])
    print(f"1. Outputs: {len(names)} calls, SHA-256 of the results, {len(parent)} parent runs and {len(new)} new runs")
    same = [n for n in names if len({run[n] for run in parent + new}) == 1]
    print(f"  byte for byte in every parent run and every new run ({len(same)} of {len(names)}):")
    for start in range(0, len(same), 4):
        print("    " + "; ".join(same[start:start + 4]))
    for name in names:
        if name in same:
            continue
        of_parent, of_new = {run[name] for run in parent}, {run[name] for run in new}
        fine = len(of_parent) > 1 and of_new <= of_parent
        ok = ok and fine
        print(f"  {name}: parent {sorted(of_parent)} new {sorted(of_new)}: "
              + ("the parent's own runs differ; the new ones are among them" if fine else "NOT byte for byte  FAILS"))
    return ok


def report_time(label, parent, new, unit=1e6, higher_is_better=False):
    """Lower is better: the new median no higher than the parent's median plus the parent's own range (throughput: no
    lower than the median minus the range)."""
    spread = max(parent) - min(parent)
    if higher_is_better:
        bound = statistics.median(parent) - spread
        fine = statistics.median(new) >= bound
    else:
        bound = statistics.median(parent) + spread
        fine = statistics.median(new) <= bound
    row = lambda values: " ".join(f"{unit * v:.5g}" for v in values)  # noqa: E731
    print(f"  {label:<44} parent {row(parent)} | new {row(new)} | medians {unit * statistics.median(parent):.5g} / "
          f"{unit * statistics.median(new):.5g}, bound {unit * bound:.5g}: {'met' if fine else 'NOT MET'}")
    return fine


def drive(parent_lib, new_lib, only, options):
    me = os.path.abspath(__file__)
    libs = (("parent", parent_lib), ("new", new_lib))
    ok = True
    if only in (None, "measure"):
        runs = {"parent": [], "new": []}
        for _ in range(6):
            for tag, lib in libs:
                runs[tag].append(json.loads(_child(lib, [me, "--measure"] + options, 600)))
        ok = report_outputs([r["hashes"] for r in runs["parent"]], [r["hashes"] for r in runs["new"]]) and ok
        print("3. Speed: wall time of one call in microseconds, synchronised; six processes per library, interleaved, the "
              "median of each")
        for name in runs["parent"][0]["seconds"]:
            ok = report_time(name, [r["seconds"][name] for r in runs["parent"]], [r["seconds"][name] for r in runs["new"]]) and ok
        sys.stdout.flush()
    if only in (None, "bench"):
        rates = {"parent": [], "new": []}
        for _ in range(3):
            for tag, lib in libs:
                line = _child(lib, [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3"], 600)
                rates[tag].append(json.loads(line)["value"])
        print("3. Speed: bench.py --gpus 1 --steps 10 --warmup 3, structures/s (three processes per library, interleaved)")
        ok = report_time("value", rates["parent"], rates["new"], unit=1.0, higher_is_better=True) and ok
    print("ALL CRITERIA MET" if ok else "A CRITERION IS NOT MET")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--small-calls", type=int, default=200)
    ap.add_argument("--small-warmup", type=int, default=20)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--drive", nargs=2, metavar=("PARENT", "NEW"))
    ap.add_argument("--only", choices=("measure", "bench"))
    args = ap.parse_args()
    options = ["--small-calls", str(args.small_calls), "--small-warmup", str(args.small_warmup), "--calls", str(args.calls)]
    if args.measure:
        measure(args.small_calls, args.small_warmup, args.calls)
    elif args.drive:
        sys.exit(drive(args.drive[0], args.drive[1], args.only, options))
    else:
        ap.error("one of --measure, --drive")


if __name__ == "__main__":
    main()
