#!/usr/bin/env python3
"""Polarized MD Raman spectra: host (numpy/scipy, 21 basis spectra) against the GPU reduction
(rn_md_raman_polarized from a host series, rn_md_raman_polarized_device from a series in HBM), for
S in {1e4, 1e5, 1e6} steps and K in {2, 720} configurations.  One warm-up call of each path per size
(plans, buffers), a device synchronise before every clock read, the median of the timed calls, and the
largest difference from the host result at every timed size.  Also the per-configuration host cost of the
direct route (one correlation and one FFT per configuration, timed on two configurations).

Usage: python tools/polarized_spectrum_bench.py [--steps 10000,100000,1000000] [--configs 2,720] [--reps 3]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch  # before the HIP library: one HIP runtime per process (torch's)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scipy.spatial.transform import Rotation  # noqa: E402

from ramannoodle_amd.spectrum import DeviceMDRamanSpectrum, MDRamanSpectrum, calc_signal_spectrum  # noqa: E402


def timed(fn, reps):
    out, times = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="10000,100000,1000000")
    ap.add_argument("--configs", default="2,720")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    torch.cuda.init()
    rng = np.random.default_rng(0)
    print(f"device: {torch.cuda.get_device_name(0)}; float64; times are medians of {args.reps} calls after a warm-up")
    for steps in (int(s) for s in args.steps.split(",")):
        a = rng.normal(size=(steps, 3, 3))
        a = a + np.swapaxes(a, 1, 2)
        host = MDRamanSpectrum(a, 1.0)
        resident = DeviceMDRamanSpectrum(torch.tensor(a, device="cuda"), 1.0)
        # the direct route: one correlation and one FFT per configuration
        e_i, e_s = rng.normal(size=(2, 3)), rng.normal(size=(2, 3))
        e_i /= np.linalg.norm(e_i, axis=1, keepdims=True)
        e_s /= np.linalg.norm(e_s, axis=1, keepdims=True)
        da = np.diff(a, axis=0)
        t0 = time.perf_counter()
        for k in range(2):
            calc_signal_spectrum(np.einsum("a,tab,b->t", e_s[k], da, e_i[k]), 1.0)
        per_config = (time.perf_counter() - t0) / 2
        for k in (int(c) for c in args.configs.split(",")):
            e_i, e_s = rng.normal(size=(k, 3)), rng.normal(size=(k, 3))
            rot = Rotation.random(k, random_state=k).as_matrix()
            reps = 1 if steps * k > 10**8 else args.reps
            host.measure_polarized(e_i, e_s, rot)
            (_, i_host), t_host = timed(lambda: host.measure_polarized(e_i, e_s, rot), reps)
            host.measure_polarized(e_i, e_s, rot, device=0)
            (_, i_dev), t_dev = timed(lambda: host.measure_polarized(e_i, e_s, rot, device=0), reps)
            err_dev = np.abs(i_dev - i_host).max() / np.abs(i_host).max()
            del i_dev
            resident.measure_polarized(e_i, e_s, rot)
            (_, i_res), t_res = timed(lambda: resident.measure_polarized(e_i, e_s, rot), reps)
            err_res = np.abs(i_res - i_host).max() / np.abs(i_host).max()
            del i_res, i_host
            print(f"S = {steps:8d}  K = {k:4d}: host {t_host * 1e3:9.1f} ms   device from host alpha "
                  f"{t_dev * 1e3:8.2f} ms   device-resident alpha {t_res * 1e3:8.2f} ms   "
                  f"speed-up {t_host / t_res:6.1f}x   direct host route ~{per_config * k * 1e3:9.1f} ms "
                  f"({per_config * 1e3:.2f} ms/config)   max rel diff {err_dev:.1e} / {err_res:.1e}", flush=True)


if __name__ == "__main__":
    main()
