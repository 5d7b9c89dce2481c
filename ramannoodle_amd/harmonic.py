"""Harmonic trajectories (an addition): the atoms of a ``Phonons`` object moved along its modes with thermal amplitudes
and random phases, as a ``Trajectory`` (``Phonons.get_harmonic_trajectory``, ``Phonons.get_harmonic_ensemble``) that
every MD-side analysis takes unchanged, or as a tensor in HBM (``synthesize_device``) that the device consumers read in
place.

Definition.  All float64.  ``ref[j]``: fractional reference positions, ``K = 3N`` columns, ``j = 3 i + r``; ``D[m][j]``:
the fractional displacement of a unit mass-weighted amplitude of mode ``m``, ``D_m[i] = (u_m[i] / sqrt(m_i)) @ inv(L)``
with ``u = spectrum.mode_vectors(displacements, lattice, masses)`` (the convention of
``quasiharmonic.modes_from_moments``); ``omega_dt[m] = omega_m timestep`` with ``omega_m = 2 pi wavenumber_m /
_PER_FS_TO_CM1`` in rad/fs; per run ``r``: ``amp[r][m]`` (amu^1/2 Angstrom) and ``phase[r][m]`` (rad); ``t0 >= 0``: the
absolute index of the first frame.

* ``theta[r][t][m] = omega_dt[m] * (t0 + t) + phase[r][m]``: one rounded product, then one rounded sum (not fused);
* ``y[r][t][j] = ref[j] + sum_m amp[r][m] * cos(theta[r][t][m]) * D[m][j]``;
* ``out[r][t][j] = y - floor(y)`` (``structure.apply_pbc``).

``synthesize_host`` states this in numpy; ``synthesize_device`` computes it on the GPU (``include/rn_harmonic.h``),
differing by the order of the sum over ``m``, the last bits of the cosine and the rounding of the products only.

Amplitudes and phases (``draw``) are made on the host, ``R M`` numbers each.  With ``c = quasiharmonic.AMU_A2_PER_FS2_IN_EV``,
``k_B = constants.BOLTZMANN_CONSTANT`` and ``hbar = constants.REDUCED_PLANCK_CONSTANT``: the mean mode energy is ``E_m =
k_B T`` for ``statistics="classical"`` and ``E_m = (hbar omega_m / 2) / tanh(hbar omega_m / (2 k_B T))`` for
``"quantum"`` (``mode_energies``); ``sampling="mean"`` gives every run the energy ``e = E_m``, ``sampling="random"``
draws ``e = E_m (-log1p(-u))`` with ``u`` uniform in [0, 1): the exponential energy distribution of a thermal
oscillator, for both statistics; ``amp = sqrt(2 e / c) / omega_m``, so that the mean of ``amp^2 cos^2`` is the thermal
variance ``E_m / (c omega_m^2)``; the phases are uniform in [0, 2 pi).  Order of the draws, all from one
``numpy.random.default_rng(seed)``: for each run in ascending order, the ``M`` phases (``rng.random(M)``), then, for
``"random"`` only, the ``M`` energies (``rng.random(M)``).  Run ``r`` of a draw of ``R`` runs is therefore run ``r`` of
any longer draw with the same seed.

What the result is: harmonic dynamics with the full nonlinear polarizability.  Frequencies do not shift and lines do not
broaden; evaluated with a model, the finite displacements give overtone and combination bands, intensities that depend
on temperature and, with quantum amplitudes, zero-point motion.  Not checked: amplitudes beyond half a cell (the wrapped
positions then no longer tell which image an atom is in).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
from numpy.typing import NDArray

from ramannoodle_amd.constants import BOLTZMANN_CONSTANT, REDUCED_PLANCK_CONSTANT
from ramannoodle_amd.quasiharmonic import AMU_A2_PER_FS2_IN_EV

STATISTICS = ("classical", "quantum")
SAMPLINGS = ("mean", "random")
MAX_FRAME_INDEX = 2 ** 53  # t0 + T may not exceed it: the frame index must be exact in a double
_HOST_FRAMES = 4096  # frames per product of synthesize_host: bounds its temporaries


def angular_frequencies(wavenumbers) -> NDArray[np.float64]:
    """Wavenumbers in 1/cm as angular frequencies in rad/fs."""
    from ramannoodle_amd.spectrum import _PER_FS_TO_CM1
    return 2.0 * np.pi * np.asarray(wavenumbers, dtype=np.float64) / _PER_FS_TO_CM1


def _temperature(temperature) -> float:
    try:
        temperature = float(temperature)
    except (TypeError, ValueError) as exc:
        raise ValueError(f"invalid temperature: {temperature!r}") from exc
    if not (temperature > 0 and np.isfinite(temperature)):
        raise ValueError(f"invalid temperature: {temperature} <= 0")
    return temperature


def _positive_wavenumbers(wavenumbers) -> NDArray[np.float64]:
    wavenumbers = np.asarray(wavenumbers, dtype=np.float64)
    if wavenumbers.ndim != 1 or wavenumbers.size < 1:
        raise ValueError("wavenumbers must hold M >= 1 values")
    if not (np.all(np.isfinite(wavenumbers)) and np.all(wavenumbers > 0)):
        raise ValueError("wavenumbers must be finite and positive: a mode of zero or imaginary frequency cannot be populated")
    return wavenumbers


def mode_energies(wavenumbers, temperature, statistics: str = "classical") -> NDArray[np.float64]:
    """The mean energies ``E_m`` (eV) of the modes at ``temperature`` (K): ``k_B T`` (``"classical"``) or ``(hbar omega /
    2) / tanh(hbar omega / (2 k_B T))`` (``"quantum"``: zero-point motion included)."""
    if statistics not in STATISTICS:
        raise ValueError(f"unknown statistics {statistics!r}: one of {STATISTICS}")
    temperature = _temperature(temperature)
    wavenumbers = _positive_wavenumbers(wavenumbers)
    thermal = BOLTZMANN_CONSTANT * temperature
    if statistics == "classical":
        return np.full(wavenumbers.shape, thermal)
    half_quantum = 0.5 * REDUCED_PLANCK_CONSTANT * angular_frequencies(wavenumbers)
    return half_quantum / np.tanh(half_quantum / thermal)


def draw(wavenumbers, temperature, statistics: str = "classical", sampling: str = "mean", runs: int = 1, seed=0):
    """``(amp[R][M], phase[R][M])`` of ``runs`` independent runs (the module says how and in which order they are drawn)."""
    if sampling not in SAMPLINGS:
        raise ValueError(f"unknown sampling {sampling!r}: one of {SAMPLINGS}")
    energies = mode_energies(wavenumbers, temperature, statistics)
    if isinstance(runs, (bool, np.bool_)) or not isinstance(runs, (int, np.integer)) or runs < 1:
        raise ValueError(f"runs = {runs!r} must be a positive integer")
    omega = angular_frequencies(wavenumbers)
    rng = np.random.default_rng(seed)
    amp = np.empty((int(runs), omega.size))
    phase = np.empty((int(runs), omega.size))
    for r in range(int(runs)):
        phase[r] = 2.0 * np.pi * rng.random(omega.size)
        energy = energies * -np.log1p(-rng.random(omega.size)) if sampling == "random" else energies
        amp[r] = np.sqrt(2.0 * energy / AMU_A2_PER_FS2_IN_EV) / omega
    return amp, phase


def _arguments(ref, D, omega_dt, amp, phase, frames, first_frame):
    """The arrays of the definition as contiguous float64 ``(ref[K], D[M][K], omega_dt[M], amp[R][M], phase[R][M])``."""
    ref = np.ascontiguousarray(ref, dtype=np.float64).reshape(-1)
    if ref.size < 3 or ref.size % 3:
        raise ValueError("ref must be (N,3) or (3N,) with N >= 1")
    D = np.ascontiguousarray(D, dtype=np.float64)
    if D.ndim == 3:
        D = D.reshape(len(D), -1)
    if D.ndim != 2 or D.shape[0] < 1 or D.shape[1] != ref.size:
        raise ValueError(f"D must be (M,N,3) or (M,3N) with M >= 1 and 3N = {ref.size}")
    modes = D.shape[0]
    omega_dt = np.ascontiguousarray(omega_dt, dtype=np.float64)
    if omega_dt.shape != (modes,):
        raise ValueError(f"omega_dt must hold the {modes} values of the modes of D")
    amp = np.ascontiguousarray(amp, dtype=np.float64)
    phase = np.ascontiguousarray(phase, dtype=np.float64)
    if amp.ndim == 1:
        amp = amp[None]
    if phase.ndim == 1:
        phase = phase[None]
    if amp.ndim != 2 or amp.shape[0] < 1 or amp.shape[1] != modes or phase.shape != amp.shape:
        raise ValueError(f"amp and phase must both be (R,M) with R >= 1 and M = {modes}")
    for name, value in (("frames", frames), ("first_frame", first_frame)):
        if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
            raise ValueError(f"{name} = {value!r} must be an integer")
    if frames < 1:
        raise ValueError(f"frames = {frames} must be positive")
    if first_frame < 0 or first_frame + frames > MAX_FRAME_INDEX:
        raise ValueError(f"first_frame = {first_frame} with {frames} frames: the frame indices must lie in [0, 2^53]")
    return ref, D, omega_dt, np.ascontiguousarray(amp), np.ascontiguousarray(phase)


def synthesize_host(ref, D, omega_dt, amp, phase, frames: int, first_frame: int = 0) -> NDArray[np.float64]:
    """The wrapped positions ``(R,T,N,3)`` of the module's definition, in numpy: the statement the device path is tested
    against.  ``ref``: ``(N,3)`` or ``(3N,)``; ``D``: ``(M,N,3)`` or ``(M,3N)``; ``amp``, ``phase``: ``(R,M)`` (or ``(M,)``
    for one run); ``frames`` = ``T``; ``first_frame`` = ``t0``."""
    ref, D, omega_dt, amp, phase = _arguments(ref, D, omega_dt, amp, phase, frames, first_frame)
    for name, array in (("ref", ref), ("D", D), ("omega_dt", omega_dt), ("amp", amp), ("phase", phase)):
        if not np.all(np.isfinite(array)):
            raise ValueError(f"{name} has a non-finite entry")
    runs, columns = len(amp), ref.size
    out = np.empty((runs, int(frames), columns))
    for start in range(0, int(frames), _HOST_FRAMES):
        stop = min(start + _HOST_FRAMES, int(frames))
        index = np.arange(int(first_frame) + start, int(first_frame) + stop).astype(np.float64)
        product = omega_dt[None, :] * index[:, None]
        for r in range(runs):
            left = np.cos(product + phase[r][None, :])
            left *= amp[r][None, :]
            y = left @ D
            y += ref[None, :]
            out[r, start:stop] = y - np.floor(y)
    return out.reshape(runs, int(frames), columns // 3, 3)


def synthesize_device(ref, D, omega_dt, amp, phase, frames: int, first_frame: int = 0, device: int = 0, out=None):
    """The same positions on the GPU (``rn_ht_synthesize_device``): a contiguous float64 CUDA tensor ``(R,T,N,3)`` on GPU
    ``device``, written by a kernel on torch's current stream, so that work queued on that stream afterwards
    (``calc_polarizabilities_device``, the device VDOS classes, ``moments_device``) reads it in place.  ``out``: a
    tensor of that shape, type and layout to write into (its GPU is then the device); ``None``: a new one.  The inputs
    are host arrays, copied to the GPU before the call returns."""
    import torch
    from ramannoodle_amd import _lib
    ref, D, omega_dt, amp, phase = _arguments(ref, D, omega_dt, amp, phase, frames, first_frame)
    runs, modes, atoms = len(amp), len(D), ref.size // 3
    shape = (runs, int(frames), atoms, 3)
    lib = _lib.load()
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=f"cuda:{int(device)}")
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous() and out.dtype == torch.float64
              and tuple(out.shape) == shape):
        raise ValueError(f"out must be a contiguous float64 CUDA tensor of shape {shape}")
    with torch.cuda.device(out.device):
        stream = torch.cuda.current_stream(out.device).cuda_stream
        rc = lib.rn_ht_synthesize_device(out.device.index, C.c_void_p(ref.ctypes.data), C.c_void_p(D.ctypes.data),
                                         C.c_void_p(omega_dt.ctypes.data), C.c_void_p(amp.ctypes.data),
                                         C.c_void_p(phase.ctypes.data), atoms, modes, runs, int(frames), int(first_frame),
                                         C.c_void_p(out.data_ptr()), C.c_void_p(stream))
    _lib.check_status(rc, "rn_ht_synthesize_device", "rn_ht_last_error")
    return out


def synthesize_download(ref, D, omega_dt, amp, phase, frames: int, first_frame: int = 0, device: int = 0):
    """The same positions computed on GPU ``device`` and copied to a host array ``(R,T,N,3)`` (``rn_ht_synthesize``);
    needs no torch."""
    from ramannoodle_amd import _lib
    ref, D, omega_dt, amp, phase = _arguments(ref, D, omega_dt, amp, phase, frames, first_frame)
    runs, modes, atoms = len(amp), len(D), ref.size // 3
    out = np.empty((runs, int(frames), atoms, 3))
    lib = _lib.load()
    rc = lib.rn_ht_synthesize(int(device), C.c_void_p(ref.ctypes.data), C.c_void_p(D.ctypes.data),
                              C.c_void_p(omega_dt.ctypes.data), C.c_void_p(amp.ctypes.data), C.c_void_p(phase.ctypes.data),
                              atoms, modes, runs, int(frames), int(first_frame), C.c_void_p(out.ctypes.data))
    _lib.check_status(rc, "rn_ht_synthesize", "rn_ht_last_error")
    return out


def phonon_arguments(phonons, lattice, timestep, masses=None, modes=None, min_wavenumber: float = 1.0):
    """``(ref[N][3], D[M][N][3], omega_dt[M], wavenumbers[M], index[M])`` of the definition for the selected modes of
    ``phonons``.  ``modes=None``: every mode whose wavenumber exceeds ``min_wavenumber`` (acoustic, zero and imaginary
    modes cannot be populated); otherwise an integer index array as for ``get_mode_vdos``, of which a mode at or below
    ``min_wavenumber`` is a ``ValueError``, as are a bad or singular ``lattice``, bad ``masses``, ``timestep <= 0``, no
    mode left and a selected mode with ``omega timestep >= pi`` (more than half a cycle per frame: it would alias)."""
    from ramannoodle_amd.dynamics import verify_lattices
    from ramannoodle_amd.exceptions import verify_ndarray_shape
    from ramannoodle_amd.spectrum import _vdos_masses, mode_vectors
    ref = np.ascontiguousarray(phonons._ref_positions, dtype=np.float64)
    atoms = ref.shape[0]
    if lattice is None:
        raise ValueError("a harmonic trajectory needs lattice (3,3), the cell of the phonon calculation")
    verify_ndarray_shape("lattice", np.asarray(lattice), (3, 3))
    lattice = verify_lattices(np.asarray(lattice)[None], 1)[0]
    masses = _vdos_masses(masses, atoms)
    try:
        timestep = float(timestep)
    except (TypeError, ValueError) as exc:
        raise ValueError(f"invalid timestep: {timestep!r}") from exc
    if not (timestep > 0 and np.isfinite(timestep)):
        raise ValueError(f"invalid timestep: {timestep} <= 0")
    try:
        min_wavenumber = float(min_wavenumber)
    except (TypeError, ValueError) as exc:
        raise ValueError(f"invalid min_wavenumber: {min_wavenumber!r}") from exc
    if not min_wavenumber >= 0:
        raise ValueError(f"invalid min_wavenumber: {min_wavenumber} < 0")
    wavenumbers = np.asarray(phonons._wavenumbers)
    if wavenumbers.dtype.kind not in "iuf":
        raise ValueError("the wavenumbers of phonons must be real numbers")
    wavenumbers = wavenumbers.astype(np.float64)
    if modes is None:
        index = np.flatnonzero(wavenumbers > min_wavenumber)
        if index.size == 0:
            raise ValueError(f"no mode left: none of the {len(wavenumbers)} wavenumbers exceeds {min_wavenumber}")
    else:
        index = np.asarray(modes)
        if index.dtype.kind not in "iu" or index.ndim != 1:
            raise ValueError("modes must be a one-dimensional integer array")
        if index.size == 0:
            raise ValueError("modes is empty: no mode left")
        if index.min() < 0 or index.max() >= len(wavenumbers):
            raise ValueError(f"modes must lie in [0, {len(wavenumbers)})")
        bad = np.flatnonzero(~(wavenumbers[index] > min_wavenumber))
        if bad.size:
            raise ValueError(f"mode {int(index[bad[0]])} has the wavenumber {wavenumbers[index[bad[0]]]}, not above "
                             f"min_wavenumber = {min_wavenumber}: it cannot be populated")
    chosen = wavenumbers[index]
    if not np.all(np.isfinite(chosen)):
        raise ValueError(f"mode {int(index[np.flatnonzero(~np.isfinite(chosen))[0]])} has a non-finite wavenumber")
    omega_dt = angular_frequencies(chosen) * timestep
    bad = np.flatnonzero(omega_dt >= np.pi)
    if bad.size:
        raise ValueError(f"mode {int(index[bad[0]])} ({chosen[bad[0]]} 1/cm) turns by {omega_dt[bad[0]]:.4g} rad >= pi per "
                         f"timestep of {timestep} fs: it would alias")
    vectors = mode_vectors(np.asarray(phonons._displacements)[index], lattice, masses)
    D = np.ascontiguousarray((vectors / np.sqrt(masses)[None, :, None]) @ np.linalg.inv(lattice))
    return ref, D, omega_dt, chosen, index


def harmonic_runs(phonons, lattice, temperature, steps, timestep, masses=None, modes=None, min_wavenumber: float = 1.0,
                  statistics: str = "classical", sampling: str = "mean", seed=0, runs: int = 1, on_device: bool = False,
                  device: int = 0) -> NDArray[np.float64]:
    """What ``Phonons.get_harmonic_trajectory`` and ``Phonons.get_harmonic_ensemble`` share: the wrapped positions
    ``(runs, steps, N, 3)`` on the host.  Every ``ValueError`` comes before any device work."""
    ref, D, omega_dt, wavenumbers, _ = phonon_arguments(phonons, lattice, timestep, masses, modes, min_wavenumber)
    temperature = _temperature(temperature)
    if isinstance(steps, (bool, np.bool_)) or not isinstance(steps, (int, np.integer)) or steps < 1:
        raise ValueError(f"steps = {steps!r} must be a positive integer")
    if steps > MAX_FRAME_INDEX:
        raise ValueError(f"steps = {steps} exceeds 2^53")
    amp, phase = draw(wavenumbers, temperature, statistics, sampling, runs, seed)
    if on_device:
        return synthesize_device(ref, D, omega_dt, amp, phase, int(steps), 0, device).cpu().numpy()
    return synthesize_host(ref, D, omega_dt, amp, phase, int(steps), 0)
