"""Quasi-harmonic (principal-mode) analysis of MD runs (an addition): effective modes and frequencies from the run
itself, as a ``Phonons`` object that ``get_mode_vdos``, ``get_mode_raman_spectrum``, ``measure_interference`` and
``fit_peaks`` take unchanged.

The mass-weighted covariance of the atomic displacements is diagonalised; its eigenvectors are the effective modes at the
run's temperature and its eigenvalues (the variances of the mode amplitudes) give the effective frequencies.

Definition.  All float64.  ``x[t]``: wrapped fractional positions of frames ``t = 0..T-1``, flattened to ``K = 3N``
columns, ``j = 3 i + r``; ``a``: an anchor structure, ``K`` values; ``bounds[0..B]``: strictly ascending from 0 to ``T``,
block ``b`` holds frames ``bounds[b] .. bounds[b+1]-1``; ``joined[b]`` in {0, 1}: 1 when the step out of the block's
last frame exists and belongs to block ``b``, 0 when it does not exist (a run boundary, the end of the data); the last
block has ``joined = 0``.

* displacement ``w_t = x_t - a - rint(x_t - a)`` (the minimum image), step ``s_t = x_{t+1} - x_t - rint(x_{t+1} - x_t)``
  for every frame of a block but its last when ``joined[b] = 0``;
* per block ``first[b] = sum_t w_t``, ``second[b][0] = sum_t w_t w_t^T``, ``second[b][1] = sum_t s_t s_t^T`` (both
  ``[K][K]``, full, symmetric bit for bit) and ``counts[b] = (frames, steps)``: plain fractional coordinates, no masses,
  no lattice.  The pooled moments are the sums over the blocks in ascending ``b`` (``pool_moments``).

``moments_host`` states the moments in numpy; ``moments_device`` computes them on the GPU (``include/rn_quasiharmonic.h``),
differing by the order of the sums only.  ``modes_from_moments`` turns moments into modes on the host.

Not checked: every atom must stay within half a cell of its anchor, in every fractional coordinate, for the whole run:
no diffusion.  An atom that hops to another site has a bimodal displacement: its variance grows with the squared hop
length, so the analysis returns a spurious soft "mode" along the hop (a large variance, a low frequency) and the mean
structure puts the atom between its two sites; once it passes half a cell from the anchor the minimum image folds it back
and the displacement jumps by a cell, which spoils every mode the atom takes part in.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
from numpy.typing import NDArray

from ramannoodle_amd._source import is_tensor, source
from ramannoodle_amd.constants import BOLTZMANN_CONSTANT
from ramannoodle_amd.structure import apply_pbc

# The energy unit of the variances, 1 amu Angstrom^2 / fs^2, in eV: u (1e-10 m)^2 / (1e-15 s)^2 = u 1e10 J, divided by
# e J/eV, with CODATA 2018 u = 1.66053906660e-27 kg and e = 1.602176634e-19 C (exact): 103.642696...
_ATOMIC_MASS_KG = 1.66053906660e-27
_ELEMENTARY_CHARGE = 1.602176634e-19
AMU_A2_PER_FS2_IN_EV = _ATOMIC_MASS_KG * 1e10 / _ELEMENTARY_CHARGE


def _per_fs_to_cm1(angular):
    """Angular frequencies in rad/fs as wavenumbers in 1/cm."""
    from ramannoodle_amd.spectrum import _PER_FS_TO_CM1
    return angular * (_PER_FS_TO_CM1 / (2.0 * np.pi))


def _blocks_arguments(frames: int, bounds, joined) -> tuple[NDArray[np.int64], NDArray[np.int32]]:
    bounds = np.ascontiguousarray(bounds, dtype=np.int64)
    joined = np.ascontiguousarray(joined, dtype=np.int32)
    if bounds.ndim != 1 or bounds.size < 2 or joined.shape != (bounds.size - 1,):
        raise ValueError("bounds must hold B + 1 >= 2 values and joined B flags")
    if bounds[0] != 0 or bounds[-1] != frames or np.any(np.diff(bounds) <= 0):
        raise ValueError(f"bounds must ascend strictly from 0 to {frames} frames")
    if np.any((joined != 0) & (joined != 1)) or joined[-1] != 0:
        raise ValueError("joined must hold 0 or 1, and 0 for the last block")
    return bounds, joined


def _frames_arguments(positions, anchor) -> tuple[NDArray[np.float64], NDArray[np.float64]]:
    positions = np.asarray(positions, dtype=np.float64)
    if positions.ndim == 3:
        positions = positions.reshape(len(positions), -1)
    if positions.ndim != 2 or positions.shape[0] < 1 or positions.shape[1] < 3 or positions.shape[1] % 3:
        raise ValueError("positions must be (T,N,3) or (T,3N) with T >= 1 and N >= 1")
    anchor = np.ascontiguousarray(anchor, dtype=np.float64).reshape(-1)
    if anchor.size != positions.shape[1]:
        raise ValueError(f"anchor holds {anchor.size} values, the frames have {positions.shape[1]} columns")
    return np.ascontiguousarray(positions), anchor


def _symmetric(matrix):
    """The lower triangle of ``matrix`` and its mirror: symmetric bit for bit."""
    lower = np.tril(matrix)
    return lower + np.tril(matrix, -1).T


def moments_host(positions, anchor, bounds, joined):
    """``(first[B][K], second[B][2][K][K], counts[B][2])`` of the module's definition, in numpy: the statement the device
    path is tested against.  ``positions``: ``(T,N,3)`` or ``(T,3N)``."""
    x, anchor = _frames_arguments(positions, anchor)
    bounds, joined = _blocks_arguments(len(x), bounds, joined)
    blocks, columns = len(joined), x.shape[1]
    first = np.zeros((blocks, columns))
    second = np.zeros((blocks, 2, columns, columns))
    counts = np.zeros((blocks, 2), dtype=np.int64)
    for b in range(blocks):
        lo, hi = int(bounds[b]), int(bounds[b + 1])
        w = x[lo:hi] - anchor
        w = w - np.rint(w)
        steps = hi - lo - 1 + int(joined[b])
        s = x[lo + 1:lo + 1 + steps] - x[lo:lo + steps]
        s = s - np.rint(s)
        first[b] = w.sum(axis=0)
        second[b, 0] = _symmetric(w.T @ w)
        second[b, 1] = _symmetric(s.T @ s)
        counts[b] = (hi - lo, steps)
    return first, second, counts


def moments_device(positions, anchor, bounds, joined, device: int = 0):
    """The same moments on GPU ``device`` (``rn_qh_moments``).  ``positions``: a host array as for ``moments_host``, or
    a contiguous float64 CUDA tensor ``(T,N,3)`` / ``(T,3N)``, which is read where it is, on its GPU, ordered after
    torch's current stream (``rn_qh_moments_device``).  ``first``, ``second`` and ``counts`` come back as host arrays."""
    from ramannoodle_amd import _lib
    if is_tensor(positions):
        pointer, device, stream, _ = source(positions, "a tensor of positions must be a contiguous float64 CUDA tensor")
        if positions.dim() not in (2, 3) or positions.shape[0] < 1 or positions[0].numel() < 3 or positions[0].numel() % 3:
            raise ValueError("positions must be (T,N,3) or (T,3N) with T >= 1 and N >= 1")
        frames, columns = positions.shape[0], positions[0].numel()
        anchor = np.ascontiguousarray(anchor, dtype=np.float64).reshape(-1)
        if anchor.size != columns:
            raise ValueError(f"anchor holds {anchor.size} values, the frames have {columns} columns")
    else:
        host, anchor = _frames_arguments(positions, anchor)
        frames, columns = host.shape
        pointer, stream = host.ctypes.data, None
    bounds, joined = _blocks_arguments(frames, bounds, joined)
    blocks = len(joined)
    first = np.zeros((blocks, columns))
    second = np.zeros((blocks, 2, columns, columns))
    counts = np.zeros((blocks, 2), dtype=np.int64)
    lib = _lib.load()
    entry = lib.rn_qh_moments if stream is None else lib.rn_qh_moments_device
    tail = () if stream is None else (C.c_void_p(stream),)
    rc = entry(int(device), C.c_void_p(pointer), frames, columns // 3, C.c_void_p(anchor.ctypes.data),
               C.c_void_p(bounds.ctypes.data), C.c_void_p(joined.ctypes.data), blocks, C.c_void_p(first.ctypes.data),
               C.c_void_p(second.ctypes.data), C.c_void_p(counts.ctypes.data), *tail)
    _lib.check_status(rc, "rn_qh_moments", "rn_qh_last_error")
    return first, second, counts


def chunk_frames() -> int:
    """The frames of a chunk of the device sums (``rn_qh_chunk_frames``)."""
    from ramannoodle_amd import _lib
    return int(_lib.load().rn_qh_chunk_frames())


def pool_moments(first, second, counts):
    """The pooled moments ``(first[K], second[2][K][K], counts[2])``: the sums over the blocks in ascending order."""
    total_first, total_second, total_counts = first[0].copy(), second[0].copy(), counts[0].copy()
    for b in range(1, len(first)):
        total_first += first[b]
        total_second += second[b]
        total_counts += counts[b]
    return total_first, total_second, total_counts


@dataclass(frozen=True)
class QuasiHarmonicModes:
    """The result of ``get_quasiharmonic_modes`` / ``modes_from_moments``; every per-mode array is in the order of
    ``phonons``, ascending in its wavenumbers.

    ``phonons``: a ``Phonons`` about ``mean_positions`` whose wavenumbers are the temperature estimate when a temperature
    was given and the steps estimate otherwise; ``wavenumbers_steps`` ``(M,)``; ``wavenumbers_temperature`` ``(M,)`` or
    ``None``; ``variances`` ``(M,)`` in amu Angstrom^2; ``vectors`` ``(M,N,3)``, the mass-weighted unit eigenvectors;
    ``mean_positions`` ``(N,3)``, fractional and wrapped; ``rank`` = ``M``; ``block_variances`` and ``block_wavenumbers``
    ``(blocks, M)``: each block's own variance along the pooled vectors and its steps estimate (NaN for a block without
    steps); ``wavenumber_errors`` ``(M,)``: the standard error of ``block_wavenumbers`` over the blocks, NaN for one block;
    ``counts``: the pooled ``(frames, steps)``."""
    phonons: object
    wavenumbers_steps: NDArray[np.float64]
    wavenumbers_temperature: NDArray[np.float64] | None
    variances: NDArray[np.float64]
    vectors: NDArray[np.float64]
    mean_positions: NDArray[np.float64]
    rank: int
    block_variances: NDArray[np.float64]
    block_wavenumbers: NDArray[np.float64]
    wavenumber_errors: NDArray[np.float64]
    counts: NDArray[np.int64]


def _steps_wavenumbers(variances, step_variances, timestep: float):
    """``arccos(clip(1 - sigma / (2 lambda), -1, 1)) / timestep`` in 1/cm: exact for a sampled harmonic oscillation,
    because ``<(q(t + dt) - q(t))^2> = 2 lambda (1 - cos(omega dt))``."""
    with np.errstate(invalid="ignore", divide="ignore"):
        cosine = np.clip(1.0 - step_variances / (2.0 * variances), -1.0, 1.0)
    return _per_fs_to_cm1(np.arccos(cosine) / timestep)


def _quotients(matrix, vectors):
    """``v_i^T matrix v_i`` of the columns ``v_i``."""
    return np.einsum("ki,ki->i", vectors, matrix @ vectors)


def modes_from_moments(first, second, counts, lattice, masses, timestep, temperature=None, remove_translations=True,
                       rank_tolerance=1e-10, anchor=None) -> QuasiHarmonicModes:
    """Modes from the block moments ``first[B][K]``, ``second[B][2][K][K]``, ``counts[B][2]`` (``moments_host``,
    ``moments_device``).  With ``G`` block diagonal with blocks ``sqrt(m_i) L^T`` (fractional to mass-weighted Cartesian
    coordinates) and the pooled sums over ``T`` frames and ``T_s`` steps,

    ``B = G (second_0 / T - first first^T / T^2) G^T`` and ``S = G (second_1 / T_s) G^T``;

    with ``remove_translations`` both become ``P . P``, ``P = 1 - sum_r t_r t_r^T``, ``t_r[3i+s] = sqrt(m_i / sum m)
    delta_rs``.  ``numpy.linalg.eigh`` of ``B``, sorted descending in the eigenvalue, keeps ``lambda_i > rank_tolerance
    lambda_max``: ``M`` modes (the rank) with unit vectors ``u_i``.  Two frequency estimates: from the steps, with
    ``sigma_i = u_i^T S u_i``, ``omega_i = arccos(clip(1 - sigma_i / (2 lambda_i), -1, 1)) / timestep`` (no temperature
    needed); and, when ``temperature`` (K) is given, equipartition, ``omega_i = sqrt(k_B T / (c lambda_i))`` with ``c =
    AMU_A2_PER_FS2_IN_EV``.  ``mean_positions = apply_pbc(anchor + first / T)`` (``anchor=None``: zeros); the fractional
    displacements of ``phonons`` are ``D[m,i] = (u_m[i] / sqrt(m_i)) @ inv(L)``, so that ``spectrum.mode_vectors`` gives
    back ``u``.  Per block, along the pooled ``u_i``: the Rayleigh quotient of the block's own centred ``B_b`` and the
    steps estimate from the block's ``B_b`` and ``S_b``.  ``ValueError`` when no eigenvalue is positive (rank 0)."""
    from ramannoodle_amd.dynamics import Phonons
    first = np.asarray(first, dtype=np.float64)
    second = np.asarray(second, dtype=np.float64)
    counts = np.asarray(counts, dtype=np.int64)
    lattice = np.asarray(lattice, dtype=np.float64)
    masses = np.asarray(masses, dtype=np.float64)
    blocks, columns = first.shape
    atoms = columns // 3
    if second.shape != (blocks, 2, columns, columns) or counts.shape != (blocks, 2) or masses.shape != (atoms,):
        raise ValueError("first, second, counts and masses do not belong together")
    if temperature is not None and not temperature > 0:
        raise ValueError(f"invalid temperature: {temperature} <= 0")
    root = np.sqrt(masses)
    metric = (np.eye(atoms)[:, None, :, None] * (root[:, None, None, None] * lattice.T[None, :, None, :]))
    metric = metric.reshape(columns, columns)  # G
    projector = np.eye(columns)
    if remove_translations:
        translations = (np.sqrt(masses / masses.sum())[:, None, None] * np.eye(3)[None]).reshape(columns, 3)
        projector = projector - translations @ translations.T

    def covariances(block_first, block_second, block_counts):
        """(centred displacement covariance, step second moment) in fractional coordinates"""
        frames, steps = int(block_counts[0]), int(block_counts[1])
        mean = block_first / frames
        with np.errstate(invalid="ignore", divide="ignore"):
            return block_second[0] / frames - np.outer(mean, mean), block_second[1] / np.float64(steps)

    total_first, total_second, total_counts = pool_moments(first, second, counts)
    if total_counts[1] < 1:
        raise ValueError("the moments hold no step")
    displacement, step = covariances(total_first, total_second, total_counts)
    left = projector @ metric
    values, vectors = np.linalg.eigh(left @ displacement @ left.T)
    values, vectors = values[::-1], vectors[:, ::-1]
    keep = values > rank_tolerance * values[0] if values[0] > 0 else np.zeros(columns, dtype=bool)
    rank = int(keep.sum())
    if rank == 0:
        raise ValueError("the displacement covariance has rank 0: the frames do not move")
    values, vectors = values[keep], vectors[:, keep]
    step_values = _quotients(left @ step @ left.T, vectors)
    wavenumbers_steps = _steps_wavenumbers(values, step_values, timestep)
    wavenumbers_temperature = None
    if temperature is not None:
        wavenumbers_temperature = _per_fs_to_cm1(np.sqrt(BOLTZMANN_CONSTANT * temperature / (AMU_A2_PER_FS2_IN_EV * values)))

    # per block along the pooled vectors: u^T P G C G^T P u = v^T C v with v = G^T P u
    dual = left.T @ vectors
    block_variances = np.zeros((blocks, rank))
    block_wavenumbers = np.full((blocks, rank), np.nan)
    for b in range(blocks):
        block_displacement, block_step = covariances(first[b], second[b], counts[b])
        block_variances[b] = _quotients(block_displacement, dual)
        if counts[b, 1] > 0:
            block_wavenumbers[b] = _steps_wavenumbers(block_variances[b], _quotients(block_step, dual), timestep)
    if blocks > 1:
        errors = block_wavenumbers.std(axis=0, ddof=1) / np.sqrt(blocks)
    else:
        errors = np.full(rank, np.nan)

    chosen = wavenumbers_steps if wavenumbers_temperature is None else wavenumbers_temperature
    order = np.argsort(chosen, kind="stable")
    unit = np.ascontiguousarray(vectors.T[order].reshape(rank, atoms, 3))
    mean = (0.0 if anchor is None else np.asarray(anchor, dtype=np.float64).reshape(atoms, 3))
    mean_positions = apply_pbc(mean + (total_first / total_counts[0]).reshape(atoms, 3))
    displacements = np.ascontiguousarray((unit / root[None, :, None]) @ np.linalg.inv(lattice))
    return QuasiHarmonicModes(
        phonons=Phonons(mean_positions, np.ascontiguousarray(chosen[order]), displacements),
        wavenumbers_steps=wavenumbers_steps[order],
        wavenumbers_temperature=None if wavenumbers_temperature is None else wavenumbers_temperature[order],
        variances=values[order], vectors=unit, mean_positions=mean_positions, rank=rank,
        block_variances=block_variances[:, order], block_wavenumbers=block_wavenumbers[:, order],
        wavenumber_errors=errors[order], counts=total_counts)


def run_blocks(run_lengths, blocks: int) -> tuple[NDArray[np.int64], NDArray[np.int32]]:
    """``(bounds, joined)`` of joined runs of ``run_lengths`` frames, each cut into ``blocks`` contiguous blocks: within a
    run ``bounds[b] = floor(b n / blocks)`` and ``joined = 1`` but for the run's last block, so no step crosses a run
    boundary."""
    bounds, joined, offset = [0], [], 0
    for length in run_lengths:
        bounds += [offset + (b * length) // blocks for b in range(1, blocks + 1)]
        joined += [1] * (blocks - 1) + [0]
        offset += length
    return np.array(bounds, dtype=np.int64), np.array(joined, dtype=np.int32)


def quasiharmonic_modes(positions_ts, run_lengths, timestep: float, lattice, masses=None, temperature=None,
                        ref_positions=None, blocks: int = 1, remove_translations: bool = True, on_device: bool = False,
                        device: int = 0) -> QuasiHarmonicModes:
    """What ``Trajectory.get_quasiharmonic_modes`` and ``TrajectoryEnsemble.get_quasiharmonic_modes`` share:
    ``positions_ts`` ``(S,N,3)`` are the joined frames of runs of ``run_lengths`` frames.  Every ``ValueError`` comes
    before any device work."""
    from ramannoodle_amd.dynamics import verify_lattices
    from ramannoodle_amd.exceptions import verify_ndarray_shape
    from ramannoodle_amd.spectrum import _vdos_masses
    frames, atoms = positions_ts.shape[0], positions_ts.shape[1]
    if min(run_lengths) < 2:
        raise ValueError("quasi-harmonic modes need at least 2 frames of every run")
    if isinstance(blocks, (bool, np.bool_)) or not isinstance(blocks, (int, np.integer)) or blocks < 1:
        raise ValueError(f"blocks = {blocks!r} must be a positive integer")
    if blocks > min(run_lengths):
        raise ValueError(f"blocks = {blocks} is more than the {min(run_lengths)} frames of a run")
    if lattice is None:
        raise ValueError("get_quasiharmonic_modes needs lattice (3,3)")
    verify_ndarray_shape("lattice", np.asarray(lattice), (3, 3))
    lattice = verify_lattices(np.asarray(lattice)[None], 1)[0]
    masses = _vdos_masses(masses, atoms)
    if temperature is not None:
        temperature = float(temperature)
        if not temperature > 0:
            raise ValueError(f"invalid temperature: {temperature} <= 0")
    if ref_positions is None:
        anchor = positions_ts[0]
    else:
        anchor = np.asarray(ref_positions)
        if anchor.shape != (atoms, 3) or anchor.dtype.kind not in "iuf":
            raise ValueError(f"ref_positions has wrong shape or type: {anchor.shape} != ({atoms}, 3) reals")
    anchor = np.ascontiguousarray(anchor, dtype=np.float64)
    if not np.all(np.isfinite(anchor)):
        raise ValueError("ref_positions has a non-finite entry")
    bounds, joined = run_blocks(run_lengths, int(blocks))
    assert bounds[-1] == frames
    if on_device:
        import torch
        positions = torch.tensor(positions_ts, dtype=torch.float64, device=f"cuda:{int(device)}")
        first, second, counts = moments_device(positions, anchor, bounds, joined)
    else:
        first, second, counts = moments_host(positions_ts, anchor, bounds, joined)
    return modes_from_moments(first, second, counts, lattice, masses, timestep, temperature, remove_translations,
                              anchor=anchor)
