"""Callers of the polarizability model: phonons and MD trajectories
(``ramannoodle/dynamics/_phonon.py``, ``ramannoodle/dynamics/_trajectory.py``)."""
from __future__ import annotations

from collections.abc import Sequence

import numpy as np
from numpy.typing import NDArray

from ramannoodle_amd.abstract import Dynamics, PolarizabilityModel
from ramannoodle_amd.constants import RAMAN_TENSOR_CENTRAL_DIFFERENCE
from ramannoodle_amd.exceptions import get_type_error, verify_ndarray_shape
from ramannoodle_amd.spectrum import MDRamanSpectrum, PhononRamanSpectrum
from ramannoodle_amd.structure import apply_pbc


SINGULAR_VOLUME = 1e-12  # |det L| <= this times |a| |b| |c|: a singular lattice


def verify_lattices(lattice_ts, frames: int) -> NDArray[np.float64]:
    """The lattices of a variable-cell trajectory as float64 ``(frames,3,3)`` (rows = lattice vectors in Angstrom):
    ``ValueError`` on another shape, a non-finite entry or a singular lattice, naming the first offending frame."""
    verify_ndarray_shape("lattice_ts", lattice_ts, (frames, 3, 3))
    lattices = np.array(lattice_ts, dtype=np.float64)
    bad = np.nonzero(~np.isfinite(lattices).all(axis=(1, 2)))[0]
    if bad.size:
        raise ValueError(f"lattice_ts[{bad[0]}] has a non-finite entry")
    # a determinant of zero, within the rounding of its products (the library's rule: csrc/api.hip, check_lattices)
    bad = np.nonzero(~(np.abs(np.linalg.det(lattices)) > SINGULAR_VOLUME * np.linalg.norm(lattices, axis=2).prod(axis=1)))[0]
    if bad.size:
        raise ValueError(f"lattice_ts[{bad[0]}] is singular")
    return lattices


class Phonons(Dynamics):
    """Harmonic lattice vibrations: wavenumbers ``(M,)`` and fractional displacements
    ``(M,N,3)`` about ``ref_positions`` ``(N,3)`` (``dynamics/_phonon.py:13-108``)."""

    def __init__(self, ref_positions, wavenumbers, displacements) -> None:
        verify_ndarray_shape("ref_positions", ref_positions, (None, 3))
        verify_ndarray_shape("wavenumbers", wavenumbers, (None,))
        verify_ndarray_shape("displacements", displacements,
                             (wavenumbers.size, ref_positions.shape[0], 3))
        self._ref_positions = ref_positions
        self._wavenumbers = wavenumbers
        self._displacements = displacements

    @property
    def ref_positions(self):
        return self._ref_positions.copy()

    @property
    def wavenumbers(self):
        return self._wavenumbers.copy()

    @property
    def displacements(self):
        return self._displacements.copy()

    def get_raman_spectrum(self, polarizability_model: PolarizabilityModel) -> PhononRamanSpectrum:
        """Raman tensors by the reference's finite difference
        ``(alpha(r + delta d) - alpha(r - delta d)) / delta`` with ``delta = 1e-3``
        (divided by ``delta``, not ``2 delta``: ``dynamics/_phonon.py:93-106``).

        A model exposing ``calc_raman_tensors`` (the device PotGNN) evaluates all ``2M``
        displaced cells in one float64 batch; any other model goes through the
        reference's per-mode loop.
        """
        delta = RAMAN_TENSOR_CENTRAL_DIFFERENCE
        batched = getattr(polarizability_model, "calc_raman_tensors", None)
        try:
            if batched is not None:
                raman_tensors = batched(self._ref_positions, self._displacements, delta)
            else:
                tensors = []
                for displacement in self._displacements:
                    eps = displacement * delta
                    plus = polarizability_model.calc_polarizabilities(
                        np.array([self._ref_positions + eps]))[0]
                    minus = polarizability_model.calc_polarizabilities(
                        np.array([self._ref_positions - eps]))[0]
                    tensors.append((plus - minus) / delta)
                raman_tensors = np.array(tensors)
        except ValueError as exc:
            raise ValueError("polarizability_model and phonons are incompatible") from exc
        return PhononRamanSpectrum(self._wavenumbers, raman_tensors)

    def get_partial_raman_spectrum(self, polarizability_model: PolarizabilityModel, groups):
        """Atom-group decomposition of the spectrum (an addition): ``PartialPhononRamanSpectrum`` of the partial Raman
        tensors ``R[m,g] = 2 sum_{i in g} J_i . d_{m,i}`` at the reference positions.  ``groups``: an integer array
        ``(N,)`` or ``"species"`` (``spectrum.group_labels``).  Needs a model with ``calc_partial_raman_tensors`` (the
        device PotGNN): finite differences of masked displacements are not exactly additive, so there is no fallback."""
        from ramannoodle_amd.spectrum import PartialPhononRamanSpectrum
        partial = getattr(polarizability_model, "calc_partial_raman_tensors", None)
        if partial is None:
            raise TypeError(f"{type(polarizability_model).__name__} has no calc_partial_raman_tensors: partial spectra "
                            "need the Jacobian of the model (the device PotGNN)")
        try:
            tensors = partial(self._ref_positions, self._displacements, groups)
        except ValueError as exc:
            raise ValueError(f"polarizability_model and phonons are incompatible: {exc}") from exc
        return PartialPhononRamanSpectrum(self._wavenumbers, tensors)

    def get_harmonic_trajectory(self, lattice, temperature, steps, timestep, masses=None, modes=None,
                                min_wavenumber: float = 1.0, statistics: str = "classical", sampling: str = "mean",
                                seed=0, on_device: bool = False, device: int = 0):
        """A harmonic trajectory of the phonons (an addition): a ``Trajectory`` of ``steps`` frames, ``timestep`` fs
        apart, of the atoms moving along the modes with thermal amplitudes at ``temperature`` (K) and random phases
        (``ramannoodle_amd.harmonic`` states the definition), for every analysis that starts from a ``Trajectory``.
        ``lattice`` ``(3,3)``: the cell of the phonon calculation; ``masses`` ``(N,)`` (``None``: unit masses);
        ``modes=None``: every mode whose wavenumber exceeds ``min_wavenumber`` (acoustic, zero and imaginary modes cannot
        be populated), otherwise an integer index array as for ``get_mode_vdos``; ``statistics``: ``"classical"``
        (``k_B T`` per mode) or ``"quantum"`` (with zero-point motion); ``sampling``: ``"mean"`` (every mode at its mean
        energy) or ``"random"`` (energies drawn from the thermal distribution); ``seed``: of the phases and energies.
        ``on_device=True``: the positions are synthesised on GPU ``device`` and copied to the host; the route that keeps
        them in HBM is ``harmonic.synthesize_device``.  ``ValueError``, before any device work: a bad or singular
        ``lattice``, bad ``masses``, ``temperature <= 0``, ``steps < 1``, ``timestep <= 0``, a selected mode at or below
        ``min_wavenumber`` or turning by pi or more per timestep, an unknown ``statistics`` or ``sampling``, no mode
        left.  Not checked: amplitudes beyond half a cell."""
        from ramannoodle_amd.harmonic import harmonic_runs
        positions = harmonic_runs(self, lattice, temperature, steps, timestep, masses, modes, min_wavenumber, statistics,
                                  sampling, seed, 1, on_device, device)
        return Trajectory(positions[0], timestep)

    def get_harmonic_ensemble(self, lattice, temperature, steps, timestep, masses=None, modes=None,
                              min_wavenumber: float = 1.0, statistics: str = "classical", sampling: str = "mean", seed=0,
                              on_device: bool = False, device: int = 0, runs: int = 1):
        """``runs`` independent harmonic trajectories (``get_harmonic_trajectory``; run 0 is the trajectory of the same
        seed) as a ``TrajectoryEnsemble``: averaging over the runs cancels the cross terms between modes.  ``runs < 1``
        is a ``ValueError``."""
        from ramannoodle_amd.harmonic import harmonic_runs
        positions = harmonic_runs(self, lattice, temperature, steps, timestep, masses, modes, min_wavenumber, statistics,
                                  sampling, seed, runs, on_device, device)
        return TrajectoryEnsemble([Trajectory(run, timestep) for run in positions])


def _cells(lattice_ts, device=None) -> dict:
    """The ``lattices`` keyword of a variable-cell run for the model's entries (on ``device``: as a tensor); nothing for
    a fixed cell, so that models without the keyword keep working."""
    if lattice_ts is None:
        return {}
    if device is None:
        return {"lattices": lattice_ts}
    import torch
    return {"lattices": torch.tensor(lattice_ts, dtype=torch.float64, device=device)}



def _vdos_arguments(lattice, lattice_ts, masses, groups, atomic_numbers, atoms: int):
    """``(lattice, masses, labels, G)`` of ``get_vdos``: the fixed-cell ``lattice`` ``(3,3)`` or the trajectory's own
    ``lattice_ts`` (exactly one of the two), and ``groups`` resolved through ``spectrum.group_labels``."""
    from ramannoodle_amd.spectrum import group_labels
    if lattice_ts is None:
        if lattice is None:
            raise ValueError("a fixed-cell trajectory needs lattice (3,3)")
        verify_ndarray_shape("lattice", np.asarray(lattice), (3, 3))
        lattice = verify_lattices(np.asarray(lattice)[None], 1)[0]
    elif lattice is not None:
        raise ValueError("the trajectory carries a lattice per frame: lattice must be None")
    else:
        lattice = lattice_ts
    if groups is None:
        return lattice, masses, None, 1
    if atomic_numbers is None:
        if isinstance(groups, str):
            raise ValueError(f"groups = {groups!r} needs atomic_numbers")
        atomic_numbers = np.zeros(atoms, dtype=np.int64)
    else:
        verify_ndarray_shape("atomic_numbers", np.asarray(atomic_numbers), (atoms,))
    labels, count = group_labels(groups, atomic_numbers)
    return lattice, masses, labels, count


def _mode_vdos_arguments(phonons, lattice, lattice_ts, masses, modes, atoms: int):
    """``(lattice of the steps, vectors)`` of ``get_mode_vdos``: ``lattice`` ``(3,3)`` is the cell of the phonon
    calculation and, unless the trajectory carries ``lattice_ts``, of the steps; ``modes`` selects rows of ``phonons``."""
    from ramannoodle_amd.spectrum import mode_vectors
    if not isinstance(phonons, Phonons):
        raise get_type_error("phonons", phonons, "Phonons")
    if lattice is None:
        raise ValueError("get_mode_vdos needs lattice (3,3), the cell of the phonon calculation")
    verify_ndarray_shape("lattice", np.asarray(lattice), (3, 3))
    lattice = verify_lattices(np.asarray(lattice)[None], 1)[0]
    displacements = phonons._displacements
    if displacements.shape[1] != atoms:
        raise ValueError(f"phonons and trajectory are incompatible: {displacements.shape[1]} atoms != {atoms} atoms")
    if modes is not None:
        index = np.asarray(modes)
        if index.dtype.kind not in "iu" or index.ndim != 1:
            raise ValueError("modes must be a one-dimensional integer array")
        if index.size == 0:
            raise ValueError("modes is empty")
        if index.min() < 0 or index.max() >= len(displacements):
            raise ValueError(f"modes must lie in [0, {len(displacements)})")
        displacements = displacements[index]
    vectors = mode_vectors(displacements, lattice, np.ones(atoms) if masses is None else masses)
    return (lattice if lattice_ts is None else lattice_ts), vectors


def _mode_increments(polarizability_model, positions_ts, lattice_ts, phonons, lattice, masses, modes, rest):
    """The per-mode increments of ``get_mode_raman_spectrum`` over the frames ``positions_ts``, a CUDA tensor
    ``(S-1,C,3,3)`` (``PotGNN.calc_mode_increments_device``)."""
    from ramannoodle_amd.spectrum import _projectors_of_vectors, _vdos_masses
    increments = getattr(polarizability_model, "calc_mode_increments_device", None)
    if increments is None:
        raise TypeError(f"{type(polarizability_model).__name__} has no calc_mode_increments_device: mode spectra "
                        "need the Jacobian of the model (the device PotGNN)")
    atoms = positions_ts.shape[1]
    if lattice is None:
        lattice = getattr(polarizability_model, "ref_lattice", None)
        if lattice is None:
            raise ValueError("get_mode_raman_spectrum needs lattice (3,3): the model has no ref_lattice")
    # (the cell of the steps is not needed: the projection happens in fractional coordinates)
    _, vectors = _mode_vdos_arguments(phonons, lattice, None, masses, modes, atoms)
    displacements, projectors = _projectors_of_vectors(vectors, np.asarray(lattice, dtype=np.float64),
                                                       _vdos_masses(masses, atoms))
    import torch
    try:
        verify_ndarray_shape("positions_ts", positions_ts, (None, polarizability_model.num_atoms, 3))
        positions = torch.tensor(positions_ts, dtype=torch.float64, device=f"cuda:{polarizability_model.device_index}")
        return increments(positions, displacements, projectors, rest=rest, **_cells(lattice_ts, positions.device))
    except ValueError as exc:
        raise ValueError(f"polarizability_model and trajectory are incompatible: {exc}") from exc


def _descriptors(model, positions_ts, lattice_ts, on_device: bool):
    """What ``Trajectory.get_descriptors`` and ``TrajectoryEnsemble.get_descriptors`` share."""
    if getattr(model, "calc_descriptors", None) is None:
        raise TypeError("descriptors need a model with a latent space (the device PotGNN): calc_descriptors")
    try:
        if on_device:
            import torch
            verify_ndarray_shape("positions_batch", positions_ts, (None, model.num_atoms, 3))
            positions = torch.tensor(positions_ts, dtype=torch.float64, device=f"cuda:{model.device_index}")
            return model.calc_descriptors_device(positions, **_cells(lattice_ts, positions.device))
        return model.calc_descriptors(positions_ts, **_cells(lattice_ts))
    except ValueError as exc:
        raise ValueError("polarizability_model and trajectory are incompatible") from exc


class Trajectory(Dynamics, Sequence):
    """MD trajectory: fractional positions ``(S,N,3)`` (wrapped into the cell on
    construction) and a timestep in fs (``dynamics/_trajectory.py:16-109``).

    ``lattice_ts`` (an addition; the reference knows one fixed cell): ``(S,3,3)``, the lattice of every frame of a
    variable-cell run (NPT, a heating ramp, a pressure scan), rows = lattice vectors in Angstrom, finite and
    non-singular.  The spectra then evaluate every frame in its own cell, and the partial spectrum has one more
    group, the last: the cell (``PotGNN.calc_group_increments_device``).  ``None``: the model's reference cell."""

    def __init__(self, positions_ts, timestep: float, lattice_ts=None) -> None:
        verify_ndarray_shape("positions_ts", positions_ts, (None, None, 3))
        try:
            timestep = float(timestep)
        except TypeError as exc:
            raise get_type_error("timestep", timestep, "float") from exc
        if timestep <= 0:
            raise ValueError("timestep must be positive")
        self._positions_ts = apply_pbc(positions_ts)
        self._timestep = timestep
        self._lattice_ts = None if lattice_ts is None else verify_lattices(lattice_ts, len(self._positions_ts))

    @property
    def positions_ts(self):
        return self._positions_ts.copy()

    @property
    def lattice_ts(self):
        """The lattice of every frame ``(S,3,3)`` (a copy), or ``None`` for a fixed cell."""
        return None if self._lattice_ts is None else self._lattice_ts.copy()

    @property
    def timestep(self) -> float:
        return self._timestep

    def get_raman_spectrum(self, polarizability_model: PolarizabilityModel,
                           on_device: bool = False) -> MDRamanSpectrum:
        """``dynamics/_trajectory.py:71-90``.  ``on_device=True`` (an addition; needs the device
        PotGNN): the polarizability time series stays in HBM and the returned
        ``DeviceMDRamanSpectrum`` reduces it there, so only the intensities reach the host."""
        try:
            if on_device:
                import torch
                from ramannoodle_amd.spectrum import DeviceMDRamanSpectrum
                evaluate = getattr(polarizability_model, "calc_polarizabilities_device", None)
                if evaluate is None:
                    raise TypeError("on_device=True needs a model with calc_polarizabilities_device")
                verify_ndarray_shape("positions_batch", self._positions_ts,
                                     (None, polarizability_model.num_atoms, 3))
                positions = torch.tensor(self._positions_ts, dtype=torch.float64,
                                         device=f"cuda:{polarizability_model.device_index}")
                return DeviceMDRamanSpectrum(evaluate(positions, **_cells(self._lattice_ts, positions.device)),
                                             self._timestep)
            polarizability_ts = polarizability_model.calc_polarizabilities(self._positions_ts, **_cells(self._lattice_ts))
        except ValueError as exc:
            raise ValueError("polarizability_model and trajectory are incompatible") from exc
        return MDRamanSpectrum(polarizability_ts, self._timestep)

    def get_descriptors(self, model, on_device: bool = False):
        """Structure descriptors of every frame (an addition; ``PotGNN.calc_descriptors``): ``(S, columns)`` float64, a
        host array, or with ``on_device=True`` a CUDA tensor that never leaves HBM (``calc_descriptors_device``).  A
        trajectory with ``lattice_ts`` is evaluated in each frame's own cell."""
        return _descriptors(model, self._positions_ts, self._lattice_ts, on_device)

    def get_partial_raman_spectrum(self, polarizability_model: PolarizabilityModel, groups, on_device: bool = False):
        """Atom-group decomposition of the spectrum (an addition): ``PartialMDRamanSpectrum`` of the per-group trapezoid
        increments of the polarizability (``PotGNN.calc_group_increments``).  ``groups``: an integer array ``(N,)`` or
        ``"species"`` (``spectrum.group_labels``).  ``on_device=True``: the increments stay in HBM and the returned
        ``DevicePartialMDRamanSpectrum`` reduces them there.  Needs a model with ``calc_group_increments_device`` (the
        device PotGNN); there is no fallback."""
        import torch
        from ramannoodle_amd.spectrum import DevicePartialMDRamanSpectrum, PartialMDRamanSpectrum
        increments = getattr(polarizability_model, "calc_group_increments_device", None)
        if increments is None:
            raise TypeError(f"{type(polarizability_model).__name__} has no calc_group_increments_device: partial spectra "
                            "need the Jacobian of the model (the device PotGNN)")
        try:
            verify_ndarray_shape("positions_ts", self._positions_ts, (None, polarizability_model.num_atoms, 3))
            positions = torch.tensor(self._positions_ts, dtype=torch.float64,
                                     device=f"cuda:{polarizability_model.device_index}")
            result = increments(positions, groups, **_cells(self._lattice_ts, positions.device))
        except ValueError as exc:
            raise ValueError(f"polarizability_model and trajectory are incompatible: {exc}") from exc
        if on_device:
            return DevicePartialMDRamanSpectrum(result, self._timestep)
        return PartialMDRamanSpectrum(result.cpu().numpy(), self._timestep)

    def get_vdos(self, lattice=None, masses=None, groups=None, atomic_numbers=None, on_device: bool = False,
                 device: int = 0):
        """The vibrational density of states of the run (an addition): ``VibrationalDensityOfStates`` of the positions,
        on the wavenumber axis of ``get_raman_spectrum(...).measure()``.  ``lattice`` ``(3,3)``: required for a fixed
        cell, ``None`` when the trajectory carries ``lattice_ts`` (either violation is a ``ValueError``); ``masses``
        ``(N,)``, finite and positive (``None``: unit masses); ``groups``: ``None`` (one group), an integer array
        ``(N,)`` or ``"species"``, which needs ``atomic_numbers`` (``spectrum.group_labels``).  ``on_device=True``: the
        positions (and the lattices of a variable-cell run) are put into the HBM of GPU ``device`` and the returned
        ``DeviceVibrationalDensityOfStates`` reduces them there."""
        from ramannoodle_amd.spectrum import DeviceVibrationalDensityOfStates, VibrationalDensityOfStates
        lattice, masses, labels, count = _vdos_arguments(lattice, self._lattice_ts, masses, groups, atomic_numbers,
                                                         self._positions_ts.shape[1])
        if not on_device:
            return VibrationalDensityOfStates(self._positions_ts, self._timestep, lattice, masses, labels, count)
        import torch
        positions = torch.tensor(self._positions_ts, dtype=torch.float64, device=f"cuda:{int(device)}")
        if self._lattice_ts is not None:
            lattice = torch.tensor(lattice, dtype=torch.float64, device=positions.device)
        return DeviceVibrationalDensityOfStates(positions, self._timestep, lattice, masses, labels, count)

    def get_mode_vdos(self, phonons, lattice, masses=None, modes=None, on_device: bool = False, device: int = 0):
        """The mode-projected VDOS of the run (an addition): ``ModeVibrationalDensityOfStates`` of the positions and
        the mass-weighted, normalised eigenvectors of ``phonons`` (``spectrum.mode_vectors``), one row per mode, on the
        wavenumber axis of ``get_vdos(...).measure()`` and ``get_raman_spectrum(...).measure()``.  ``lattice`` ``(3,3)``,
        always required, is the cell of the phonon calculation: it takes the displacements to Cartesian coordinates and
        is the cell of the steps unless the trajectory carries ``lattice_ts``.  ``masses`` ``(N,)`` (``None``: unit
        masses); ``modes``: an integer index array selecting rows of ``phonons`` (``ValueError`` when empty or out of
        range).  A ``phonons`` of another atom count is a ``ValueError``.  ``on_device=True``: the positions go to the
        HBM of GPU ``device`` and the returned ``DeviceModeVibrationalDensityOfStates`` reduces them there."""
        from ramannoodle_amd.spectrum import DeviceModeVibrationalDensityOfStates, ModeVibrationalDensityOfStates
        lattice, vectors = _mode_vdos_arguments(phonons, lattice, self._lattice_ts, masses, modes,
                                                self._positions_ts.shape[1])
        if not on_device:
            return ModeVibrationalDensityOfStates(self._positions_ts, self._timestep, lattice, vectors, masses)
        import torch
        positions = torch.tensor(self._positions_ts, dtype=torch.float64, device=f"cuda:{int(device)}")
        if self._lattice_ts is not None:
            lattice = torch.tensor(lattice, dtype=torch.float64, device=positions.device)
        return DeviceModeVibrationalDensityOfStates(positions, self._timestep, lattice, vectors, masses)

    def get_mode_raman_spectrum(self, polarizability_model: PolarizabilityModel, phonons, lattice=None, masses=None,
                                modes=None, rest: bool = True, on_device: bool = False):
        """Phonon-mode decomposition of the spectrum (an addition): ``ModeMDRamanSpectrum`` of the per-mode trapezoid
        increments of the polarizability (``PotGNN.calc_mode_increments``): which mode makes which peak of the MD
        spectrum, and how much of it is interference between modes.  ``phonons``, ``masses`` and ``modes`` as for
        ``get_mode_vdos``; ``lattice`` ``(3,3)`` is the cell of the phonon calculation (``None``: the model's reference
        lattice).  ``rest=True`` adds a channel for what the chosen modes leave out, so that the channels sum to the
        whole increment; a variable-cell trajectory gains the cell channel, the last.  ``on_device=True``: the
        increments stay in HBM and the returned ``DeviceModeMDRamanSpectrum`` reduces them there.  Needs a model with
        ``calc_mode_increments_device`` (the device PotGNN); there is no fallback."""
        from ramannoodle_amd.spectrum import DeviceModeMDRamanSpectrum, ModeMDRamanSpectrum
        result = _mode_increments(polarizability_model, self._positions_ts, self._lattice_ts, phonons, lattice, masses,
                                  modes, rest)
        if on_device:
            return DeviceModeMDRamanSpectrum(result, self._timestep)
        return ModeMDRamanSpectrum(result.cpu().numpy(), self._timestep)

    def get_quasiharmonic_modes(self, lattice, masses=None, temperature=None, ref_positions=None, blocks: int = 1,
                                remove_translations: bool = True, on_device: bool = False, device: int = 0):
        """Quasi-harmonic (principal-mode) analysis of the run (an addition): ``QuasiHarmonicModes`` from the
        mass-weighted covariance of the atomic displacements (``ramannoodle_amd.quasiharmonic`` states the definition).
        Its ``phonons`` is a ``Phonons`` about the mean structure with ascending wavenumbers, for ``get_mode_vdos``,
        ``get_mode_raman_spectrum``, ``measure_interference`` and ``fit_peaks``.  ``lattice`` ``(3,3)``: the fixed cell;
        ``masses`` ``(N,)`` (``None``: unit masses); ``temperature`` in K (``None``: frequencies from the steps
        alone; given: also from equipartition, and those go into ``phonons``); ``ref_positions`` ``(N,3)``: the anchor of
        the minimum-image displacements (``None``: frame 0); ``blocks``: the run is cut into that many contiguous blocks,
        whose own frequencies give ``block_wavenumbers`` and ``wavenumber_errors``; ``remove_translations``: project the
        three rigid translations out.  ``on_device=True``: the positions go to the HBM of GPU ``device`` and the
        covariance moments are summed there.  ``ValueError``, before any device work: fewer than 2 frames, ``blocks < 1``
        or more than the frames, a trajectory with ``lattice_ts`` (a fluctuating cell has no single mass-weighted
        metric), a bad ``lattice``, ``masses`` or ``ref_positions``, ``temperature <= 0``; and a covariance of rank 0.
        Not checked: every atom must stay within half a cell of the anchor (no diffusion; the module says what a
        hopping atom does to the result)."""
        from ramannoodle_amd.quasiharmonic import quasiharmonic_modes
        if self._lattice_ts is not None:
            raise ValueError("quasi-harmonic modes and a trajectory with a lattice per frame are incompatible: a "
                             "fluctuating cell has no single mass-weighted metric")
        return quasiharmonic_modes(self._positions_ts, [len(self._positions_ts)], self._timestep, lattice, masses,
                                   temperature, ref_positions, blocks, remove_translations, on_device, device)

    def get_band_modes(self, bands, lattice, masses=None, polarizability_model=None, segment_steps=None, hop=None,
                       taper="hann", remove_translations: bool = True, on_device: bool = False, device: int = 0):
        """The atomic motion, and its Raman tensor, under peaks of the run's spectra (an addition): ``BandModes`` from
        the band-limited covariance of the mass-weighted velocities (``ramannoodle_amd.bandmodes`` states the
        definition).  ``bands`` ``(B,2)``: half-open intervals ``[lo, hi)`` in 1/cm on the axis of
        ``get_vdos(...).measure()`` (``spectrum.band_weights``); ``lattice`` ``(3,3)``: the fixed cell; ``masses``
        ``(N,)`` (``None``: unit masses); ``polarizability_model``: when given, every frame is evaluated and the moments
        gain the six polarizability columns, so that every mode has its effective Raman tensor; ``segment_steps``,
        ``hop``, ``taper`` as ``spectrum.segment_plan`` (``segment_steps=None``: the whole run as one boxcar segment);
        ``remove_translations``: project the three rigid translations out.  ``on_device=True``: the positions go to
        the HBM of GPU ``device`` (with a model: of the model's GPU, where ``calc_polarizabilities_device`` evaluates
        them) and the moments are summed there.  ``ValueError``, before any device work: a trajectory with
        ``lattice_ts``, a bad ``lattice`` or ``masses``, what ``band_weights`` refuses, fewer than three frames, a
        model of another atom count."""
        from ramannoodle_amd.bandmodes import band_modes
        if self._lattice_ts is not None:
            raise ValueError("band modes and a trajectory with a lattice per frame are incompatible: a fluctuating cell "
                             "has no single mass-weighted metric")
        return band_modes(self._positions_ts, None, self._timestep, bands, lattice, masses, polarizability_model,
                          segment_steps, hop, taper, remove_translations, on_device, device)

    def __len__(self) -> int:
        return len(self._positions_ts)

    def __getitem__(self, key):
        try:
            return self._positions_ts[key]
        except IndexError as exc:
            if "out of bounds" in str(exc):
                raise IndexError("trajectory index out of bounds") from exc
            raise


class TrajectoryEnsemble:
    """Several MD trajectories of one system (an addition): independent runs whose spectra are averaged, for example
    NVE branches started from NVT snapshots.  ``trajectories``: a sequence of ``Trajectory`` sharing a timestep and an
    atom count.  All frames of all runs go through the model in one batch; the spectra never join a run to the next.
    Either every run has a lattice per frame (``Trajectory.lattice_ts``) or none has; the lattices are joined as the
    frames are."""

    def __init__(self, trajectories) -> None:
        trajectories = list(trajectories)
        if not trajectories:
            raise ValueError("an ensemble needs at least one trajectory")
        for index, trajectory in enumerate(trajectories):
            if not isinstance(trajectory, Trajectory):
                raise get_type_error(f"trajectories[{index}]", trajectory, "Trajectory")
        timesteps = sorted({trajectory.timestep for trajectory in trajectories})
        if len(timesteps) != 1:
            raise ValueError(f"trajectories must share a timestep, not {timesteps}")
        atoms = sorted({trajectory[0].shape[0] for trajectory in trajectories})
        if len(atoms) != 1:
            raise ValueError(f"trajectories must share a number of atoms, not {atoms}")
        self._trajectories = trajectories
        self._timestep = timesteps[0]
        self._run_lengths = [len(trajectory) for trajectory in trajectories]
        self._positions_ts = np.concatenate([trajectory._positions_ts for trajectory in trajectories], axis=0)
        with_cells = [trajectory._lattice_ts is not None for trajectory in trajectories]
        if any(with_cells) and not all(with_cells):
            raise ValueError("either every trajectory has a lattice per frame or none has: trajectories "
                             f"{[i for i, w in enumerate(with_cells) if not w]} have none")
        self._lattice_ts = (np.concatenate([trajectory._lattice_ts for trajectory in trajectories], axis=0)
                            if all(with_cells) else None)

    @property
    def trajectories(self):
        return list(self._trajectories)

    @property
    def run_lengths(self) -> list[int]:
        return list(self._run_lengths)

    @property
    def timestep(self) -> float:
        return self._timestep

    def _split(self, joined, rows_short: int = 0):
        """The runs of an array over the joined frames (``rows_short = 1``: over the steps between them, the step across
        each run boundary dropped)."""
        bounds = np.cumsum(self._run_lengths)
        return [joined[end - length:end - rows_short] for length, end in zip(self._run_lengths, bounds)]

    def get_raman_spectrum(self, polarizability_model: PolarizabilityModel, on_device: bool = False):
        """``MDRamanEnsemble`` of the runs' polarizability time series, all frames evaluated in one
        ``calc_polarizabilities`` call.  ``on_device=True`` (needs the device PotGNN): one
        ``calc_polarizabilities_device`` call; the joined series stays in HBM and the returned
        ``DeviceMDRamanEnsemble`` reduces it there."""
        from ramannoodle_amd.spectrum import DeviceMDRamanEnsemble, MDRamanEnsemble
        try:
            if on_device:
                import torch
                evaluate = getattr(polarizability_model, "calc_polarizabilities_device", None)
                if evaluate is None:
                    raise TypeError("on_device=True needs a model with calc_polarizabilities_device")
                verify_ndarray_shape("positions_batch", self._positions_ts,
                                     (None, polarizability_model.num_atoms, 3))
                positions = torch.tensor(self._positions_ts, dtype=torch.float64,
                                         device=f"cuda:{polarizability_model.device_index}")
                return DeviceMDRamanEnsemble(evaluate(positions, **_cells(self._lattice_ts, positions.device)),
                                             self._timestep, self._run_lengths)
            polarizability_ts = polarizability_model.calc_polarizabilities(self._positions_ts, **_cells(self._lattice_ts))
        except ValueError as exc:
            raise ValueError("polarizability_model and trajectory are incompatible") from exc
        return MDRamanEnsemble(self._split(polarizability_ts), self._timestep)

    def get_descriptors(self, model, on_device: bool = False):
        """Structure descriptors of the frames of every run, joined in the order of the runs (``Trajectory.get_descriptors``):
        one evaluation."""
        return _descriptors(model, self._positions_ts, self._lattice_ts, on_device)

    def get_partial_raman_spectrum(self, polarizability_model: PolarizabilityModel, groups, on_device: bool = False):
        """``PartialMDRamanEnsemble`` of the runs' per-group increments (``groups`` as for ``Trajectory``), from one
        ``calc_group_increments_device`` call over the joined frames: the increments across the run boundaries are
        computed and never read.  ``on_device=True``: they stay in HBM (``DevicePartialMDRamanEnsemble``).  Needs a model
        with ``calc_group_increments_device`` (the device PotGNN); there is no fallback."""
        import torch
        from ramannoodle_amd.spectrum import DevicePartialMDRamanEnsemble, PartialMDRamanEnsemble
        increments = getattr(polarizability_model, "calc_group_increments_device", None)
        if increments is None:
            raise TypeError(f"{type(polarizability_model).__name__} has no calc_group_increments_device: partial spectra "
                            "need the Jacobian of the model (the device PotGNN)")
        if min(self._run_lengths) < 2:
            raise ValueError("every trajectory needs at least two frames for its increments")
        try:
            verify_ndarray_shape("positions_ts", self._positions_ts, (None, polarizability_model.num_atoms, 3))
            positions = torch.tensor(self._positions_ts, dtype=torch.float64,
                                     device=f"cuda:{polarizability_model.device_index}")
            result = increments(positions, groups, **_cells(self._lattice_ts, positions.device))
        except ValueError as exc:
            raise ValueError(f"polarizability_model and trajectory are incompatible: {exc}") from exc
        if on_device:
            return DevicePartialMDRamanEnsemble(result, self._timestep, self._run_lengths)
        return PartialMDRamanEnsemble(self._split(result.cpu().numpy(), 1), self._timestep)

    def get_vdos(self, lattice=None, masses=None, groups=None, atomic_numbers=None, on_device: bool = False,
                 device: int = 0):
        """``VibrationalDensityOfStatesEnsemble`` of the runs (arguments as ``Trajectory.get_vdos``): the VDOS averaged
        over the runs, whose segments never read the step from one run to the next.  ``on_device=True``: the joined
        positions go to the HBM of GPU ``device`` (``DeviceVibrationalDensityOfStatesEnsemble``)."""
        from ramannoodle_amd.spectrum import (DeviceVibrationalDensityOfStatesEnsemble,
                                              VibrationalDensityOfStatesEnsemble)
        lattice, masses, labels, count = _vdos_arguments(lattice, self._lattice_ts, masses, groups, atomic_numbers,
                                                         self._positions_ts.shape[1])
        if not on_device:
            per_run = lattice if self._lattice_ts is None else self._split(lattice)
            return VibrationalDensityOfStatesEnsemble(self._split(self._positions_ts), self._timestep, per_run, masses,
                                                      labels, count)
        import torch
        positions = torch.tensor(self._positions_ts, dtype=torch.float64, device=f"cuda:{int(device)}")
        if self._lattice_ts is not None:
            lattice = torch.tensor(lattice, dtype=torch.float64, device=positions.device)
        return DeviceVibrationalDensityOfStatesEnsemble(positions, self._timestep, lattice, masses, labels, count,
                                                        run_lengths=self._run_lengths)

    def get_mode_vdos(self, phonons, lattice, masses=None, modes=None, on_device: bool = False, device: int = 0):
        """``ModeVibrationalDensityOfStatesEnsemble`` of the runs (arguments as ``Trajectory.get_mode_vdos``): the
        mode-projected VDOS averaged over the runs, whose segments never read the step from one run to the next.
        ``on_device=True``: the joined positions go to the HBM of GPU ``device``
        (``DeviceModeVibrationalDensityOfStatesEnsemble``)."""
        from ramannoodle_amd.spectrum import (DeviceModeVibrationalDensityOfStatesEnsemble,
                                              ModeVibrationalDensityOfStatesEnsemble)
        lattice, vectors = _mode_vdos_arguments(phonons, lattice, self._lattice_ts, masses, modes,
                                                self._positions_ts.shape[1])
        if not on_device:
            per_run = lattice if self._lattice_ts is None else self._split(lattice)
            return ModeVibrationalDensityOfStatesEnsemble(self._split(self._positions_ts), self._timestep, per_run,
                                                          vectors, masses)
        import torch
        positions = torch.tensor(self._positions_ts, dtype=torch.float64, device=f"cuda:{int(device)}")
        if self._lattice_ts is not None:
            lattice = torch.tensor(lattice, dtype=torch.float64, device=positions.device)
        return DeviceModeVibrationalDensityOfStatesEnsemble(positions, self._timestep, lattice, vectors, masses,
                                                            run_lengths=self._run_lengths)

    def get_mode_raman_spectrum(self, polarizability_model: PolarizabilityModel, phonons, lattice=None, masses=None,
                                modes=None, rest: bool = True, on_device: bool = False):
        """``ModeMDRamanEnsemble`` of the runs' per-mode increments (arguments as
        ``Trajectory.get_mode_raman_spectrum``), from one ``calc_mode_increments_device`` call over the joined frames:
        the increments across the run boundaries are computed and never read.  ``on_device=True``: they stay in HBM
        (``DeviceModeMDRamanEnsemble``).  Needs a model with ``calc_mode_increments_device`` (the device PotGNN); there
        is no fallback."""
        from ramannoodle_amd.spectrum import DeviceModeMDRamanEnsemble, ModeMDRamanEnsemble
        if min(self._run_lengths) < 2:
            raise ValueError("every trajectory needs at least two frames for its increments")
        result = _mode_increments(polarizability_model, self._positions_ts, self._lattice_ts, phonons, lattice, masses,
                                  modes, rest)
        if on_device:
            return DeviceModeMDRamanEnsemble(result, self._timestep, self._run_lengths)
        return ModeMDRamanEnsemble(self._split(result.cpu().numpy(), 1), self._timestep)

    def get_quasiharmonic_modes(self, lattice, masses=None, temperature=None, ref_positions=None, blocks: int = 1,
                                remove_translations: bool = True, on_device: bool = False, device: int = 0):
        """``QuasiHarmonicModes`` of the joined runs (arguments as ``Trajectory.get_quasiharmonic_modes``): every run is
        cut into ``blocks`` blocks and no step crosses a run boundary; the anchor is frame 0 of the first run unless
        ``ref_positions`` is given.  ``on_device=True``: the joined positions go to the HBM of GPU ``device``."""
        from ramannoodle_amd.quasiharmonic import quasiharmonic_modes
        if self._lattice_ts is not None:
            raise ValueError("quasi-harmonic modes and trajectories with a lattice per frame are incompatible: a "
                             "fluctuating cell has no single mass-weighted metric")
        return quasiharmonic_modes(self._positions_ts, self._run_lengths, self._timestep, lattice, masses, temperature,
                                   ref_positions, blocks, remove_translations, on_device, device)

    def get_band_modes(self, bands, lattice, masses=None, polarizability_model=None, segment_steps=None, hop=None,
                       taper="hann", remove_translations: bool = True, on_device: bool = False, device: int = 0):
        """``BandModes`` of the joined runs (arguments as ``Trajectory.get_band_modes``): the moments are the mean over
        the segments of every run, none of which crosses a run boundary (``spectrum.ensemble_segment_starts``);
        ``segment_steps=None`` takes each run whole and needs runs of one length, as the ensemble VDOS does.  With a
        model, all frames are evaluated in one call."""
        from ramannoodle_amd.bandmodes import band_modes
        if self._lattice_ts is not None:
            raise ValueError("band modes and trajectories with a lattice per frame are incompatible: a fluctuating cell "
                             "has no single mass-weighted metric")
        return band_modes(self._positions_ts, self._run_lengths, self._timestep, bands, lattice, masses,
                          polarizability_model, segment_steps, hop, taper, remove_translations, on_device, device)
