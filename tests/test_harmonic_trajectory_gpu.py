"""Harmonic trajectories on the GPU (``include/rn_harmonic.h``) against the host statement ``synthesize_host``, their
determinism, ``get_harmonic_trajectory(on_device=True)`` end to end, the round trip of the tensor through the device
consumers and a run evaluated with a model.

Tolerance (``tests.harmonic_cases.difference_bound``; derived, not measured).  Device and host are compared after the
minimum image ``d - rint(d)``, because a value at a face may wrap to either side.  Per column ``2 (M + 8) 2^-52 s_j +
2^-50`` with ``s_j = max_r sum_m |amp[r][m] D[m][j]|``: on each side each of the M terms carries a cosine of at most 2
ulp on an identical argument plus two products, the M terms are summed in any order, then come one addition to a value of
order one and the wrap.  ``s_j <= 0.05`` in every case."""
import functools

import numpy as np
import pytest
import torch

from ramannoodle_amd import harmonic
from ramannoodle_amd.dynamics import Phonons, TrajectoryEnsemble
from ramannoodle_amd.quasiharmonic import modes_from_moments, moments_device
from ramannoodle_amd.spectrum import (_PER_FS_TO_CM1, DeviceMDRamanSpectrum, DeviceModeVibrationalDensityOfStates,
                                      mode_vectors)
from tests.conftest import load_golden
from tests.harmonic_cases import (DEVICE_CASES, MAX_REACH, device_case, difference_bound, minimum_image, mode_basis,
                                  planted_phonons, reach)
from tests.helpers import product_model_from_golden
from tests.quasiharmonic_cases import LATTICE, PLANTED_FRAMES, PLANTED_TIMESTEP
from tests.test_harmonic_trajectory import planted_checks

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(name):
    """``(inputs, frames, first frame, synthesize_host(...))``, computed once"""
    inputs, frames, first = device_case(name)
    want = harmonic.synthesize_host(*inputs, frames, first)
    for array in (*inputs, want):
        array.setflags(write=False)
    return inputs, frames, first, want


def _worst(got, want, amp, D):
    """The largest device-minus-host difference over its bound, and the check itself."""
    shape = want.shape
    difference = np.abs(minimum_image(np.asarray(got).reshape(shape) - want)).reshape(shape[0], shape[1], -1)
    bound = difference_bound(amp, D)
    assert np.all(np.isfinite(difference))
    return (difference.max(axis=(0, 1)) / bound).max(), difference.max(), bound.max()


@pytest.mark.parametrize("name", list(DEVICE_CASES))
def test_device_agrees_with_the_host_statement(name):
    (ref, D, omega_dt, amp, phase), frames, first, want = _case(name)
    assert reach(amp, D).max() <= MAX_REACH * (1 + 1e-12)
    tensor = harmonic.synthesize_device(ref, D, omega_dt, amp, phase, frames, first)
    assert tensor.is_cuda and tensor.is_contiguous() and tensor.dtype == torch.float64
    assert tuple(tensor.shape) == want.shape == (len(amp), frames, len(ref), 3)
    got = tensor.cpu().numpy()
    ratio, difference, bound = _worst(got, want, amp, D)
    print(f"{name}: worst difference {difference:.3e}, bound {bound:.3e}, worst ratio {ratio:.3f}")
    assert ratio <= 1.0
    assert np.all((got >= 0) & (got <= 1))
    # determinism: both entries agree bit for bit, a repeated call is bit-identical, also into a tensor of the caller's
    np.testing.assert_array_equal(harmonic.synthesize_download(ref, D, omega_dt, amp, phase, frames, first), got)
    out = torch.full(want.shape, -1.0, dtype=torch.float64, device="cuda")
    assert harmonic.synthesize_device(ref, D, omega_dt, amp, phase, frames, first, out=out) is out
    np.testing.assert_array_equal(out.cpu().numpy(), got)


@pytest.mark.parametrize("name, cut", [("66 columns, 17 modes, 257 frames", 37),
                                       ("129 columns, one mode, 257 frames, three runs", 203),
                                       ("five modes, 17 frames, three runs, far out", 3)])
def test_a_run_in_two_calls_is_the_run_in_one(name, cut):
    """A frame's value depends on its absolute index only: frames [0, T) equal [0, a) and [a, T) with t0 = a, bit for
    bit, for an ``a`` that is not a multiple of 16 (the frames of a wave) nor of 64 (of a workgroup)."""
    (ref, D, omega_dt, amp, phase), frames, first, _ = _case(name)
    assert cut % 16 and 0 < cut < frames
    whole = harmonic.synthesize_device(ref, D, omega_dt, amp, phase, frames, first).cpu().numpy()
    head = harmonic.synthesize_device(ref, D, omega_dt, amp, phase, cut, first).cpu().numpy()
    tail = harmonic.synthesize_device(ref, D, omega_dt, amp, phase, frames - cut, first + cut).cpu().numpy()
    np.testing.assert_array_equal(head, whole[:, :cut])
    np.testing.assert_array_equal(tail, whole[:, cut:])


def test_the_public_methods_on_the_device():
    phonons, masses, _, wavenumbers = planted_phonons()
    arguments = dict(masses=masses, statistics="classical", sampling="random", seed=3)
    want = phonons.get_harmonic_trajectory(LATTICE, 20.0, 100, 2.0, **arguments)
    got = phonons.get_harmonic_trajectory(LATTICE, 20.0, 100, 2.0, on_device=True, **arguments)
    assert len(got) == 100 and got.timestep == 2.0
    _, D, _, selected, _ = harmonic.phonon_arguments(phonons, LATTICE, 2.0, masses)
    amp, _ = harmonic.draw(selected, 20.0, "classical", "random", 3, seed=3)
    assert reach(amp, D).max() <= MAX_REACH
    ratio, difference, bound = _worst(got.positions_ts[None], want.positions_ts[None], amp[:1], D)
    print(f"trajectory: worst difference {difference:.3e}, bound {bound:.3e}, worst ratio {ratio:.3f}")
    assert ratio <= 1.0
    ensemble = phonons.get_harmonic_ensemble(LATTICE, 20.0, 100, 2.0, runs=3, on_device=True, **arguments)
    assert isinstance(ensemble, TrajectoryEnsemble) and ensemble.run_lengths == [100, 100, 100]
    runs = [trajectory.positions_ts for trajectory in ensemble.trajectories]
    np.testing.assert_array_equal(runs[0], got.positions_ts)
    assert not np.array_equal(runs[0], runs[1]) and not np.array_equal(runs[1], runs[2])
    host = phonons.get_harmonic_ensemble(LATTICE, 20.0, 100, 2.0, runs=3, **arguments)
    ratio, difference, bound = _worst(np.stack(runs), np.stack([t.positions_ts for t in host.trajectories]), amp, D)
    print(f"ensemble: worst difference {difference:.3e}, bound {bound:.3e}, worst ratio {ratio:.3f}")
    assert ratio <= 1.0


def test_planted_round_trip_in_hbm():
    """The tensor goes to the covariance moments and to the mode VDOS where it is: the four bounds of the host test."""
    phonons, masses, vectors, wavenumbers = planted_phonons()
    ref, D, omega_dt, selected, _ = harmonic.phonon_arguments(phonons, LATTICE, PLANTED_TIMESTEP, masses)
    amp, phase = harmonic.draw(selected, 300.0, "classical", "mean", 1, seed=0)
    tensor = harmonic.synthesize_device(ref, D, omega_dt, amp, phase, PLANTED_FRAMES)
    run = tensor[0]
    assert run.is_contiguous() and run.data_ptr() == tensor.data_ptr()
    first, second, counts = moments_device(run, ref, [0, PLANTED_FRAMES], [0])
    modes = modes_from_moments(first, second, counts, LATTICE, masses, PLANTED_TIMESTEP, temperature=300.0, anchor=ref)
    axis, rows = DeviceModeVibrationalDensityOfStates(run, PLANTED_TIMESTEP, LATTICE,
                                                      mode_vectors(phonons.displacements, LATTICE, masses), masses).measure()
    planted_checks(modes, axis, rows, vectors, wavenumbers, "HBM")


def test_a_single_mode_evaluated_with_a_model():
    """The polarizabilities of the synthesised tensor are those of its host copy bit for bit, and the strongest bin of
    the spectrum above half the mode's wavenumber lies within one bin of the mode."""
    g = load_golden("triclinic20")
    model = product_model_from_golden(g).eval()
    lattice = np.asarray(g["lattice"], dtype=np.float64).reshape(3, 3)
    sites = np.asarray(g["positions"], dtype=np.float64)
    atoms, frames, timestep = len(sites), 1024, 1.0
    rng = np.random.default_rng(8)
    masses = rng.uniform(1.0, 4.0, atoms)
    columns = 3 * atoms
    translations = np.sqrt(masses / masses.sum())[None, :, None] * np.eye(3)[:, None, :]
    vectors = np.concatenate([translations, mode_basis(masses, columns - 3, rng)])
    np.testing.assert_allclose(vectors.reshape(columns, columns) @ vectors.reshape(columns, columns).T, np.eye(columns),
                               atol=1e-12)  # a complete orthonormal basis
    cycles = np.concatenate([[0, 0, 0], 30 + 5 * np.arange(columns - 3)])  # commensurate with the 1024 frames
    wavenumbers = cycles / (frames * timestep) * _PER_FS_TO_CM1
    displacements = np.ascontiguousarray((vectors / np.sqrt(masses)[None, :, None]) @ np.linalg.inv(lattice))
    phonons = Phonons(sites, wavenumbers, displacements)
    tensors = phonons.get_raman_spectrum(model).raman_tensors
    mode = int(np.argmax((tensors[3:] ** 2).sum(axis=(1, 2)))) + 3
    ref, D, omega_dt, selected, index = harmonic.phonon_arguments(phonons, lattice, timestep, masses, modes=[mode])
    assert index.tolist() == [mode]
    amp, phase = harmonic.draw(selected, 10.0, "classical", "mean", 1, seed=0)
    tensor = harmonic.synthesize_device(ref, D, omega_dt, amp, phase, frames, device=model.device_index)[0]
    copy = torch.tensor(tensor.cpu().numpy(), dtype=torch.float64, device=tensor.device)
    alpha = model.calc_polarizabilities_device(tensor)
    assert torch.equal(alpha, model.calc_polarizabilities_device(copy))
    axis, intensities = DeviceMDRamanSpectrum(alpha, timestep).measure()
    window = axis > 0.5 * wavenumbers[mode]
    strongest = axis[window][np.argmax(intensities[window])]
    print(f"mode {mode} at {wavenumbers[mode]:.2f} 1/cm: strongest bin at {strongest:.2f} 1/cm, bins of {axis[1] - axis[0]:.2f}")
    assert abs(strongest - wavenumbers[mode]) <= axis[1] - axis[0]
