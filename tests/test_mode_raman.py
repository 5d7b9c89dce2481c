"""Phonon-mode projection of MD Raman spectra: what needs no GPU.

``spectrum.mode_projectors`` (the completeness identity and its errors), the host reducer ``_md_modes_host`` against the
host atom-group path, ``ModeMDRamanSpectrum.select``, the ctypes signatures of the new entries, and the argument errors
of the classes and of ``Trajectory.get_mode_raman_spectrum``."""
import ctypes as C

import numpy as np
import pytest

from ramannoodle_amd import _lib
from ramannoodle_amd.dynamics import Phonons, Trajectory
from ramannoodle_amd.spectrum import (MAX_SELECTED, DeviceModeMDRamanSpectrum, ModeMDRamanSpectrum,
                                      PartialMDRamanSpectrum, mode_projectors, mode_vectors)

LATTICE = np.array([[4.1, 0.3, -0.2], [0.5, 5.2, 0.4], [-0.3, 0.6, 6.3]])


def _basis(atoms, seed=0):
    """Fractional displacements of a complete orthonormal mass-weighted basis, and the masses."""
    rng = np.random.default_rng(seed)
    e = np.linalg.qr(rng.normal(size=(3 * atoms, 3 * atoms)))[0].T.reshape(3 * atoms, atoms, 3)
    masses = rng.uniform(1.0, 60.0, size=atoms)
    return (e / np.sqrt(masses)[None, :, None]) @ np.linalg.inv(LATTICE), masses


def _increments(steps, channels, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(steps)[:, None, None, None]
    freq = 1 + np.arange(channels * 9).reshape(1, channels, 3, 3) % 23
    incr = 0.05 * rng.normal(size=(steps, channels, 3, 3)) + np.cos(0.07 * t * freq)
    return incr * np.logspace(-1, 1, channels)[None, :, None, None]


def _row_errors(got, want):
    scale = np.abs(want).max(axis=-1)
    assert np.all(scale > 0)
    return np.abs(got - want).max(axis=-1) / scale


def test_projectors_are_complete():
    atoms = 7
    fractional, masses = _basis(atoms)
    disp, proj = mode_projectors(fractional, LATTICE, masses)
    assert disp.shape == proj.shape == (3 * atoms, atoms, 3) and disp.dtype == proj.dtype == np.float64
    identity = np.einsum("mia,mjb->iajb", disp, proj).reshape(3 * atoms, 3 * atoms)
    assert np.abs(identity - np.eye(3 * atoms)).max() <= 1e-12
    # D is the displacement of a unit amplitude, P reads the amplitude back
    vectors = mode_vectors(fractional, LATTICE, masses)
    np.testing.assert_allclose(disp @ LATTICE * np.sqrt(masses)[None, :, None], vectors, atol=1e-13)
    np.testing.assert_allclose(np.einsum("mir,kir->mk", proj, disp), np.eye(3 * atoms), atol=1e-12)
    # a scaled displacement is normalised away, as in mode_vectors
    again = mode_projectors(3.0 * fractional, LATTICE, masses)
    np.testing.assert_allclose(again[0], disp, atol=1e-14)


def test_projectors_refuse_what_mode_vectors_refuses():
    fractional, masses = _basis(4)
    nan = fractional.copy()
    nan[2, 1, 0] = np.nan
    zero = fractional.copy()
    zero[1] = 0.0
    for arguments in ((fractional[0], LATTICE, masses), (fractional[:, :, :2], LATTICE, masses),
                      (fractional, LATTICE[:2], masses), (fractional, np.zeros((3, 3)), masses),
                      (fractional, LATTICE, masses[:3]), (fractional, LATTICE, -masses), (nan, LATTICE, masses),
                      (zero, LATTICE, masses)):
        with pytest.raises(ValueError):
            mode_projectors(*arguments)
        with pytest.raises(ValueError):
            mode_vectors(*arguments)


@pytest.mark.parametrize("channels", [1, 3, 16])
def test_host_reducer_matches_the_host_partial_path(channels):
    incr = _increments(150, channels, seed=channels)
    modes, pairs = ModeMDRamanSpectrum(incr, 1.5), PartialMDRamanSpectrum(incr, 1.5)
    index = np.arange(channels)

    def compare(got, want):  # got [..., C+1, bins], want [..., G, G, bins]
        assert got.shape == want.shape[:-3] + (channels + 1, want.shape[-1])
        assert _row_errors(got[..., :channels, :], want[..., index, index, :]).max() <= 1e-10
        assert _row_errors(got[..., channels, :], want.sum(axis=(-3, -2))).max() <= 1e-10

    (w_modes, got), (w_pairs, want) = modes.measure(), pairs.measure()
    np.testing.assert_array_equal(w_modes, w_pairs)
    compare(got, want)
    compare(modes.measure(laser_correction=True, bose_einstein_correction=True)[1],
            pairs.measure(laser_correction=True, bose_einstein_correction=True)[1])
    rng = np.random.default_rng(1)
    e_i, e_s = rng.normal(size=(3, 3)), rng.normal(size=(3, 3))
    compare(modes.measure_polarized(e_i, e_s)[1], pairs.measure_polarized(e_i, e_s)[1])
    assert modes.measure_polarized(e_i[0], e_s[0])[1].shape == (channels + 1, len(w_modes))
    for average in (True, False):
        keywords = dict(segment_steps=41, hop=25, taper="hann", average=average)
        compare(modes.measure_segments(**keywords)[1], pairs.measure_segments(**keywords)[1])
        compare(modes.measure_segments_polarized(e_i, e_s, **keywords)[1],
                pairs.measure_segments_polarized(e_i, e_s, **keywords)[1])
    np.testing.assert_array_equal(modes.segment_starts(41, 25), pairs.segment_starts(41, 25))


def test_interference_is_the_off_diagonal_sum():
    incr = _increments(150, 5, seed=9)
    _, got = ModeMDRamanSpectrum(incr, 1.0).measure()
    _, pairs = PartialMDRamanSpectrum(incr, 1.0).measure()
    off_diagonal = pairs.sum(axis=(0, 1)) - np.trace(pairs)
    interference = got[-1] - got[:-1].sum(axis=0)
    assert np.abs(interference - off_diagonal).max() <= 1e-10 * np.abs(got[-1]).max()


def test_select_layout_and_sums():
    incr = _increments(90, 40, seed=4)
    spectrum = ModeMDRamanSpectrum(incr, 2.0)
    assert spectrum.num_channels == 40
    chosen = spectrum.select([7, 2, 39])
    assert isinstance(chosen, PartialMDRamanSpectrum) and chosen.timestep == 2.0
    assert chosen.increments.shape == (90, 4, 3, 3)
    np.testing.assert_array_equal(chosen.increments[:, :3], incr[:, [7, 2, 39]])
    others = np.delete(incr, [7, 2, 39], axis=1).sum(axis=1)
    np.testing.assert_allclose(chosen.increments[:, 3], others, rtol=0, atol=1e-13 * np.abs(others).max())
    np.testing.assert_allclose(chosen.increments.sum(axis=1), incr.sum(axis=1), rtol=0,
                               atol=1e-13 * np.abs(incr.sum(axis=1)).max())
    _, pairs = chosen.measure()
    _, modes = spectrum.measure()
    assert _row_errors(pairs[[0, 1, 2], [0, 1, 2]], modes[[7, 2, 39]]).max() <= 1e-10
    assert _row_errors(pairs.sum(axis=(0, 1))[None], modes[-1:]).max() <= 1e-10
    assert spectrum.select(np.arange(MAX_SELECTED)).increments.shape[1] == MAX_SELECTED + 1
    everything = ModeMDRamanSpectrum(incr[:, :3], 2.0).select([0, 1, 2])
    assert np.all(everything.increments[:, 3] == 0.0)
    for bad in ([], np.arange(MAX_SELECTED + 1), [40], [-1], [1, 1], [0.5], [[1, 2]]):
        with pytest.raises(ValueError):
            spectrum.select(bad)


def test_signatures_list_the_new_entries():
    table = _lib.SIGNATURES
    for name in ("rn_potgnn_mode_contract_device", "rn_potgnn_mode_increments_device", "rn_md_raman_modes",
                 "rn_md_raman_modes_device", "rn_md_raman_modes_set_profiling", "rn_md_raman_modes_phase_times"):
        assert name in table, name
    host, device = table["rn_md_raman_modes"], table["rn_md_raman_modes_device"]
    assert device[0] == host[0] and device[1] == host[1] + [C.c_void_p]
    # ... and differ from the atom-group segment reducer in nothing: C takes the place of G
    assert host == table["rn_md_raman_partial_segments"]
    assert device == table["rn_md_raman_partial_segments_device"]
    assert table["rn_potgnn_mode_contract_device"][1][-1] == C.c_void_p
    assert table["rn_potgnn_mode_increments_device"][1][-1] == C.c_void_p


def test_classes_refuse_bad_arguments():
    incr = _increments(30, 3, seed=1)
    with pytest.raises(ValueError):
        ModeMDRamanSpectrum(incr[..., :2], 1.0)
    with pytest.raises(ValueError):
        ModeMDRamanSpectrum(incr[:, :0], 1.0)
    with pytest.raises((ValueError, AttributeError)):
        DeviceModeMDRamanSpectrum(incr, 1.0)  # not a CUDA tensor
    spectrum = ModeMDRamanSpectrum(incr, 1.0)
    with pytest.raises(NotImplementedError):
        spectrum.measure(orientation=np.eye(3))
    with pytest.raises(ValueError):
        spectrum.measure_segments(31 + 1)
    with pytest.raises(ValueError):
        spectrum.measure_segments(8, taper="kaiser")
    with pytest.raises(ValueError):
        ModeMDRamanSpectrum(incr[:1], 1.0).measure()


class _NoJacobian:
    num_atoms = 4
    device_index = 0


class _Recorder(_NoJacobian):
    """Stands in for the device model: records the call and refuses it as the model refuses other atom counts."""
    ref_lattice = LATTICE

    def __init__(self):
        self.calls = []

    def calc_mode_increments_device(self, positions, displacements, projectors, rest=True, **keywords):
        self.calls.append((displacements, projectors, rest, keywords))
        raise ValueError("stop here")


def test_trajectory_front_end_without_a_gpu():
    fractional, masses = _basis(4)
    phonons = Phonons(np.zeros((4, 3)), np.arange(12.0), fractional)
    traj = Trajectory(np.random.default_rng(0).uniform(size=(6, 4, 3)), 1.0)
    with pytest.raises(TypeError):
        traj.get_mode_raman_spectrum(_NoJacobian(), phonons, LATTICE)
    model = _Recorder()
    with pytest.raises(TypeError):
        traj.get_mode_raman_spectrum(model, fractional, LATTICE)
    for modes in ([], [12], [-1], [0.5], [[0, 1]]):
        with pytest.raises(ValueError):
            traj.get_mode_raman_spectrum(model, phonons, LATTICE, modes=np.array(modes))
    with pytest.raises(ValueError):
        traj.get_mode_raman_spectrum(model, phonons, np.zeros((3, 3)))
    with pytest.raises(ValueError):
        traj.get_mode_raman_spectrum(model, phonons, LATTICE, masses=masses[:3])
    with pytest.raises(ValueError):
        Trajectory(np.zeros((6, 5, 3)), 1.0).get_mode_raman_spectrum(model, phonons, LATTICE)
    assert not model.calls
