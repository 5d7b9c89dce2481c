"""Quasi-harmonic modes of MD runs (``ramannoodle_amd.quasiharmonic``): what needs no GPU.

``moments_host`` against the definition frame by frame, planted modes recovered from a synthetic harmonic run, the
temperature estimate, the chain into ``get_mode_vdos``, blocks and ensembles, every ``ValueError``, the C entry's
refusals (they come before the device is touched) and the new symbols."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ramannoodle_amd import _lib
from ramannoodle_amd.constants import BOLTZMANN_CONSTANT
from ramannoodle_amd.dynamics import Phonons, Trajectory, TrajectoryEnsemble
from ramannoodle_amd.quasiharmonic import (AMU_A2_PER_FS2_IN_EV, QuasiHarmonicModes, modes_from_moments, moments_host,
                                           pool_moments, run_blocks)
from ramannoodle_amd.spectrum import _PER_FS_TO_CM1, mode_vectors
from tests.quasiharmonic_cases import (LATTICE, PLANTED_FRAMES, PLANTED_MODES, PLANTED_TIMESTEP, brute_force_moments,
                                       face_frames, planted_run)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rn_qh_moments", "rn_qh_moments_device", "rn_qh_chunk_frames", "rn_qh_set_profiling", "rn_qh_phase_times",
           "rn_qh_last_error")
EPSILON = np.finfo(np.float64).eps


@pytest.mark.parametrize("atoms, frames, bounds, joined", [
    (3, 9, [0, 9], [0]),
    (4, 12, [0, 5, 6, 12], [1, 0, 0]),   # a one-frame block without a step: a zero step moment
    (4, 12, [0, 1, 7, 12], [1, 1, 0]),   # a one-frame block whose only step leaves it
])
def test_moments_host_is_the_definition_frame_by_frame(atoms, frames, bounds, joined):
    """Both sides sum at most 12 terms of one sign pattern in another order: each is within (T - 1) eps sum |terms| of
    the exact sum, and sum_t |w_j w_l| <= the largest diagonal entry, |sum_t w| <= T max |w| <= T / 2."""
    positions = face_frames(atoms, frames, seed=atoms)
    anchor = positions[2]
    assert np.abs(positions - anchor).max() > 0.9  # wrapped values on both sides of a face: the minimum image acts
    got = moments_host(positions, anchor, bounds, joined)
    want = brute_force_moments(positions, anchor, bounds, joined)
    np.testing.assert_array_equal(got[2], want[2])
    np.testing.assert_array_equal(got[2], [[hi - lo, hi - lo - 1 + j] for lo, hi, j in zip(bounds, bounds[1:], joined)])
    bound = 2 * (frames - 1) * EPSILON
    assert np.abs(got[0] - want[0]).max() <= bound * frames / 2
    for b in range(len(joined)):
        for s in range(2):
            assert np.abs(got[1][b, s] - want[1][b, s]).max() <= bound * np.abs(want[1][b, s]).max()
            np.testing.assert_array_equal(got[1][b, s], got[1][b, s].T)
    # every displacement is the small one, not the wrapped one
    assert np.sqrt(np.diagonal(got[1][:, 0], axis1=1, axis2=2).sum(axis=0) / frames).max() < 0.03
    if bounds == [0, 5, 6, 12]:
        assert not got[1][1, 1].any() and got[1][1, 0].any()
    # the pooled sums: the ascending sum of the block sums, bit for bit
    pooled = pool_moments(*got)
    first, second, counts = got[0][0].copy(), got[1][0].copy(), got[2][0].copy()
    for b in range(1, len(joined)):
        first, second, counts = first + got[0][b], second + got[1][b], counts + got[2][b]
    for mine, theirs in zip(pooled, (first, second, counts)):
        np.testing.assert_array_equal(mine, theirs)


def _overlaps(vectors, planted):
    return np.abs(np.einsum("mk,mk->m", vectors.reshape(len(vectors), -1), planted.reshape(len(planted), -1)))


def test_planted_modes_are_recovered():
    """The steps estimate uses T frames for the variance and the T - 1 steps for the step variance: the missing step's
    square lies between 0 and twice the mean one, so sigma is off by at most 1 / (T - 1) relative and the frequency by
    half of that times tan(w dt / 2) / (w dt / 2) <= 1.011 here: 2.5e-4.  Measured on the host statement: 2.46e-4
    (the overlaps: 1 - 9e-16).  With the margin of 5 that is 1.2e-3, above the 1e-3 this test may not exceed: 1e-3."""
    positions, masses, planted, wavenumbers = planted_run()
    modes = Trajectory(positions, PLANTED_TIMESTEP).get_quasiharmonic_modes(LATTICE, masses)
    assert isinstance(modes, QuasiHarmonicModes) and isinstance(modes.phonons, Phonons)
    assert modes.rank == PLANTED_MODES == len(modes.variances)
    overlaps = _overlaps(modes.vectors, planted)
    deviation = np.abs(modes.wavenumbers_steps / wavenumbers - 1.0).max()
    print(f"planted modes: 1 - min overlap {1.0 - overlaps.min():.2e}, wavenumbers off by {deviation:.3e} relative")
    assert overlaps.min() >= 1.0 - 1e-9
    assert deviation <= 1e-3
    assert modes.wavenumbers_temperature is None and np.isnan(modes.wavenumber_errors).all()
    np.testing.assert_array_equal(modes.phonons.wavenumbers, modes.wavenumbers_steps)
    assert np.all(np.diff(modes.phonons.wavenumbers) > 0)
    amplitudes = 0.3 * 40 / (40 + 7 * np.arange(PLANTED_MODES))
    np.testing.assert_allclose(modes.variances, amplitudes ** 2 / 2, rtol=1e-9)  # commensurate: the mean of cos^2 is 1/2
    # the mean structure: frame-0 anchor plus the mean displacement, within the amplitude of the origin
    assert modes.mean_positions.shape == (5, 3) and np.all((modes.mean_positions >= 0) & (modes.mean_positions < 1))
    assert modes.block_wavenumbers.shape == (1, PLANTED_MODES)
    np.testing.assert_allclose(modes.block_wavenumbers[0], modes.wavenumbers_steps, rtol=1e-9)
    np.testing.assert_array_equal(modes.counts, [PLANTED_FRAMES, PLANTED_FRAMES - 1])


def test_temperature_estimate_is_equipartition_of_the_returned_variances():
    positions, masses, planted, _ = planted_run()
    modes = Trajectory(positions, PLANTED_TIMESTEP).get_quasiharmonic_modes(LATTICE, masses, temperature=300.0)
    angular = np.sqrt(BOLTZMANN_CONSTANT * 300.0 / (AMU_A2_PER_FS2_IN_EV * modes.variances))
    np.testing.assert_allclose(modes.wavenumbers_temperature, angular * _PER_FS_TO_CM1 / (2 * np.pi), rtol=1e-14)
    np.testing.assert_array_equal(modes.phonons.wavenumbers, modes.wavenumbers_temperature)
    assert np.all(np.diff(modes.phonons.wavenumbers) > 0)
    assert abs(AMU_A2_PER_FS2_IN_EV - 103.642696) < 1e-6
    assert _overlaps(modes.vectors, planted).min() >= 1.0 - 1e-9  # the same order here: the variances descend


def test_phonons_chain_into_the_mode_vdos():
    positions, masses, _, wavenumbers = planted_run()
    trajectory = Trajectory(positions, PLANTED_TIMESTEP)
    modes = trajectory.get_quasiharmonic_modes(LATTICE, masses)
    np.testing.assert_allclose(mode_vectors(modes.phonons.displacements, LATTICE, masses), modes.vectors, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(modes.phonons.ref_positions, modes.mean_positions)
    axis, rows = trajectory.get_mode_vdos(modes.phonons, LATTICE, masses).measure()
    assert rows.shape == (PLANTED_MODES, len(axis))
    # every mode's row peaks at its own frequency, within a bin
    np.testing.assert_allclose(axis[rows.argmax(axis=1)], wavenumbers, rtol=0, atol=1.01 * (axis[1] - axis[0]))


def test_blocks_and_ensembles():
    positions, masses, _, _ = planted_run()
    trajectory = Trajectory(positions, PLANTED_TIMESTEP)
    modes = trajectory.get_quasiharmonic_modes(LATTICE, masses, blocks=4)
    assert modes.block_wavenumbers.shape == (4, PLANTED_MODES) and np.isfinite(modes.block_wavenumbers).all()
    assert modes.block_variances.shape == (4, PLANTED_MODES) and np.all(modes.block_variances > 0)
    assert np.isfinite(modes.wavenumber_errors).all() and np.all(modes.wavenumber_errors >= 0)
    np.testing.assert_array_equal(modes.counts, [PLANTED_FRAMES, PLANTED_FRAMES - 1])
    whole = trajectory.get_quasiharmonic_modes(LATTICE, masses)
    np.testing.assert_allclose(modes.wavenumbers_steps, whole.wavenumbers_steps, rtol=1e-9)
    # the run and its time reversal: the step across the boundary is dropped
    ensemble = TrajectoryEnsemble([trajectory, Trajectory(positions[::-1], PLANTED_TIMESTEP)])
    joined = ensemble.get_quasiharmonic_modes(LATTICE, masses, blocks=2)
    np.testing.assert_array_equal(joined.counts, [2 * PLANTED_FRAMES, 2 * (PLANTED_FRAMES - 1)])
    assert joined.rank == PLANTED_MODES and joined.block_wavenumbers.shape == (4, PLANTED_MODES)
    np.testing.assert_allclose(joined.wavenumbers_steps, whole.wavenumbers_steps, rtol=1e-9)
    bounds, flags = run_blocks([10, 7], 3)
    np.testing.assert_array_equal(bounds, [0, 3, 6, 10, 12, 14, 17])
    np.testing.assert_array_equal(flags, [1, 1, 0, 1, 1, 0])


def test_value_errors():
    positions, masses, _, _ = planted_run()
    short = positions[:40]
    trajectory = Trajectory(short, 1.0)
    for on_device in (False, True):  # (before any device work: this machine may have no GPU)
        call = lambda t=trajectory, lattice=LATTICE, m=masses, **kw: t.get_quasiharmonic_modes(  # noqa: E731
            lattice, m, on_device=on_device, **kw)
        with pytest.raises(ValueError, match="at least 2 frames"):
            call(t=Trajectory(short[:1], 1.0))
        with pytest.raises(ValueError, match="blocks"):
            call(blocks=0)
        with pytest.raises(ValueError, match="blocks"):
            call(blocks=41)
        with pytest.raises(ValueError, match="blocks"):
            call(blocks=2.0)
        with pytest.raises(ValueError, match="incompatible"):
            call(t=Trajectory(short, 1.0, lattice_ts=np.broadcast_to(LATTICE, (40, 3, 3))))
        with pytest.raises(ValueError, match="lattice"):
            call(lattice=None)
        with pytest.raises(ValueError, match="lattice"):
            call(lattice=LATTICE[:2])
        with pytest.raises(ValueError, match="singular"):
            call(lattice=np.ones((3, 3)))
        with pytest.raises(ValueError, match="masses"):
            call(m=masses[:4])
        with pytest.raises(ValueError, match="masses"):
            call(m=-masses)
        with pytest.raises(ValueError, match="temperature"):
            call(temperature=0.0)
        with pytest.raises(ValueError, match="temperature"):
            call(temperature=-3.0)
        with pytest.raises(ValueError, match="ref_positions"):
            call(ref_positions=short[0][:4])
        with pytest.raises(ValueError, match="ref_positions"):
            call(ref_positions=short[0].reshape(-1))
        ensemble = TrajectoryEnsemble([trajectory, Trajectory(short[:3], 1.0)])
        with pytest.raises(ValueError, match="blocks"):
            ensemble.get_quasiharmonic_modes(LATTICE, masses, blocks=4, on_device=on_device)
        with pytest.raises(ValueError, match="incompatible"):
            TrajectoryEnsemble([Trajectory(short, 1.0, lattice_ts=np.broadcast_to(LATTICE, (40, 3, 3)))]
                               ).get_quasiharmonic_modes(LATTICE, masses, on_device=on_device)
    still = Trajectory(np.broadcast_to(short[0], (6, 5, 3)).copy(), 1.0)
    with pytest.raises(ValueError, match="rank 0"):
        still.get_quasiharmonic_modes(LATTICE, masses)
    with pytest.raises(ValueError):
        modes_from_moments(np.zeros((1, 15)), np.zeros((1, 2, 15, 15)), np.array([[4, 3]]), LATTICE, masses[:4], 1.0)
    with pytest.raises(ValueError):
        moments_host(short, short[0], [0, 20, 20, 40], [1, 1, 0])
    with pytest.raises(ValueError):
        moments_host(short, short[0], [0, 20, 40], [1, 1])


def _call(frames=6, atoms=2, bounds=(0, 2, 6), joined=(1, 0), blocks=None, null=None):
    lib = _lib.load()
    bounds, joined = np.array(bounds, dtype=np.int64), np.array(joined, dtype=np.int32)
    blocks = len(joined) if blocks is None else blocks
    rows, columns, count = max(frames, 1), 3 * max(atoms, 1), max(blocks, 1)
    arrays = {"pos": np.full((rows, columns), 0.25), "anchor": np.full(columns, 0.25), "bounds": bounds, "joined": joined,
              "first": np.zeros((count, columns)), "second": np.zeros((count, 2, columns, columns)),
              "counts": np.zeros((count, 2), dtype=np.int64)}
    p = {name: C.c_void_p(None if name == null else array.ctypes.data) for name, array in arrays.items()}
    rc = lib.rn_qh_moments(0, p["pos"], frames, atoms, p["anchor"], p["bounds"], p["joined"], blocks, p["first"],
                           p["second"], p["counts"])
    return rc, lib.rn_qh_last_error().decode()


def test_the_c_entry_refuses_bad_arguments_before_it_touches_the_device():
    refusals = [(dict(null=name), "null pointer") for name in ("pos", "anchor", "bounds", "joined", "first", "second", "counts")]
    refusals += [
        (dict(atoms=0), "not positive"),
        (dict(atoms=-1), "not positive"),
        (dict(frames=0, bounds=(0, 0), joined=(0,)), "not positive"),
        (dict(blocks=0), "B = 0"),
        (dict(blocks=-2), "B = -2"),
        (dict(bounds=(1, 2, 6)), "from 0 to T"),
        (dict(bounds=(0, 2, 5)), "from 0 to T"),
        (dict(bounds=(0, 2, 7)), "from 0 to T"),
        (dict(bounds=(0, 0, 6)), "strictly ascending"),
        (dict(bounds=(0, 4, 3, 6), joined=(1, 1, 0)), "strictly ascending"),
        (dict(joined=(2, 0)), "neither 0 nor 1"),
        (dict(joined=(-1, 0)), "neither 0 nor 1"),
        (dict(joined=(1, 1)), "last block"),
        (dict(bounds=(0, 6), joined=(1,)), "last block"),
    ]
    for arguments, text in refusals:
        rc, message = _call(**arguments)
        assert rc == _lib.RN_ERR_INVALID_ARGUMENT, (arguments, rc)
        assert text in message, (arguments, message)
    chunk = _lib.load().rn_qh_chunk_frames()
    assert chunk >= 16 and chunk % 4 == 0


def test_new_symbols_are_declared_listed_and_exported():
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True,
                        text=True).stdout
    exported = set(re.findall(r" T (\w+)", nm))
    with open(os.path.join(ROOT, "include", "rn_quasiharmonic.h"), encoding="utf-8") as file:
        text = re.sub(r"/\*.*?\*/", "", file.read(), flags=re.S)
    assert set(re.findall(r"\b(rn_qh_\w+)\s*\(", text)) == set(ENTRIES)
    assert set(_lib.QH_SIGNATURES) == set(ENTRIES)
    assert not set(ENTRIES) & (set(_lib.SIGNATURES) | set(_lib.LINESHAPE_SIGNATURES) | set(_lib.INTERP_SIGNATURES))
    for name in ENTRIES:
        assert name in exported, name
    host, device = _lib.QH_SIGNATURES["rn_qh_moments"], _lib.QH_SIGNATURES["rn_qh_moments_device"]
    assert device[0] == host[0] and device[1] == host[1] + [C.c_void_p]
