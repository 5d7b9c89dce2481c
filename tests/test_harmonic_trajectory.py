"""Harmonic trajectories from ``Phonons`` (``ramannoodle_amd.harmonic``): what needs no GPU.

``synthesize_host`` against the definition written as loops, the planted round trip through the quasi-harmonic analysis
and the mode VDOS, quantum amplitudes, random sampling, the selection of modes, every ``ValueError``, the C entry's
refusals (they come before the device is touched) and the new symbols."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from ramannoodle_amd import _lib, harmonic
from ramannoodle_amd.constants import BOLTZMANN_CONSTANT, REDUCED_PLANCK_CONSTANT
from ramannoodle_amd.dynamics import Phonons, Trajectory, TrajectoryEnsemble
from ramannoodle_amd.quasiharmonic import AMU_A2_PER_FS2_IN_EV
from ramannoodle_amd.spectrum import mode_vectors
from tests.harmonic_cases import face_sites, minimum_image, planted_phonons, raw_inputs
from tests.quasiharmonic_cases import LATTICE, PLANTED_FRAMES, PLANTED_MODES, PLANTED_TIMESTEP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rn_ht_synthesize", "rn_ht_synthesize_device", "rn_ht_set_profiling", "rn_ht_phase_times", "rn_ht_last_error")


def test_synthesize_host_is_the_definition_written_as_loops():
    """Both sides take the same cosines of the same angles (bit for bit: one product, one sum) and the same products;
    they differ by the order of the sum over M = 7 modes and, at most, one rounding of the product of three factors:
    (M + 2) eps s_j, then one addition to a value below 2 and the wrap: 2^-51."""
    atoms, modes, runs, frames, first = 3, 7, 2, 5, 11
    ref, D, omega_dt, amp, phase = raw_inputs(atoms, modes, runs, seed=3)
    got = harmonic.synthesize_host(ref, D, omega_dt, amp, phase, frames, first)
    assert got.shape == (runs, frames, atoms, 3) and got.dtype == np.float64
    want = np.zeros((runs, frames, 3 * atoms))
    angles = np.zeros((runs, frames, modes))
    for r in range(runs):
        for t in range(frames):
            for j in range(3 * atoms):
                y = 0.0
                for m in range(modes):
                    theta = float(omega_dt[m]) * float(first + t)
                    theta = theta + float(phase[r, m])
                    angles[r, t, m] = theta
                    y += float(amp[r, m]) * math.cos(theta) * float(D[m, j])
                y = float(ref.reshape(-1)[j]) + y
                want[r, t, j] = y - math.floor(y)
    reach = (np.abs(amp)[:, :, None] * np.abs(D)[None]).sum(axis=1).max(axis=0)
    difference = np.abs(minimum_image(got.reshape(want.shape) - want))
    print(f"loops: worst difference {difference.max():.2e}")
    assert np.all(difference <= (modes + 2) * 2.0 ** -52 * reach + 2.0 ** -51)
    assert np.all((got >= 0) & (got <= 1))
    # the wrap acts: coordinates on both sides of a face
    assert np.ptp(got.reshape(want.shape)[:, :, ::3], axis=1).max() > 0.9
    # the angle is one rounded product and one rounded sum
    np.testing.assert_array_equal(angles, omega_dt[None, None] * (first + np.arange(frames, dtype=np.float64))[None, :, None]
                                  + phase[:, None])
    # a frame depends on its absolute index only; a single run may be given as (M,)
    np.testing.assert_array_equal(harmonic.synthesize_host(ref, D, omega_dt, amp, phase, 2, first + 3), got[:, 3:5])
    np.testing.assert_array_equal(harmonic.synthesize_host(ref, D.reshape(modes, atoms, 3), omega_dt, amp[1], phase[1],
                                                           frames, first)[0], got[1])


def _overlaps(vectors, planted):
    return np.abs(np.einsum("mk,mk->m", vectors.reshape(len(vectors), -1), planted.reshape(len(planted), -1)))


def planted_checks(modes, axis, rows, vectors, wavenumbers, label):
    """The four bounds of the planted round trip (shared with the GPU tests): conditions the statement meets with room
    (a numpy prototype gave 3e-15, 1 - 7e-16, 2.4e-4 and 0.06 bins), not measurements of the code."""
    assert modes.rank == PLANTED_MODES
    temperature = np.abs(modes.wavenumbers_temperature / wavenumbers - 1.0).max()
    overlaps = _overlaps(modes.vectors, vectors)
    steps = np.abs(modes.wavenumbers_steps / wavenumbers - 1.0).max()
    bins = np.abs(axis[rows.argmax(axis=1)] - wavenumbers).max() / (axis[1] - axis[0])
    print(f"{label}: temperature estimate off by {temperature:.2e}, 1 - min overlap {1.0 - overlaps.min():.2e}, steps "
          f"estimate off by {steps:.2e}, peaks off by {bins:.3f} bins")
    assert temperature <= 1e-9
    assert overlaps.min() >= 1.0 - 1e-9
    assert steps <= 1e-3
    assert rows.shape == (PLANTED_MODES, len(axis)) and bins <= 1.01


def test_planted_round_trip():
    phonons, masses, vectors, wavenumbers = planted_phonons()
    trajectory = phonons.get_harmonic_trajectory(LATTICE, 300.0, PLANTED_FRAMES, PLANTED_TIMESTEP, masses)
    assert isinstance(trajectory, Trajectory) and len(trajectory) == PLANTED_FRAMES and trajectory.timestep == 1.0
    positions = trajectory.positions_ts
    assert positions.shape == (PLANTED_FRAMES, 5, 3) and np.all((positions >= 0) & (positions < 1))
    assert np.ptp(positions[:, :, 0], axis=0).min() > 0.9  # every atom crosses its face
    modes = trajectory.get_quasiharmonic_modes(LATTICE, masses, temperature=300.0)
    axis, rows = trajectory.get_mode_vdos(phonons, LATTICE, masses).measure()
    planted_checks(modes, axis, rows, vectors, wavenumbers, "host")
    # the mean structure is the reference: commensurate cosines sum to zero
    assert np.abs(minimum_image(modes.mean_positions - phonons.ref_positions)).max() <= 1e-12


def test_quantum_amplitudes():
    phonons, masses, _, wavenumbers = planted_phonons()
    omega = harmonic.angular_frequencies(wavenumbers)
    run = lambda temperature, statistics: phonons.get_harmonic_trajectory(  # noqa: E731
        LATTICE, temperature, PLANTED_FRAMES, PLANTED_TIMESTEP, masses, statistics=statistics
    ).get_quasiharmonic_modes(LATTICE, masses).variances
    thermal = BOLTZMANN_CONSTANT * 30.0
    want = REDUCED_PLANCK_CONSTANT / (2.0 * omega) / np.tanh(REDUCED_PLANCK_CONSTANT * omega / (2.0 * thermal)) / AMU_A2_PER_FS2_IN_EV
    got = run(30.0, "quantum")  # (ascending in the frequency, as the planted modes are)
    print(f"quantum variances at 30 K off by {np.abs(got / want - 1.0).max():.2e}")
    np.testing.assert_allclose(got, want, rtol=1e-9)
    classical = run(30.0, "classical")
    np.testing.assert_allclose(classical, thermal / (AMU_A2_PER_FS2_IN_EV * omega ** 2), rtol=1e-9)
    assert np.all(got > 2.0 * classical)  # zero-point motion: hbar omega / 2 > 8 k_B T for every planted mode
    # towards the classical variances as T grows: x coth x = 1 + x^2 / 3 - .., x = hbar omega / (2 k_B T)
    ratios = []
    for temperature in (3.0e3, 3.0e4, 3.0e6):
        energies = harmonic.mode_energies(wavenumbers, temperature, "quantum")
        x = REDUCED_PLANCK_CONSTANT * omega / (2.0 * BOLTZMANN_CONSTANT * temperature)
        np.testing.assert_allclose(energies / (BOLTZMANN_CONSTANT * temperature), 1.0 + x ** 2 / 3.0, rtol=0, atol=x.max() ** 4)
        ratios.append((energies / (BOLTZMANN_CONSTANT * temperature) - 1.0).max())
    assert ratios[0] > ratios[1] > ratios[2] > 0 and ratios[2] < 1e-6
    warm = run(300.0, "quantum") / run(300.0, "classical")
    np.testing.assert_allclose(warm, harmonic.mode_energies(wavenumbers, 300.0, "quantum") / (BOLTZMANN_CONSTANT * 300.0),
                               rtol=1e-9)


def test_random_sampling():
    """-log1p(-u) has mean 1 and variance 1: the mean of 4096 draws has the standard deviation 1/64, and the bound
    5 / sqrt(4096) is five of them."""
    wavenumbers = np.linspace(50.0, 900.0, 256)
    runs = 16
    amp, phase = harmonic.draw(wavenumbers, 250.0, "quantum", "random", runs, seed=2024)
    assert amp.shape == phase.shape == (runs, 256)
    again = harmonic.draw(wavenumbers, 250.0, "quantum", "random", runs, seed=2024)
    np.testing.assert_array_equal(again[0], amp)
    np.testing.assert_array_equal(again[1], phase)
    other = harmonic.draw(wavenumbers, 250.0, "quantum", "random", runs, seed=2025)
    assert not np.any(other[0] == amp) and not np.any(other[1] == phase)
    assert not np.any(amp[0] == amp[1]) and not np.any(phase[0] == phase[1])
    assert np.all((phase >= 0) & (phase < 2.0 * np.pi)) and np.all(amp > 0)
    omega = harmonic.angular_frequencies(wavenumbers)
    energies = harmonic.mode_energies(wavenumbers, 250.0, "quantum")
    ratio = amp ** 2 * omega[None] ** 2 * AMU_A2_PER_FS2_IN_EV / (2.0 * energies[None])
    print(f"random sampling: mean energy ratio {ratio.mean():.4f} over {ratio.size} draws")
    assert ratio.size == 4096 and abs(ratio.mean() - 1.0) <= 5.0 / np.sqrt(4096)
    assert abs(phase.mean() / np.pi - 1.0) <= 5.0 / np.sqrt(3.0 * 4096)  # uniform: standard deviation pi / sqrt 3
    # the documented order: per run the phases, then the energies, from one generator; a shorter draw is a prefix
    rng = np.random.default_rng(2024)
    for r in range(2):
        np.testing.assert_array_equal(phase[r], 2.0 * np.pi * rng.random(256))
        np.testing.assert_array_equal(amp[r], np.sqrt(2.0 * (energies * -np.log1p(-rng.random(256))) / AMU_A2_PER_FS2_IN_EV)
                                      / omega)
    np.testing.assert_array_equal(harmonic.draw(wavenumbers, 250.0, "quantum", "random", 3, seed=2024)[0], amp[:3])
    # mean sampling: every run at the mean energy, its own phases
    mean_amp, mean_phase = harmonic.draw(wavenumbers, 250.0, "classical", "mean", 2, seed=1)
    np.testing.assert_allclose(mean_amp ** 2 * omega[None] ** 2 * AMU_A2_PER_FS2_IN_EV / 2.0, BOLTZMANN_CONSTANT * 250.0,
                               rtol=1e-13)
    assert not np.any(mean_phase[0] == mean_phase[1])
    # through the public methods
    phonons, masses, _, _ = planted_phonons()
    call = lambda **kw: phonons.get_harmonic_ensemble(LATTICE, 300.0, 16, 1.0, masses, sampling="random", **kw)  # noqa: E731
    ensemble = call(runs=3, seed=4)
    assert isinstance(ensemble, TrajectoryEnsemble) and ensemble.run_lengths == [16, 16, 16]
    first, second, third = (t.positions_ts for t in ensemble.trajectories)
    assert not np.array_equal(first, second) and not np.array_equal(second, third)
    np.testing.assert_array_equal(call(runs=3, seed=4).trajectories[2].positions_ts, third)
    assert not np.array_equal(call(runs=1, seed=5).trajectories[0].positions_ts, first)
    np.testing.assert_array_equal(phonons.get_harmonic_trajectory(LATTICE, 300.0, 16, 1.0, masses, sampling="random",
                                                                  seed=4).positions_ts, first)


def _projections(trajectory, phonons, masses):
    """The amplitudes ``(T, M)`` of the trajectory's displacements from the reference along the modes of ``phonons``."""
    vectors = mode_vectors(phonons.displacements, LATTICE, masses)
    moved = minimum_image(trajectory.positions_ts - phonons.ref_positions[None]) @ LATTICE * np.sqrt(masses)[None, :, None]
    return np.einsum("tk,mk->tm", moved.reshape(len(moved), -1), vectors.reshape(len(vectors), -1))


def test_selection_of_modes():
    planted, masses, vectors, wavenumbers = planted_phonons()
    # the planted modes and three translations of no, negative (imaginary) and tiny frequency
    translations = np.broadcast_to(np.eye(3)[:, None, :], (3, 5, 3)) @ np.linalg.inv(LATTICE)
    phonons = Phonons(planted.ref_positions, np.concatenate([[0.0, -35.0, 0.4], wavenumbers]),
                      np.concatenate([translations, planted.displacements]))
    sqrt2 = np.sqrt(2.0)
    amplitude = np.sqrt(2.0 * BOLTZMANN_CONSTANT * 300.0 / AMU_A2_PER_FS2_IN_EV) / harmonic.angular_frequencies(wavenumbers)
    everything = _projections(phonons.get_harmonic_trajectory(LATTICE, 300.0, PLANTED_FRAMES, 1.0, masses), phonons, masses)
    np.testing.assert_allclose(np.sqrt((everything[:, 3:] ** 2).mean(axis=0)) * sqrt2, amplitude, rtol=1e-9)
    assert np.abs(everything[:, :3]).max() <= 1e-12  # default: the modes above 1 1/cm
    chosen = np.array([4, 9, 14])
    some = _projections(phonons.get_harmonic_trajectory(LATTICE, 300.0, PLANTED_FRAMES, 1.0, masses, modes=chosen), phonons,
                        masses)
    left_out = np.setdiff1d(np.arange(15), chosen)
    assert np.abs(some[:, left_out]).max() <= 1e-12  # the modes left out leave no motion along their vectors
    np.testing.assert_allclose(np.sqrt((some[:, chosen] ** 2).mean(axis=0)) * sqrt2, amplitude[chosen - 3], rtol=1e-9)
    np.testing.assert_array_equal(harmonic.phonon_arguments(phonons, LATTICE, 1.0, masses, min_wavenumber=0.3)[4],
                                  np.arange(2, 15))  # 0.4 1/cm is in
    ref, D, omega_dt, selected, index = harmonic.phonon_arguments(phonons, LATTICE, 1.0, masses, min_wavenumber=200.0)
    np.testing.assert_array_equal(index, np.flatnonzero(phonons.wavenumbers > 200.0))
    np.testing.assert_array_equal(selected, phonons.wavenumbers[index])
    np.testing.assert_allclose(D, (vectors[index - 3] / np.sqrt(masses)[None, :, None]) @ np.linalg.inv(LATTICE), rtol=0,
                               atol=1e-14)
    np.testing.assert_allclose(omega_dt, harmonic.angular_frequencies(selected), rtol=1e-15)
    for bad in (0, 1, 2):
        with pytest.raises(ValueError, match=f"mode {bad} "):
            phonons.get_harmonic_trajectory(LATTICE, 300.0, 8, 1.0, masses, modes=[5, bad])


def test_value_errors():
    phonons, masses, _, wavenumbers = planted_phonons()
    for on_device in (False, True):  # (before any device work: these tests run without a GPU)
        for method, more in ((phonons.get_harmonic_trajectory, {}), (phonons.get_harmonic_ensemble, {"runs": 2})):
            def call(lattice=LATTICE, temperature=300.0, steps=8, timestep=1.0, m=masses, **kw):
                return method(lattice, temperature, steps, timestep, m, on_device=on_device, **{**more, **kw})
            with pytest.raises(ValueError, match="lattice"):
                call(lattice=None)
            with pytest.raises(ValueError, match="lattice"):
                call(lattice=LATTICE[:2])
            with pytest.raises(ValueError, match="singular"):
                call(lattice=np.ones((3, 3)))
            with pytest.raises(ValueError, match="non-finite"):
                call(lattice=LATTICE * np.nan)
            with pytest.raises(ValueError, match="masses"):
                call(m=masses[:4])
            with pytest.raises(ValueError, match="masses"):
                call(m=-masses)
            with pytest.raises(ValueError, match="temperature"):
                call(temperature=0.0)
            with pytest.raises(ValueError, match="temperature"):
                call(temperature=-3.0)
            with pytest.raises(ValueError, match="steps"):
                call(steps=0)
            with pytest.raises(ValueError, match="steps"):
                call(steps=2.0)
            with pytest.raises(ValueError, match="timestep"):
                call(timestep=0.0)
            with pytest.raises(ValueError, match="timestep"):
                call(timestep=-1.0)
            with pytest.raises(ValueError, match="mode 11 .*pi"):  # 117 cycles in 2048 fs: the only mode past half a cycle in 9 fs
                call(timestep=9.0)
            with pytest.raises(ValueError, match="mode 7 .*pi"):  # 89 cycles: past half a cycle in 12 fs; 54 cycles are not
                call(timestep=12.0, modes=[2, 7])
            with pytest.raises(ValueError, match="statistics"):
                call(statistics="bose")
            with pytest.raises(ValueError, match="sampling"):
                call(sampling="median")
            with pytest.raises(ValueError, match="no mode left"):
                call(min_wavenumber=5000.0)
            with pytest.raises(ValueError, match="no mode left"):
                call(modes=np.array([], dtype=np.int64))
            with pytest.raises(ValueError, match="modes"):
                call(modes=[12])
            with pytest.raises(ValueError, match="modes"):
                call(modes=[0.5])
            with pytest.raises(ValueError, match="mode 3 "):
                call(modes=[3], min_wavenumber=float(wavenumbers[3]))
        with pytest.raises(ValueError, match="runs"):
            phonons.get_harmonic_ensemble(LATTICE, 300.0, 8, 1.0, masses, runs=0, on_device=on_device)
        with pytest.raises(ValueError, match="runs"):
            phonons.get_harmonic_ensemble(LATTICE, 300.0, 8, 1.0, masses, runs=1.5, on_device=on_device)
    ref, D, omega_dt, amp, phase = raw_inputs(2, 3, 2, seed=0)
    for arguments in ((ref[:1].reshape(-1)[:2], D, omega_dt, amp, phase, 4), (ref, D[:, :5], omega_dt, amp, phase, 4),
                      (ref, D, omega_dt[:2], amp, phase, 4), (ref, D, omega_dt, amp[:, :2], phase, 4),
                      (ref, D, omega_dt, amp, phase[:1], 4), (ref, D, omega_dt, amp, phase, 0),
                      (ref, D, omega_dt, amp, phase, 4, -1), (ref, D, omega_dt, amp, phase, 4, 2 ** 53 - 3),
                      (ref, D, omega_dt, amp, phase, 4.0), (ref, D * np.inf, omega_dt, amp, phase, 4)):
        with pytest.raises(ValueError):
            harmonic.synthesize_host(*arguments)
    with pytest.raises(ValueError, match="statistics"):
        harmonic.mode_energies(np.array([100.0]), 300.0, "fermi")
    with pytest.raises(ValueError, match="wavenumbers"):
        harmonic.mode_energies(np.array([100.0, 0.0]), 300.0)


def _call(atoms=2, modes=3, runs=2, frames=4, first=0, null=None, poison=None, entry="rn_ht_synthesize"):
    lib = _lib.load()
    n, m, r, t = max(atoms, 1), max(modes, 1), max(runs, 1), max(frames, 1)
    arrays = {"ref": np.full(3 * n, 0.25), "D": np.full((m, 3 * n), 0.01), "omega_dt": np.full(m, 0.1),
              "amp": np.full((r, m), 0.5), "phase": np.full((r, m), 1.0), "out": np.zeros((r, min(t, 64), 3 * n))}
    if poison is not None:
        name, index, value = poison
        arrays[name].reshape(-1)[index] = value
    p = {name: C.c_void_p(None if name == null else array.ctypes.data) for name, array in arrays.items()}
    tail = (C.c_void_p(None),) if entry.endswith("_device") else ()
    rc = getattr(lib, entry)(0, p["ref"], p["D"], p["omega_dt"], p["amp"], p["phase"], atoms, modes, runs, frames, first,
                             p["out"], *tail)
    return rc, lib.rn_ht_last_error().decode()


def test_the_c_entries_refuse_bad_arguments_before_they_touch_the_device():
    refusals = [(dict(null=name), "null pointer") for name in ("ref", "D", "omega_dt", "amp", "phase", "out")]
    refusals += [
        (dict(atoms=0), "not positive"),
        (dict(atoms=-1), "not positive"),
        (dict(modes=0), "not positive"),
        (dict(modes=-4), "not positive"),
        (dict(runs=0), "not positive"),
        (dict(frames=0), "not positive"),
        (dict(frames=-1), "not positive"),
        (dict(first=-1), "t0 = -1"),
        (dict(first=2 ** 53 - 3), "2^53"),
        (dict(first=2 ** 53 + 1, frames=1), "2^53"),
        (dict(first=2 ** 62, frames=2 ** 62), "2^53"),
        (dict(frames=2 ** 50), "exceed the grid"),
        (dict(poison=("ref", 4, np.nan)), "ref[4]"),
        (dict(poison=("D", 17, np.inf)), "D[17]"),
        (dict(poison=("omega_dt", 2, -np.inf)), "omega_dt[2]"),
        (dict(poison=("amp", 5, np.nan)), "amp[5]"),
        (dict(poison=("phase", 0, np.inf)), "phase[0]"),
    ]
    for entry in ("rn_ht_synthesize", "rn_ht_synthesize_device"):
        for arguments, text in refusals:
            rc, message = _call(entry=entry, **arguments)
            assert rc == _lib.RN_ERR_INVALID_ARGUMENT, (entry, arguments, rc, message)
            assert text in message, (entry, arguments, message)
    lib = _lib.load()
    assert lib.rn_ht_phase_times(None) == _lib.RN_ERR_INVALID_ARGUMENT
    times = np.ones(3)
    assert lib.rn_ht_set_profiling(0) == _lib.RN_OK and lib.rn_ht_phase_times(C.c_void_p(times.ctypes.data)) == _lib.RN_OK
    assert not times.any()


def test_new_symbols_are_declared_listed_and_exported():
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True,
                        text=True).stdout
    exported = set(re.findall(r" T (\w+)", nm))
    with open(os.path.join(ROOT, "include", "rn_harmonic.h"), encoding="utf-8") as file:
        text = re.sub(r"/\*.*?\*/", "", file.read(), flags=re.S)
    assert set(re.findall(r"\b(rn_ht_\w+)\s*\(", text)) == set(ENTRIES)
    assert set(_lib.HT_SIGNATURES) == set(ENTRIES)
    assert not set(ENTRIES) & (set(_lib.SIGNATURES) | set(_lib.LINESHAPE_SIGNATURES) | set(_lib.INTERP_SIGNATURES)
                               | set(_lib.QH_SIGNATURES))
    for name in ENTRIES:
        assert name in exported, name
    host, device = _lib.HT_SIGNATURES["rn_ht_synthesize"], _lib.HT_SIGNATURES["rn_ht_synthesize_device"]
    assert device[0] == host[0] and device[1] == host[1] + [C.c_void_p]
    assert REDUCED_PLANCK_CONSTANT == 0.6582119569
    assert face_sites(4, np.random.default_rng(0)).shape == (4, 3)
