"""The mode-projected VDOS on the host: the definition, Parseval against the VDOS, selectivity, ``mode_vectors``, the tie to
the group VDOS, the argument checks of the classes and the raw entry's checks, which come before any device work.  Every
comparison is per row: ``max|got - want| / max|want|`` of that row."""
import ctypes as C

import numpy as np
import pytest

from ramannoodle_amd import _lib
from ramannoodle_amd.dynamics import Phonons, Trajectory, TrajectoryEnsemble
from ramannoodle_amd.spectrum import (ModeVibrationalDensityOfStates, ModeVibrationalDensityOfStatesEnsemble,
                                      VibrationalDensityOfStates, VibrationalDensityOfStatesEnsemble,
                                      calc_signal_spectrum, mode_vectors)
from ramannoodle_amd.structure import apply_pbc
from tests.test_vdos_gpu import DT, LATTICE, _run


def _basis(atoms, seed=3):
    """A random orthonormal basis of the ``3 atoms`` displacements: ``(3 atoms, atoms, 3)``."""
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3 * atoms, 3 * atoms)))
    return np.ascontiguousarray(q.T.reshape(3 * atoms, atoms, 3))


def _row_errors(got, want):
    assert got.shape == want.shape
    scale = np.abs(want).max(axis=-1)
    assert np.all(scale > 0)
    return np.abs(got - want).max(axis=-1) / scale


def _steps(f, lattice):
    d = np.diff(f, axis=0)
    d -= np.rint(d)
    if lattice.ndim == 2:
        return d @ lattice
    return np.einsum("tik,tkc->tic", d, 0.5 * (lattice[:-1] + lattice[1:]))


@pytest.mark.parametrize("per_frame", [False, True])
def test_a_whole_run_row_is_calc_signal_spectrum_of_the_mode_series(per_frame):
    f, lattice, masses, _ = _run(50, 5, 1, per_frame)
    vectors = np.random.default_rng(0).normal(size=(7, 5, 3))
    wavenumbers, rows = ModeVibrationalDensityOfStates(f, DT, lattice, vectors, masses).measure()
    y = np.einsum("kic,tic->kt", vectors, _steps(f, lattice) * np.sqrt(masses)[None, :, None])
    for k in range(7):
        w, s = calc_signal_spectrum(y[k], DT)
        np.testing.assert_array_equal(wavenumbers, w[1:])
        assert _row_errors(rows[k], s[1:]) <= 1e-12


@pytest.mark.parametrize("steps,atoms,per_frame", [(50, 5, False), (64, 67, False), (257, 130, True), (130, 33, False)])
def test_an_orthonormal_basis_sums_to_the_vdos(steps, atoms, per_frame):
    f, lattice, masses, _ = _run(steps, atoms, 1, per_frame)
    modes = ModeVibrationalDensityOfStates(f, DT, lattice, _basis(atoms), masses)
    whole = VibrationalDensityOfStates(f, DT, lattice, masses)
    assert modes.num_modes == 3 * atoms
    w_modes, got = modes.measure()
    w_whole, want = whole.measure()
    np.testing.assert_array_equal(w_modes, w_whole)
    errors = [_row_errors(got.sum(axis=0), want[0])]
    for average in (True, False):
        got = modes.measure_segments(17, 8, "hann", average)[1]
        want = whole.measure_segments(17, 8, "hann", average)[1]
        assert got.shape == want.shape[:-2] + (3 * atoms, want.shape[-1])
        errors.append(_row_errors(got.sum(axis=-2), want[..., 0, :]).max())
    print("Parseval misses:", errors)
    assert max(errors) <= 1e-12


def test_two_oscillating_basis_vectors_show_in_their_rows_only():
    atoms, frames, bins = 6, 400, (20, 57)
    n = frames - 1
    rng = np.random.default_rng(11)
    masses = rng.uniform(1.0, 100.0, atoms)
    basis = _basis(atoms)
    t = np.arange(n)
    amplitudes = {4: 0.05, 13: 0.025}  # row -> amplitude of its mass-weighted step
    weighted = sum(a * np.cos(2 * np.pi * b * t / n)[:, None, None] * basis[k]
                   for (k, a), b in zip(amplitudes.items(), bins))
    steps = (weighted / np.sqrt(masses)[None, :, None]) @ np.linalg.inv(LATTICE)
    assert np.abs(steps).max() < 0.4
    first = rng.random((atoms, 3))
    f = apply_pbc(np.concatenate([first[None], first + np.cumsum(steps, axis=0)]))  # wrapped into the cell
    _, rows = ModeVibrationalDensityOfStates(f, DT, LATTICE, basis, masses).measure()
    for row, b in zip(amplitudes, bins):
        assert rows[row].argmax() == b - 1  # (the zero bin is dropped)
    weaker = rows[13].max()
    others = np.abs(np.delete(rows, list(amplitudes), axis=0)).max()
    print(f"other rows / weaker peak: {others / weaker:.1e}")
    assert others <= 1e-20 * weaker


def test_mode_vectors():
    rng = np.random.default_rng(5)
    displacements, masses = 0.1 * rng.normal(size=(4, 5, 3)), rng.uniform(1.0, 100.0, 5)
    vectors = mode_vectors(displacements, LATTICE, masses)
    want = (displacements @ LATTICE) * np.sqrt(masses)[None, :, None]
    want /= np.sqrt((want ** 2).sum(axis=(1, 2)))[:, None, None]
    np.testing.assert_allclose(vectors, want, rtol=1e-15, atol=0)
    np.testing.assert_allclose((vectors ** 2).sum(axis=(1, 2)), 1.0, rtol=1e-14)
    spoiled = displacements.copy()
    spoiled[2] = 0.0
    with pytest.raises(ValueError, match="mode 2 has zero norm"):
        mode_vectors(spoiled, LATTICE, masses)
    spoiled[2, 1, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        mode_vectors(spoiled, LATTICE, masses)
    for bad in (displacements[0], displacements[:, :, :2]):
        with pytest.raises(ValueError, match="shape"):
            mode_vectors(bad, LATTICE, masses)
    with pytest.raises(ValueError):
        mode_vectors(displacements, LATTICE[:2], masses)
    with pytest.raises(ValueError):
        mode_vectors(displacements, LATTICE, masses[:4])
    with pytest.raises(ValueError):
        mode_vectors(displacements, np.zeros((3, 3)), masses)


def test_scaling_a_vector_by_three_scales_its_row_by_nine():
    f, lattice, masses, _ = _run(50, 5, 1)
    vectors = np.random.default_rng(2).normal(size=(3, 5, 3))
    scaled = vectors.copy()
    scaled[1] *= 3.0
    _, rows = ModeVibrationalDensityOfStates(f, DT, lattice, vectors, masses).measure()
    _, got = ModeVibrationalDensityOfStates(f, DT, lattice, scaled, masses).measure()
    assert _row_errors(got, rows * np.array([1.0, 9.0, 1.0])[:, None]).max() <= 1e-14


def test_cartesian_vectors_on_one_atom_sum_to_that_atoms_group_vdos():
    f, lattice, masses, _ = _run(64, 67, 1)
    atom = 41
    vectors = np.zeros((3, 67, 3))
    vectors[np.arange(3), atom, np.arange(3)] = 1.0
    labels = np.ones(67, dtype=np.int32)
    labels[atom] = 0
    for measure in (lambda v: v.measure()[1], lambda v: v.measure_segments(17, 8, "hann", False)[1]):
        got = measure(ModeVibrationalDensityOfStates(f, DT, lattice, vectors, masses))
        want = measure(VibrationalDensityOfStates(f, DT, lattice, masses, labels, 2))
        assert _row_errors(got.sum(axis=-2), want[..., 0, :]).max() <= 1e-12


def test_ensemble_takes_the_segments_of_every_run():
    masses = _run(50, 5, 1)[2]
    runs = [_run(steps, 5, 1)[0] for steps in (50, 41)]
    vectors = _basis(5)
    modes = ModeVibrationalDensityOfStatesEnsemble(runs, DT, LATTICE, vectors, masses)
    whole = VibrationalDensityOfStatesEnsemble(runs, DT, LATTICE, masses)
    _, got = modes.measure_segments(17, 8, "hann", False)
    _, want = whole.measure_segments(17, 8, "hann", False)
    assert got.shape == (len(want), 15, want.shape[-1])
    assert _row_errors(got.sum(axis=1), want[:, 0]).max() <= 1e-12
    for q, (run, start) in enumerate(zip(*modes.segment_starts(17, 8))):
        single = ModeVibrationalDensityOfStates(runs[run][start:start + 17], DT, LATTICE, vectors, masses)
        assert _row_errors(got[q], single.measure_segments(17, 17, "hann")[1]).max() <= 1e-12
    with pytest.raises(ValueError):
        modes.measure()  # runs of two lengths
    equal = ModeVibrationalDensityOfStatesEnsemble([runs[0][:41], runs[1]], DT, LATTICE, vectors, masses)
    parts = [ModeVibrationalDensityOfStates(run[:41], DT, LATTICE, vectors, masses).measure()[1] for run in runs]
    assert _row_errors(equal.measure()[1], 0.5 * (parts[0] + parts[1])).max() <= 1e-12


def _phonons(atoms, modes, seed=0):
    rng = np.random.default_rng(seed)
    return Phonons(rng.random((atoms, 3)), np.linspace(50.0, 900.0, modes), 0.1 * rng.normal(size=(modes, atoms, 3)))


def test_get_mode_vdos():
    f, lattice_ts, masses, _ = _run(50, 5, 1, True)
    phonons = _phonons(5, 9)
    vectors = mode_vectors(phonons.displacements, LATTICE, masses)
    fixed = Trajectory(f, DT).get_mode_vdos(phonons, LATTICE, masses)
    assert isinstance(fixed, ModeVibrationalDensityOfStates) and fixed.num_modes == 9
    np.testing.assert_array_equal(fixed.vectors, vectors)
    w, rows = fixed.measure()
    np.testing.assert_array_equal(w, Trajectory(f, DT).get_vdos(LATTICE, masses).measure()[0])
    np.testing.assert_array_equal(rows, ModeVibrationalDensityOfStates(f, DT, LATTICE, vectors, masses).measure()[1])
    # a lattice per frame serves the steps; `lattice` still converts the displacements
    variable = Trajectory(f, DT, lattice_ts).get_mode_vdos(phonons, LATTICE, masses, modes=[7, 2])
    np.testing.assert_array_equal(variable.vectors, vectors[[7, 2]])
    np.testing.assert_array_equal(
        variable.measure()[1], ModeVibrationalDensityOfStates(f, DT, lattice_ts, vectors[[7, 2]], masses).measure()[1])
    # unit masses
    np.testing.assert_array_equal(Trajectory(f, DT).get_mode_vdos(phonons, LATTICE).vectors,
                                  mode_vectors(phonons.displacements, LATTICE, np.ones(5)))
    ensemble = TrajectoryEnsemble([Trajectory(f, DT), Trajectory(f[:41], DT)]).get_mode_vdos(phonons, LATTICE, masses)
    assert isinstance(ensemble, ModeVibrationalDensityOfStatesEnsemble) and ensemble.run_lengths == [50, 41]
    assert ensemble.measure_segments(17, 8, average=False)[1].shape == (5 + 4, 9, 7)


def test_argument_errors():
    f, _, masses, _ = _run(50, 5, 1)
    vectors = np.random.default_rng(1).normal(size=(4, 5, 3))
    spoiled = vectors.copy()
    spoiled[3, 4, 2] = np.inf
    for bad in (vectors[0], vectors[:, :4], vectors[:, :, :2], np.zeros((0, 5, 3)), np.zeros((16, 5, 3)), spoiled):
        with pytest.raises(ValueError):
            ModeVibrationalDensityOfStates(f, DT, LATTICE, bad, masses)
        with pytest.raises(ValueError):
            ModeVibrationalDensityOfStatesEnsemble([f, f], DT, LATTICE, bad, masses)
    for bad in (None, "vectors", np.zeros((4, 5, 3), dtype=complex)):
        with pytest.raises(TypeError):
            ModeVibrationalDensityOfStates(f, DT, LATTICE, bad, masses)
    with pytest.raises(ValueError):
        ModeVibrationalDensityOfStates(f, DT, LATTICE[:2], vectors, masses)
    with pytest.raises(ValueError):
        ModeVibrationalDensityOfStates(f, DT, LATTICE, vectors, masses[:4])
    with pytest.raises(ValueError):
        ModeVibrationalDensityOfStates(f[:, :, :2], DT, LATTICE, vectors, masses)
    trajectory, phonons = Trajectory(f, DT), _phonons(5, 9)
    with pytest.raises(ValueError, match="lattice"):
        trajectory.get_mode_vdos(phonons, None, masses)
    with pytest.raises(ValueError, match="6 atoms != 5 atoms"):
        trajectory.get_mode_vdos(_phonons(6, 9), LATTICE, masses)
    for bad in ([9], [-1], [0, 12], [], [0.5]):
        with pytest.raises(ValueError, match="modes"):
            trajectory.get_mode_vdos(phonons, LATTICE, masses, modes=np.array(bad))
    with pytest.raises(ValueError):
        trajectory.get_mode_vdos(_phonons(5, 16), LATTICE, masses)  # M > 3N
    with pytest.raises(TypeError):
        trajectory.get_mode_vdos(phonons.displacements, LATTICE, masses)


def test_signatures_and_the_checks_before_any_device_work():
    """The ``_device`` entry is the host entry plus a stream; a bad argument is refused on a machine without a GPU too
    and the output stays untouched; a good call gets as far as the device check."""
    host, device = _lib.SIGNATURES["rn_md_mode_vdos"], _lib.SIGNATURES["rn_md_mode_vdos_device"]
    assert device == (host[0], host[1] + [C.c_void_p])
    assert len(host[1]) == 17 and host[1][7] is C.c_int32
    assert _lib.SIGNATURES["rn_md_mode_vdos_set_profiling"] == (C.c_int, [C.c_int])
    assert _lib.SIGNATURES["rn_md_mode_vdos_phase_times"] == (C.c_int, [C.c_void_p])
    lib = _lib.load()
    steps, atoms, modes, width = 20, 4, 5, 9
    f = np.ascontiguousarray(_run(steps, atoms, 1)[0])
    good = {"positions": f, "lattices": np.ascontiguousarray(LATTICE[None]), "num_lattices": 1, "S": steps, "N": atoms,
            "masses": np.array([1.0, 16.0, 12.0, 48.0]), "vectors": np.random.default_rng(0).normal(size=(modes, atoms, 3)),
            "M": modes, "segment_steps": width, "starts": np.array([0, 5, steps - width], dtype=np.int64), "Q": 3,
            "taper": np.ones(width - 1), "average": 0, "device": 0, "workspace_limit": 0,
            "densities": np.full((3, modes, 3), -7.0), "num_bins": 3}
    out = good["densities"]

    def call(**changes):
        keep = [np.ascontiguousarray(v) if isinstance(v, np.ndarray) and v is not out else v
                for v in dict(good, **changes).values()]
        raw = [C.c_void_p(v.ctypes.data) if isinstance(v, np.ndarray) else (C.c_void_p(None) if v is None else v)
               for v in keep]
        return lib.rn_md_mode_vdos(*raw), lib.rn_md_mode_vdos_device(*raw, C.c_void_p(None))

    def spoiled(value):
        bad = good["vectors"].copy()
        bad[modes - 1, atoms - 1, 2] = value
        return bad

    invalid = [
        *({name: None} for name in ("positions", "lattices", "masses", "vectors", "starts", "taper", "densities")),
        {"N": 0}, {"M": 0}, {"M": -1}, {"M": 3 * atoms + 1}, {"num_lattices": 2}, {"segment_steps": 2},
        {"segment_steps": steps + 1}, {"Q": 0}, {"num_bins": 4}, {"average": 2},
        {"starts": np.array([0, -1, 3], dtype=np.int64)}, {"starts": np.array([0, 5, steps - width + 1], dtype=np.int64)},
        {"masses": np.array([1.0, 0.0, 1.0, 1.0])}, {"masses": np.array([1.0, np.nan, 1.0, 1.0])},
        {"vectors": spoiled(np.nan)}, {"vectors": spoiled(np.inf)},
    ]
    for changes in invalid:
        assert call(**changes) == (_lib.RN_ERR_INVALID_ARGUMENT,) * 2, changes
        assert np.all(out == -7.0), changes
    assert all(rc != _lib.RN_ERR_INVALID_ARGUMENT for rc in call(device=4096))
    millis = (C.c_double * 4)(1.0, 1.0, 1.0, 1.0)
    assert lib.rn_md_mode_vdos_phase_times(None) == _lib.RN_ERR_INVALID_ARGUMENT
    assert lib.rn_md_mode_vdos_set_profiling(0) == _lib.RN_OK and lib.rn_md_mode_vdos_phase_times(millis) == _lib.RN_OK
    assert list(millis) == [0.0] * 4
