"""Band modes of MD runs (``ramannoodle_amd.bandmodes``): what needs no GPU.

``band_moments_host`` against a loop written from the definition, the trace identity that ties it to the VDOS, planted
modes recovered whole and by segments, the Raman tensors of a linear polarizability, ensembles, every ``ValueError``, the
C entry's refusals (they come before the device is touched) and the new symbols."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ramannoodle_amd import _lib
from ramannoodle_amd.bandmodes import (BandModes, band_moments_host, band_series, modes_from_band_moments)
from ramannoodle_amd.dynamics import Phonons, Trajectory, TrajectoryEnsemble
from ramannoodle_amd.spectrum import (_PER_FS_TO_CM1, _segment_starts, _symmetric_components, _vdos_host, band_weights,
                                      ensemble_segment_starts, mode_vectors, segment_plan)
from tests.quasiharmonic_cases import LATTICE, PLANTED_FRAMES, PLANTED_MODES, PLANTED_TIMESTEP, face_frames, planted_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rn_bm_moments", "rn_bm_moments_device", "rn_bm_set_profiling", "rn_bm_phase_times", "rn_bm_last_error")
EPSILON = np.finfo(np.float64).eps
COMPONENTS = ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, 2))


def definition(positions, lattice, masses, alpha, width, starts, taper, bin_weights):
    """The definition, term by term: a loop over the segments, the bins, the times and the columns."""
    frames, atoms = positions.shape[:2]
    columns = 3 * atoms
    x = np.zeros((frames - 1, columns + (0 if alpha is None else 6)))
    for t in range(frames - 1):
        for i in range(atoms):
            step = positions[t + 1, i] - positions[t, i]
            step = (step - np.rint(step)) @ lattice
            x[t, 3 * i:3 * i + 3] = np.sqrt(masses[i]) * step
        if alpha is not None:
            difference = alpha[t + 1] - alpha[t]
            for c, (a, b) in enumerate(COMPONENTS):
                x[t, columns + c] = 0.5 * (difference[a, b] + difference[b, a])
    steps = width - 1
    moments = np.zeros((len(bin_weights), x.shape[1], x.shape[1]))
    for start in starts:
        for m in range(1, bin_weights.shape[1] + 1):
            transform = np.zeros(x.shape[1], dtype=complex)
            for t in range(steps):
                transform += taper[t] * x[start + t] * np.exp(-2j * np.pi * m * t / steps)
            cross = np.real(transform[:, None] * np.conj(transform[None, :]))
            for b in range(len(bin_weights)):
                moments[b] += bin_weights[b, m - 1] * cross
    return moments / len(starts)


@pytest.mark.parametrize("with_alpha", [False, True])
def test_band_moments_host_is_the_definition(with_alpha):
    """Both sides sum the same (at most 2 x 5 x 11 = 110) products in another order, each transform itself a sum of 11
    terms: within 200 eps of sqrt(want_jj want_ll), which bounds every entry of a positive semi-definite matrix."""
    positions = face_frames(3, 12, seed=5)
    rng = np.random.default_rng(2)
    alpha = rng.normal(size=(12, 3, 3)) if with_alpha else None
    masses = rng.uniform(1.0, 4.0, 3)
    taper = rng.uniform(0.5, 1.5, 9)
    starts = np.array([0, 2])
    weights = np.array([[1.0, 0.0, 1.0, 0.0], [0.3, 2.5, 0.0, 0.0]])
    assert np.abs(np.diff(positions, axis=0)).max() > 0.9  # the minimum image acts
    got = band_moments_host(positions, LATTICE, masses, alpha, 10, starts, taper, weights)
    want = definition(positions, LATTICE, masses, alpha, 10, starts, taper, weights)
    assert got.shape == (2, 15 if with_alpha else 9, 15 if with_alpha else 9)
    for b in range(2):
        np.testing.assert_array_equal(got[b], got[b].T)
        scale = np.sqrt(np.outer(np.diag(want[b]), np.diag(want[b])))
        assert np.all(np.diag(want[b]) > 0)
        assert (np.abs(got[b] - want[b]) / scale).max() <= 200 * EPSILON


@pytest.mark.parametrize("segment_steps, taper", [(None, "boxcar"), (512, "hann")])
@pytest.mark.parametrize("corrected", [False, True])
def test_trace_identity_ties_the_moments_to_the_vdos(segment_steps, taper, corrected):
    """trace(moments[b][:K,:K]) = 2 sum_m bw[b][m] D[m] - (sum_m bw[b][m]) mean_q sum_{t,j} (taper[t] x[t][j])^2 with
    the one-group VDOS D of the same table: to 1e-12 relative."""
    positions, masses, _, _ = planted_run()
    width = PLANTED_FRAMES if segment_steps is None else segment_steps
    width, hop, tau = segment_plan(PLANTED_FRAMES, width, width if segment_steps is None else None, taper)
    starts = _segment_starts(PLANTED_FRAMES, width, hop)
    assert len(starts) == (1 if segment_steps is None else 7)
    axis, density = _vdos_host(positions, LATTICE[None], masses, np.zeros(5, dtype=np.int32), 1, PLANTED_TIMESTEP, width,
                               starts, tau, True)
    weights = band_weights(axis, [[100.0, 900.0], [300.0, 2000.0], [650.0, 700.0]], bose_einstein_correction=corrected)
    assert corrected == bool(np.any((weights != 0) & (weights != 1)))
    moments = band_moments_host(positions, LATTICE, masses, None, width, starts, tau, weights)
    series = band_series(positions, LATTICE, masses)
    zero_lag = np.mean([((tau[:, None] * series[start:start + width - 1]) ** 2).sum() for start in starts])
    for b in range(len(weights)):
        trace = np.trace(moments[b])
        want = 2.0 * (weights[b] * density[0]).sum() - weights[b].sum() * zero_lag
        print(f"band {b}: trace {trace:.15e}, from the VDOS {want:.15e}, relative {abs(trace - want) / abs(want):.1e}")
        assert abs(trace - want) <= 1e-12 * abs(want)


def _bands(wavenumbers, steps, half_bins):
    spacing = _PER_FS_TO_CM1 / (steps * PLANTED_TIMESTEP)
    return np.array([[w - half_bins * spacing, w + half_bins * spacing] for w in wavenumbers]), spacing


def _top_overlaps(modes, planted):
    return np.array([abs((modes.vectors[b][0] * planted[b]).sum()) for b in range(len(planted))])


def test_planted_modes_whole_run():
    positions, masses, planted, wavenumbers = planted_run()
    bands, spacing = _bands(wavenumbers, PLANTED_FRAMES - 1, 3.5)
    modes = Trajectory(positions, PLANTED_TIMESTEP).get_band_modes(bands, LATTICE, masses)
    assert isinstance(modes, BandModes) and modes.alpha_moments is None and modes.mode_raman_tensors is None
    assert modes.moments.shape == (PLANTED_MODES, 15, 15) and len(modes.wavenumber_axis) == (PLANTED_FRAMES - 1 + 1) // 2 - 1
    np.testing.assert_array_equal(modes.bin_counts, 7)
    np.testing.assert_array_equal(modes.bands, bands)
    overlaps = _top_overlaps(modes, planted)
    top_shares = np.array([modes.shares[b][0] for b in range(PLANTED_MODES)])
    top_wavenumbers = np.array([modes.wavenumbers[b][0] for b in range(PLANTED_MODES)])
    print(f"whole run: min overlap {overlaps.min():.6f}, min share {top_shares.min():.6f}, wavenumbers off by at most "
          f"{np.abs(top_wavenumbers - wavenumbers).max() / spacing:.3f} bins")
    assert overlaps.min() >= 0.999
    assert top_shares.min() >= 0.99
    assert np.abs(top_wavenumbers - wavenumbers).max() <= spacing
    for b in range(PLANTED_MODES):
        rank = len(modes.eigenvalues[b])
        assert modes.vectors[b].shape == (rank, 5, 3) and modes.shares[b].shape == (rank,) == modes.wavenumbers[b].shape
        assert np.all(np.diff(modes.eigenvalues[b]) <= 0) and rank <= 12  # three translations are projected out
        flat = modes.vectors[b].reshape(rank, -1)
        np.testing.assert_allclose(flat @ flat.T, np.eye(rank), rtol=0, atol=1e-12)
    # the chain into the mode-projected VDOS
    phonons = modes.phonons(4, positions[0])
    assert isinstance(phonons, Phonons)
    np.testing.assert_allclose(mode_vectors(phonons.displacements, LATTICE, masses), modes.vectors[4], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(phonons.wavenumbers, modes.wavenumbers[4])
    axis, rows = Trajectory(positions, PLANTED_TIMESTEP).get_mode_vdos(phonons, LATTICE, masses).measure()
    assert abs(axis[rows[0].argmax()] - wavenumbers[4]) <= 1.01 * spacing
    with pytest.raises(ValueError, match="band"):
        modes.phonons(12, positions[0])
    with pytest.raises(ValueError, match="ref_positions"):
        modes.phonons(0, positions[0][:4])


def test_planted_modes_segments():
    positions, masses, planted, wavenumbers = planted_run()
    bands, _ = _bands(wavenumbers, 511, 1.5)
    modes = Trajectory(positions, PLANTED_TIMESTEP).get_band_modes(bands, LATTICE, masses, segment_steps=512)
    overlaps = _top_overlaps(modes, planted)
    print(f"Hann segments of 512: min overlap {overlaps.min():.6f}")
    assert overlaps.min() >= 0.98
    assert len(modes.wavenumber_axis) == 255


def _linear_alpha(positions, rng):
    """alpha linear in the unwrapped Cartesian displacements from frame 0: ``(alpha[S][3][3], R[3][3][3N])``."""
    steps = np.diff(positions, axis=0)
    steps -= np.rint(steps)
    cartesian = np.concatenate([np.zeros((1, 15)), np.cumsum((steps @ LATTICE).reshape(len(steps), -1), axis=0)])
    response = rng.normal(size=(3, 3, 15))
    response = 0.5 * (response + response.transpose(1, 0, 2))
    return np.einsum("abj,tj->tab", response, cartesian) + rng.normal(size=(3, 3)), response


class _Recorded:
    """A model that returns recorded polarizabilities."""

    def __init__(self, alpha, atoms):
        self.alpha, self.num_atoms = alpha, atoms

    def calc_polarizabilities(self, positions):
        assert len(positions) == len(self.alpha)
        return self.alpha


def test_linear_polarizability_gives_back_its_raman_tensors():
    positions, masses, _, wavenumbers = planted_run()
    alpha, response = _linear_alpha(positions, np.random.default_rng(3))
    bands, _ = _bands(wavenumbers, PLANTED_FRAMES - 1, 3.5)
    trajectory = Trajectory(positions, PLANTED_TIMESTEP)
    modes = trajectory.get_band_modes(bands, LATTICE, masses, polarizability_model=_Recorded(alpha, 5))
    assert modes.moments.shape == (PLANTED_MODES, 21, 21) and modes.alpha_moments.shape == (PLANTED_MODES, 6, 6)
    assert modes.raman_patterns.shape == (PLANTED_MODES, 6, 5, 3)
    weighted = response / np.repeat(np.sqrt(masses), 3)[None, None, :]
    worst = 0.0
    for b in range(PLANTED_MODES):
        np.testing.assert_array_equal(modes.raman_patterns[b].reshape(6, 15), modes.moments[b, 15:, :15])
        np.testing.assert_array_equal(modes.alpha_moments[b], modes.moments[b, 15:, 15:])
        assert modes.mode_raman_tensors[b].shape == (len(modes.eigenvalues[b]), 3, 3)
        got = modes.mode_raman_tensors[b][0]
        want = weighted @ modes.vectors[b][0].reshape(-1)
        np.testing.assert_array_equal(got, got.T)
        worst = max(worst, np.abs(got - want).max() / np.abs(want).max())
    print(f"top-mode Raman tensors of a linear polarizability: off by at most {worst:.1e} relative")
    assert worst <= 1e-9
    # every mode above the rank tolerance kept, translations too: sum_k lambda_k R_k (x) R_k = G C^+ G^T, which is the
    # polarizability's own moments when alpha is linear in the displacements
    every = trajectory.get_band_modes(bands, LATTICE, masses, polarizability_model=_Recorded(alpha, 5),
                                      remove_translations=False)
    for b in range(PLANTED_MODES):
        vectors = _symmetric_components(every.mode_raman_tensors[b])  # (r, 6)
        rebuilt = np.einsum("k,kc,kd->cd", every.eigenvalues[b], vectors, vectors)
        assert np.abs(rebuilt - every.alpha_moments[b]).max() <= 1e-9 * np.abs(every.alpha_moments[b]).max()


def test_ensembles_average_the_runs_and_never_cross_a_boundary():
    positions, masses, _, wavenumbers = planted_run()
    first, second = positions[:1024], positions[1024:]
    bands, _ = _bands(wavenumbers[[0, 5]], 1023, 3.5)
    runs = [Trajectory(first, PLANTED_TIMESTEP), Trajectory(second, PLANTED_TIMESTEP)]
    joined = TrajectoryEnsemble(runs).get_band_modes(bands, LATTICE, masses)
    own = [run.get_band_modes(bands, LATTICE, masses) for run in runs]
    mean = 0.5 * (own[0].moments + own[1].moments)
    # (sums of at most 14 segments of one sign on the diagonal, which bounds every entry, in another order: 14 eps)
    bound = 14 * EPSILON
    assert np.abs(joined.moments - mean).max() <= bound * np.abs(mean).max()
    # segments: the frame after the boundary belongs to the second run alone
    bands, _ = _bands(wavenumbers[[0, 5]], 255, 1.5)
    corrupted = second.copy()
    corrupted[0] = (corrupted[0] + 0.37) % 1.0
    segments = TrajectoryEnsemble(runs).get_band_modes(bands, LATTICE, masses, segment_steps=256)
    reference = [run.get_band_modes(bands, LATTICE, masses, segment_steps=256).moments for run in runs]
    mean = 0.5 * (reference[0] + reference[1])  # (both runs have 7 segments)
    assert np.abs(segments.moments - mean).max() <= bound * np.abs(mean).max()
    # ... so the first run's share does not change when that frame is corrupted, though the joined steps across it do
    other = TrajectoryEnsemble([runs[0], Trajectory(corrupted, PLANTED_TIMESTEP)])
    changed = other.get_band_modes(bands, LATTICE, masses, segment_steps=256)
    only_second = Trajectory(corrupted, PLANTED_TIMESTEP).get_band_modes(bands, LATTICE, masses, segment_steps=256)
    mean = 0.5 * (reference[0] + only_second.moments)
    assert np.abs(changed.moments - mean).max() <= bound * np.abs(mean).max()
    # the table itself: the first run's segments of the joined frames read nothing past frame 1023, bit for bit
    starts, run_index = ensemble_segment_starts([1024, 1024], 256)
    assert starts[run_index == 0].max() + 256 == 1024 and starts[run_index == 1].min() == 1024
    _, _, tau = segment_plan(1024, 256, None, "hann")
    weights = np.ones((1, 127))
    arguments = (LATTICE, masses, None, 256, starts[run_index == 0], tau, weights)
    np.testing.assert_array_equal(band_moments_host(np.concatenate([first, corrupted]), *arguments),
                                  band_moments_host(np.concatenate([first, second]), *arguments))
    with pytest.raises(ValueError, match="one length"):
        TrajectoryEnsemble([runs[0], Trajectory(second[:1000], PLANTED_TIMESTEP)]).get_band_modes(bands, LATTICE, masses)


def test_value_errors():
    positions, masses, _, _ = planted_run()
    short = positions[:40]
    trajectory = Trajectory(short, 1.0)
    bands = [[2000.0, 6000.0]]
    for on_device in (False, True):  # (before any device work: this machine may have no GPU)
        call = lambda t=trajectory, b=bands, lattice=LATTICE, m=masses, **kw: t.get_band_modes(  # noqa: E731
            b, lattice, m, on_device=on_device, **kw)
        with pytest.raises(ValueError, match="incompatible"):
            call(t=Trajectory(short, 1.0, lattice_ts=np.broadcast_to(LATTICE, (40, 3, 3))))
        with pytest.raises(ValueError, match="incompatible"):
            TrajectoryEnsemble([Trajectory(short, 1.0, lattice_ts=np.broadcast_to(LATTICE, (40, 3, 3)))]).get_band_modes(
                bands, LATTICE, masses, on_device=on_device)
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
        with pytest.raises(ValueError, match="bands"):
            call(b=[[1.0, 2.0, 3.0]])
        with pytest.raises(ValueError, match="empty"):
            call(b=[[500.0, 400.0]])
        with pytest.raises(ValueError, match="non-finite"):
            call(b=[[500.0, np.inf]])
        with pytest.raises(ValueError, match="holds no bin"):
            call(b=[[1.0, 2.0]])
        with pytest.raises(ValueError, match="at least three frames"):
            call(t=Trajectory(short[:2], 1.0))
        with pytest.raises(ValueError, match="at least three frames"):
            TrajectoryEnsemble([trajectory, Trajectory(short[:2], 1.0)]).get_band_modes(bands, LATTICE, masses,
                                                                                        on_device=on_device)
        with pytest.raises(ValueError, match="no bin"):
            call(t=Trajectory(short[:3], 1.0))
        with pytest.raises(ValueError, match="incompatible"):
            call(polarizability_model=_Recorded(np.zeros((40, 3, 3)), 4))
        with pytest.raises(ValueError, match="segment_steps"):
            call(segment_steps=41)
        with pytest.raises(ValueError, match="taper"):
            call(segment_steps=20, taper="triangle")
    still = Trajectory(np.broadcast_to(short[0], (40, 5, 3)).copy(), 1.0)
    with pytest.raises(ValueError, match="rank 0"):
        still.get_band_modes(bands, LATTICE, masses)
    with pytest.raises(ValueError):
        band_moments_host(short, LATTICE, masses, None, 40, [1], np.ones(39), np.ones((1, 19)))
    with pytest.raises(ValueError):
        band_moments_host(short, LATTICE, masses, None, 40, [0], np.ones(39), np.ones((1, 18)))
    with pytest.raises(ValueError):
        band_moments_host(short, LATTICE, masses, np.zeros((39, 3, 3)), 40, [0], np.ones(39), np.ones((1, 19)))
    with pytest.raises(ValueError):
        modes_from_band_moments(np.zeros((1, 15, 15)), np.zeros((1, 15, 15)), LATTICE, masses[:4], bands, [1.0], [1])


def _call(frames=8, atoms=2, width=6, starts=(0, 2), segments=None, rows=1, bins=None, null=None, mass=1.0,
          weight=1.0, alpha=False):
    lib = _lib.load()
    count = len(starts) if segments is None else segments
    bins = (width - 1 + 1) // 2 - 1 if bins is None else bins
    size = max(atoms, 1)
    arrays = {"pos": np.full((frames, size, 3), 0.25), "lattice": np.eye(3), "masses": np.full(size, mass),
              "alpha": np.zeros((frames, 3, 3)), "starts": np.array(starts, dtype=np.int64),
              "taper": np.ones(max(width - 1, 1)), "weights": np.full((max(rows, 1), max(bins, 1)), weight),
              "moments": np.zeros((max(rows, 1), 3 * size + 6, 3 * size + 6))}
    p = {name: C.c_void_p(None if name == null or (name == "alpha" and not alpha) else array.ctypes.data)
         for name, array in arrays.items()}
    rc = lib.rn_bm_moments(0, p["pos"], p["lattice"], frames, atoms, p["masses"], p["alpha"], width, p["starts"], count,
                           p["taper"], p["weights"], rows, bins, 0, p["moments"])
    return rc, lib.rn_bm_last_error().decode(), arrays["moments"]


def test_the_c_entry_refuses_bad_arguments_before_it_touches_the_device():
    refusals = [(dict(null=name), "null pointer") for name in ("pos", "lattice", "masses", "starts", "taper", "weights",
                                                               "moments")]
    refusals += [
        (dict(atoms=0), "N = 0"),
        (dict(atoms=-1), "N = -1"),
        (dict(rows=0), "B = 0"),
        (dict(rows=-2), "B = -2"),
        (dict(width=2, bins=0), "W = 2"),
        (dict(width=9), "start table"),          # more frames than the run has
        (dict(starts=(0, 3)), "start table"),    # the last segment would end past the run
        (dict(starts=(-1, 0)), "start table"),
        (dict(segments=0), "start table"),
        (dict(mass=0.0), "masses[0]"),
        (dict(mass=-1.0), "masses[0]"),
        (dict(mass=np.nan), "masses[0]"),
        (dict(mass=np.inf), "masses[0]"),
        (dict(bins=1), "bins = 1"),
        (dict(bins=3), "bins = 3"),
        (dict(weight=np.nan), "bin_weights[0][0]"),
        (dict(weight=-np.inf), "bin_weights[0][0]"),
    ]
    for arguments, text in refusals:
        for alpha in (False, True):
            rc, message, _ = _call(alpha=alpha, **arguments)
            assert rc == _lib.RN_ERR_INVALID_ARGUMENT, (arguments, rc)
            assert text in message, (arguments, message)
    # weights that are all zero: zeros, and no device is needed
    rc, _, moments = _call(weight=0.0)
    assert rc == _lib.RN_OK and not moments.any()


def test_new_symbols_are_declared_listed_and_exported():
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True,
                        text=True).stdout
    exported = set(re.findall(r" T (\w+)", nm))
    with open(os.path.join(ROOT, "include", "rn_bandmodes.h"), encoding="utf-8") as file:
        text = re.sub(r"/\*.*?\*/", "", file.read(), flags=re.S)
    assert set(re.findall(r"\b(rn_bm_\w+)\s*\(", text)) == set(ENTRIES)
    assert set(_lib.BM_SIGNATURES) == set(ENTRIES)
    assert not set(ENTRIES) & (set(_lib.SIGNATURES) | set(_lib.LINESHAPE_SIGNATURES) | set(_lib.INTERP_SIGNATURES)
                               | set(_lib.QH_SIGNATURES) | set(_lib.HT_SIGNATURES))
    for name in ENTRIES:
        assert name in exported, name
    host, device = _lib.BM_SIGNATURES["rn_bm_moments"], _lib.BM_SIGNATURES["rn_bm_moments_device"]
    assert device[0] == host[0] and device[1] == host[1] + [C.c_void_p]
