"""What the quasi-harmonic tests share (tests/test_quasiharmonic.py, tests/test_quasiharmonic_gpu.py,
tools/quasiharmonic_timing.py): the planted harmonic run, random frames near the cell faces, the frame-by-frame statement
of the moments and the measure of a difference between two sets of moments."""
import functools

import numpy as np

from ramannoodle_amd.spectrum import _PER_FS_TO_CM1

LATTICE = np.array([[5.0, 0.0, 0.0], [0.3, 5.2, 0.0], [0.0, -0.2, 4.9]])  # of tests/test_lineshape.py::small_trajectory
PLANTED_ATOMS, PLANTED_MODES, PLANTED_FRAMES, PLANTED_TIMESTEP = 5, 12, 2048, 1.0


@functools.lru_cache(maxsize=None)
def planted_run(seed=11):
    """A synthetic harmonic run: ``(positions[T][N][3] wrapped, masses, vectors[12][N][3], wavenumbers[12])``.  Five
    atoms with random masses in [1, 4], 12 orthonormal mass-weighted vectors orthogonal to the three translations, mode
    ``i`` making ``40 + 7 i`` cycles in T = 2048 frames of 1 fs with the amplitude ``0.3 * 40 / (40 + 7 i)`` amu^(1/2)
    Angstrom, random phases and a random origin.  Do not modify the arrays: they are shared."""
    rng = np.random.default_rng(seed)
    atoms, modes, frames = PLANTED_ATOMS, PLANTED_MODES, PLANTED_FRAMES
    masses = rng.uniform(1.0, 4.0, atoms)
    columns = 3 * atoms
    translations = (np.sqrt(masses / masses.sum())[:, None, None] * np.eye(3)[None]).reshape(columns, 3)
    basis, _ = np.linalg.qr(np.concatenate([translations, rng.normal(size=(columns, columns))], axis=1))
    vectors = basis[:, 3:3 + modes].T  # orthonormal, orthogonal to the translations (the first three columns)
    cycles = 40 + 7 * np.arange(modes)
    amplitudes = 0.3 * 40 / cycles
    phases = rng.uniform(0.0, 2.0 * np.pi, modes)
    t = np.arange(frames)
    amplitude_ts = amplitudes[:, None] * np.cos(2.0 * np.pi * cycles[:, None] * t[None] / frames + phases[:, None])
    cartesian = (amplitude_ts.T @ vectors).reshape(frames, atoms, 3) / np.sqrt(masses)[None, :, None]
    positions = (cartesian @ np.linalg.inv(LATTICE) + rng.random((atoms, 3))) % 1.0
    wavenumbers = cycles / (frames * PLANTED_TIMESTEP) * _PER_FS_TO_CM1
    for array in (positions, masses, vectors, wavenumbers):
        array.setflags(write=False)
    return positions, masses, vectors.reshape(modes, atoms, 3), wavenumbers


def face_frames(atoms, frames, seed, spread=0.01):
    """Wrapped positions ``[frames][atoms][3]`` of atoms that jitter by ``spread`` about sites of which every third
    coordinate lies within 0.005 of a cell face, so that the wrapped values sit on both sides of it and the minimum image
    acts in the displacements and in the steps."""
    rng = np.random.default_rng(seed)
    sites = rng.random((atoms, 3))
    sites.reshape(-1)[::3] = rng.uniform(-0.005, 0.005, size=len(sites.reshape(-1)[::3]))
    return (sites[None] + spread * rng.uniform(-1.0, 1.0, size=(frames, atoms, 3))) % 1.0


def brute_force_moments(positions, anchor, bounds, joined):
    """The definition, frame by frame: ``(first, second, counts)`` as ``moments_host`` returns them."""
    x = np.asarray(positions, dtype=np.float64).reshape(len(positions), -1)
    a = np.asarray(anchor, dtype=np.float64).reshape(-1)
    blocks, columns = len(joined), x.shape[1]
    first = np.zeros((blocks, columns))
    second = np.zeros((blocks, 2, columns, columns))
    counts = np.zeros((blocks, 2), dtype=np.int64)
    for b in range(blocks):
        last = bounds[b + 1] - 1
        for t in range(bounds[b], bounds[b + 1]):
            w = x[t] - a - np.rint(x[t] - a)
            first[b] += w
            second[b, 0] += np.outer(w, w)
            counts[b, 0] += 1
            if t < last or joined[b]:
                s = x[t + 1] - x[t] - np.rint(x[t + 1] - x[t])
                second[b, 1] += np.outer(s, s)
                counts[b, 1] += 1
    return first, second, counts


def moment_differences(got, want):
    """``(first, second)``: the largest difference of ``first`` relative to sqrt(frames x the largest entry of the
    block's displacement matrix), the Cauchy-Schwarz bound of a sum of displacements, and of each ``second`` matrix
    relative to its largest entry (a zero matrix must be matched exactly); the counts must agree."""
    np.testing.assert_array_equal(got[2], want[2])
    worst_first = worst_second = 0.0
    for b in range(len(want[0])):
        scale = np.sqrt(np.abs(want[1][b, 0]).max() * want[2][b, 0])  # sqrt(max sum w^2 * frames) >= max |sum w|
        difference = np.abs(got[0][b] - want[0][b]).max()
        worst_first = max(worst_first, difference / scale if scale > 0 else (0.0 if difference == 0 else np.inf))
        for s in range(2):
            scale = np.abs(want[1][b, s]).max()
            difference = np.abs(got[1][b, s] - want[1][b, s]).max()
            worst_second = max(worst_second, difference / scale if scale > 0 else (0.0 if difference == 0 else np.inf))
    return worst_first, worst_second
