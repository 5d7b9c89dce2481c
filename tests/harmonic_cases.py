"""What the harmonic-trajectory tests share (tests/test_harmonic_trajectory.py, tests/test_harmonic_trajectory_gpu.py,
tools/harmonic_trajectory_timing.py): phonons with planted modes, raw inputs of the synthesis near the cell faces, the
named device cases and the bound of a device-minus-host difference."""
import functools

import numpy as np

from ramannoodle_amd.dynamics import Phonons
from ramannoodle_amd.spectrum import _PER_FS_TO_CM1
from tests.quasiharmonic_cases import LATTICE, PLANTED_ATOMS, PLANTED_FRAMES, PLANTED_MODES, PLANTED_TIMESTEP

MAX_REACH = 0.05  # the largest s_j = max_r sum_m |amp[r][m] D[m][j]| of a device case


def face_sites(atoms, rng):
    """Reference sites ``(atoms,3)`` of which every third coordinate lies within 0.002 of a cell face, so that the wrap
    acts: the moving atom sits on both sides of it."""
    sites = rng.random((atoms, 3))
    flat = sites.reshape(-1)
    flat[::3] = rng.uniform(-0.002, 0.002, size=len(flat[::3])) % 1.0
    return sites


def mode_basis(masses, modes, rng):
    """``modes`` orthonormal mass-weighted vectors ``(modes,N,3)`` orthogonal to the three translations."""
    columns = 3 * len(masses)
    translations = (np.sqrt(masses / masses.sum())[:, None, None] * np.eye(3)[None]).reshape(columns, 3)
    basis, _ = np.linalg.qr(np.concatenate([translations, rng.normal(size=(columns, columns))], axis=1))
    return basis[:, 3:3 + modes].T.reshape(modes, len(masses), 3)


def phonons_of(vectors, masses, wavenumbers, lattice, rng):
    """A ``Phonons`` about face sites whose fractional displacements are the mass-weighted ``vectors`` divided by
    sqrt(mass), taken to fractional coordinates and given arbitrary norms (a mode's norm carries no meaning)."""
    norms = rng.uniform(0.2, 3.0, len(vectors))
    displacements = (vectors / np.sqrt(masses)[None, :, None]) @ np.linalg.inv(lattice) * norms[:, None, None]
    return Phonons(face_sites(len(masses), rng), np.array(wavenumbers, dtype=np.float64), np.ascontiguousarray(displacements))


@functools.lru_cache(maxsize=None)
def planted_phonons(seed=5):
    """``(phonons, masses, vectors[12][5][3], wavenumbers[12])``: five atoms with random masses in [1, 4], 12 planted modes,
    mode ``i`` making ``40 + 7 i`` cycles in 2048 frames of 1 fs.  Do not modify the arrays: they are shared."""
    rng = np.random.default_rng(seed)
    masses = rng.uniform(1.0, 4.0, PLANTED_ATOMS)
    vectors = mode_basis(masses, PLANTED_MODES, rng)
    wavenumbers = (40 + 7 * np.arange(PLANTED_MODES)) / (PLANTED_FRAMES * PLANTED_TIMESTEP) * _PER_FS_TO_CM1
    phonons = phonons_of(vectors, masses, wavenumbers, LATTICE, rng)
    for array in (masses, vectors, wavenumbers):
        array.setflags(write=False)
    return phonons, masses, vectors, wavenumbers


def raw_inputs(atoms, modes, runs, seed):
    """``(ref[N][3], D[M][3N], omega_dt[M], amp[R][M], phase[R][M])`` of the definition: face sites, random displacements
    and amplitudes scaled so that the largest reach ``s_j`` is ``MAX_REACH``, angles per frame in (0.01, 3), phases in
    [0, 2 pi)."""
    rng = np.random.default_rng(seed)
    ref = face_sites(atoms, rng)
    D = rng.normal(size=(modes, 3 * atoms))
    amp = rng.uniform(0.2, 1.0, size=(runs, modes))
    D *= MAX_REACH / reach(amp, D).max()
    omega_dt = rng.uniform(0.01, 3.0, modes)
    phase = rng.uniform(0.0, 2.0 * np.pi, size=(runs, modes))
    return ref, D, omega_dt, amp, phase


def reach(amp, D):
    """``s_j = max_r sum_m |amp[r][m] D[m][j]|`` per column: the farthest a coordinate can move."""
    D = np.asarray(D).reshape(len(D), -1)
    return (np.abs(np.atleast_2d(amp))[:, :, None] * np.abs(D)[None]).sum(axis=1).max(axis=0)


def difference_bound(amp, D):
    """The bound per column of the device-minus-host difference after the minimum image: ``2 (M + 8) 2^-52 s_j + 2^-50``.
    On each side every term carries a cosine of at most 2 ulp on an identical argument and two products, the M terms are
    summed in any order, then come one addition to a value of order one and the wrap."""
    modes = len(np.asarray(D))
    return 2.0 * (modes + 8) * 2.0 ** -52 * reach(amp, D) + 2.0 ** -50


def minimum_image(difference):
    """``d - rint(d)``: a value at a face may wrap to either side."""
    return difference - np.rint(difference)


# name: (atoms, modes, frames, runs, first frame); "3N" modes: as many as columns
DEVICE_CASES = {
    "one of everything": (1, 1, 1, 1, 0),
    "one atom, 3N modes, 15 frames, three runs": (1, "3N", 15, 3, 7),
    "four modes, 16 frames": (5, 4, 16, 1, 0),
    "five modes, 17 frames, three runs, far out": (5, 5, 17, 3, 2 ** 40),
    "3N = 15 modes, 33 frames": (5, "3N", 33, 1, 7),
    "66 columns, 17 modes, 257 frames": (22, 17, 257, 1, 0),
    "66 columns, 33 modes, 33 frames, three runs": (22, 33, 33, 3, 7),
    "66 columns, 3N modes, 17 frames, far out": (22, "3N", 17, 1, 2 ** 40),
    "129 columns, one mode, 257 frames, three runs": (43, 1, 257, 3, 0),
    "129 columns, 17 modes, 16 frames, far out": (43, 17, 16, 1, 2 ** 40),
    "129 columns, 33 modes, 15 frames, three runs": (43, 33, 15, 3, 7),
    "129 columns, 3N modes, 257 frames": (43, "3N", 257, 1, 0),
}


def device_case(name):
    """``(inputs of raw_inputs, frames, first frame)`` of a named case."""
    atoms, modes, frames, runs, first = DEVICE_CASES[name]
    modes = 3 * atoms if modes == "3N" else modes
    return raw_inputs(atoms, modes, runs, seed=len(name) + 100 * atoms + modes), frames, first
