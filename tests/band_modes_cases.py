"""What the band-mode GPU tests and tools/band_modes_timing.py share (tests/test_band_modes_gpu.py): the device cases,
the weight sets of a case, the measure of a difference between two sets of moments and the workspace arithmetic of
include/rn_bandmodes.h."""
import functools

import numpy as np

from ramannoodle_amd.bandmodes import band_moments_host
from ramannoodle_amd.spectrum import _segment_starts, segment_plan
from tests.quasiharmonic_cases import LATTICE, face_frames

TIME_TILE = 16    # times per k-tile of band_transform_kernel (csrc/kernels_band.hip, kSteps)
TILE = 64         # rows and columns per tile of both kernels
CHUNK_ROWS = 512  # rows of V per chunk of the update (csrc/kernels.hpp, kBandChunkRows)

# name: (atoms, W, starts or "hann": seven overlapping Hann segments).  W - 1 = n steps: 15 .. 17 and 31 .. 33 lie about
# one and two time tiles; 60 / 66, 123 / 129 and 129 / 135 columns lie about one and two column tiles.
CASES = {
    "1 atom, W = 3 (no bin)": (1, 3, [0]),
    "5 atoms, W = 18": (5, 18, [0]),
    "20 atoms, W = 34, 2 segments": (20, 34, [0, 5]),
    "41 atoms, W = 40, 3 segments": (41, 40, [0, 7, 20]),
    "43 atoms, W = 40": (43, 40, [0]),
    "5 atoms, n = 15": (5, TIME_TILE, [1]),
    "5 atoms, n = 16": (5, TIME_TILE + 1, [0]),
    "5 atoms, n = 31": (5, 2 * TIME_TILE, [0]),
    "5 atoms, n = 32": (5, 2 * TIME_TILE + 1, [2]),
    "5 atoms, n = 33": (5, 2 * TIME_TILE + 2, [0]),
    "5 atoms, 7 Hann segments of 160": (5, 160, "hann"),
}
PHASE_CASE = "1 atom, W = 20002"


@functools.lru_cache(maxsize=None)
def device_case(name):
    """``(positions, masses, alpha, W, starts, taper)`` of a case: atoms on the cell faces (``face_frames``), masses in
    [1, 100], a random-walk polarizability that is not symmetric, a random taper in [0.5, 1.5] (or the Hann taper of
    ``segment_plan``).  Do not modify the arrays: they are shared."""
    if name == PHASE_CASE:
        atoms, width, starts = 1, 20002, [0]
    else:
        atoms, width, starts = CASES[name]
    rng = np.random.default_rng(sum(name.encode()))
    if starts == "hann":
        frames = width + 6 * (width // 2)
        width, hop, taper = segment_plan(frames, width, None, "hann")
        starts = _segment_starts(frames, width, hop)
        assert len(starts) == 7
    else:
        frames = width + max(starts) + 1  # (one frame more than the segments read)
        taper = rng.uniform(0.5, 1.5, width - 1)
    positions = face_frames(atoms, frames, seed=atoms + width)
    masses = rng.uniform(1.0, 100.0, atoms)
    alpha = np.cumsum(0.01 * rng.normal(size=(frames, 3, 3)), axis=0) + rng.normal(size=(3, 3))
    starts = np.asarray(starts, dtype=np.int64)
    for array in (positions, masses, alpha, starts, taper):
        array.setflags(write=False)
    return positions, masses, alpha, width, starts, taper


def weight_sets(bins: int):
    """name -> ``bw[B][bins]`` of a case with ``bins`` bins: one bin only (the first; the last), 16 and 17 bins (32 and
    34 rows of the transform: half a row tile and two more), three overlapping bands with weights that are not 0 / 1,
    and two rows over every bin (past one row tile of 64 once ``bins > 32``)."""
    if bins == 0:
        return {"no bin": np.zeros((1, 0))}
    rng = np.random.default_rng(bins)
    sets = {"the first bin": np.eye(bins)[:1], "the last bin": np.eye(bins)[-1:]}
    for count in (16, 17):
        if bins >= count:
            sets[f"{count} bins"] = (np.arange(bins) < count).astype(np.float64)[None]
    if bins >= 3:
        bands = np.zeros((3, bins))
        for row, (lo, hi) in enumerate(((0, -(-2 * bins // 3)), (bins // 3, bins), (bins // 4, -(-3 * bins // 4)))):
            bands[row, lo:hi] = rng.uniform(0.2, 2.0, hi - lo)
        sets["three overlapping bands"] = bands
    sets["every bin, two rows"] = rng.uniform(0.2, 2.0, (2, bins))
    return sets


@functools.lru_cache(maxsize=None)
def host_moments(name, with_alpha, weights_name):
    """``band_moments_host`` of a case and one of its weight sets, computed once."""
    positions, masses, alpha, width, starts, taper = device_case(name)
    weights = weight_sets((width - 1 + 1) // 2 - 1)[weights_name]
    want = band_moments_host(positions, LATTICE, masses, alpha if with_alpha else None, width, starts, taper, weights)
    want.setflags(write=False)
    return want


def moment_error(got, want) -> float:
    """The largest ``|got - want|[j][l] / sqrt(want[j][j] want[l][l])`` over all matrices: the matrices are positive
    semi-definite, so the scale bounds every entry and no block hides behind a larger one.  Where the scale is zero
    (a zero diagonal entry) the entry must be matched exactly: ``inf`` otherwise."""
    worst = 0.0
    for mine, theirs in zip(got, want):
        diagonal = np.diag(theirs)
        assert np.all(diagonal >= 0)
        scale = np.sqrt(np.outer(diagonal, diagonal))
        difference = np.abs(mine - theirs)
        dead = scale == 0
        if np.any(difference[dead] != 0):
            return np.inf
        if np.any(~dead):
            worst = max(worst, float((difference[~dead] / scale[~dead]).max()))
    return worst


def workspace_bytes(steps, columns, rows, active_bins, segments_per_block):
    """What ``workspace_limit`` counts (include/rn_bandmodes.h, "Workspace") for ``rows`` weight rows with
    ``active_bins`` bins that have a weight, ``columns`` = K' and blocks of ``segments_per_block`` segments."""
    padded_rows = -(-2 * active_bins // TILE) * TILE
    padded_columns = -(-columns // TILE) * TILE
    tiles = padded_columns // TILE
    pairs = tiles * (tiles + 1) // 2
    fixed = steps * 16 + padded_rows * 4 + rows * padded_rows * 8 + rows * columns * columns * 8
    transforms = segments_per_block * padded_rows * padded_columns * 8
    chunks = -(-segments_per_block * padded_rows // CHUNK_ROWS)
    return fixed + transforms + chunks * rows * pairs * TILE * TILE * 8
