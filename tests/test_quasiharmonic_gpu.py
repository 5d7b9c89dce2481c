"""The covariance moments of quasi-harmonic mode analysis on the GPU (``include/rn_quasiharmonic.h``) against the host
statement ``moments_host``, their determinism, and ``get_quasiharmonic_modes(on_device=True)`` end to end.

Tolerances.  The device sums the same products in another order (chunks of ``rn_qh_chunk_frames()`` frames, k-tiles of
16, the matrix instruction's own order of four), so it differs from the host by rounding alone.  The project's rule for
sum-order differences: 20 x the worst difference measured over the shapes of this file, which profiles/quasiharmonic_modes.txt
records (each ``second`` matrix relative to its largest entry: 1.774e-15; ``first`` relative to sqrt(frames x the largest
entry of the displacement matrix), the Cauchy-Schwarz bound of a sum of displacements: 1.359e-15)."""
import functools

import numpy as np
import pytest
import torch

from ramannoodle_amd.dynamics import Trajectory, TrajectoryEnsemble
from ramannoodle_amd.quasiharmonic import chunk_frames, moments_device, moments_host, pool_moments
from tests.quasiharmonic_cases import (LATTICE, PLANTED_MODES, PLANTED_TIMESTEP, face_frames, moment_differences,
                                       planted_run)

pytestmark = pytest.mark.gpu

TOLERANCE_SECOND = 20 * 1.774e-15
TOLERANCE_FIRST = 20 * 1.359e-15

# name: (atoms, frames, bounds, joined, anchor); frames and bounds may count from the chunk length c; anchor: a frame
# index, or None for a structure of its own
CASES = {
    "two frames of one atom": (1, 2, [0, 2], [0], 0),
    "17 frames": (5, 17, [0, 17], [0], 0),
    "66 columns, two blocks": (22, 33, [0, 16, 33], [1, 0], 0),
    "129 columns, a chunk and a frame, three blocks": (43, "c+1", [0, 17, "c-1", "c+1"], [1, 1, 0], 0),
    "a chunk less a frame": (5, "c-1", [0, "c-1"], [0], 0),
    "a chunk": (5, "c", [0, "c"], [0], 0),
    "a chunk and a frame": (5, "c+1", [0, "c+1"], [0], 0),
    "a one-frame block": (5, 40, [0, 13, 14, 40], [1, 1, 0], 0),
    "a one-frame block without a step": (5, 40, [0, 13, 14, 40], [1, 0, 0], 0),
    "a middle block that is not joined": (5, 40, [0, 10, 25, 40], [1, 0, 0], 0),
    "an anchor of its own": (5, 40, [0, 20, 40], [1, 0], None),
    "an anchor from the middle": (7, 23, [0, 23], [0], 11),
}


def _resolve(value):
    if isinstance(value, str):
        c = chunk_frames()
        return {"c-1": c - 1, "c": c, "c+1": c + 1}[value]
    return value


@functools.lru_cache(maxsize=None)
def _case(name):
    """``(positions, anchor, bounds, joined, moments_host(...))``, computed once; atoms on the cell faces in every case"""
    atoms, frames, bounds, joined, anchor = CASES[name]
    frames, bounds = _resolve(frames), [_resolve(b) for b in bounds]
    positions = face_frames(atoms, frames, seed=len(name))
    if anchor is None:
        anchor = (positions[5] + 0.004) % 1.0
    else:
        anchor = positions[anchor]
    want = moments_host(positions, anchor, bounds, joined)
    for array in (positions, *want):
        array.setflags(write=False)
    return positions, anchor, bounds, joined, want


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(CASES))
def test_moments_agree_with_the_host_statement(name):
    positions, anchor, bounds, joined, want = _case(name)
    from_host = moments_device(positions, anchor, bounds, joined)
    tensor = torch.tensor(positions, dtype=torch.float64, device="cuda")
    from_hbm = moments_device(tensor, anchor, bounds, joined)
    first, second = moment_differences(from_host, want)
    print(f"{name}: first {first:.2e}, second {second:.2e}")
    assert second <= TOLERANCE_SECOND and first <= TOLERANCE_FIRST
    # determinism: both entries agree bit for bit, a repeated call is bit-identical, the matrices are symmetric
    assert _same(from_host, from_hbm)
    assert _same(moments_device(tensor, anchor, bounds, joined), from_hbm)
    assert _same(moments_device(positions, anchor, bounds, joined), from_host)
    np.testing.assert_array_equal(from_hbm[1], from_hbm[1].transpose(0, 1, 3, 2))
    if name == "a one-frame block without a step":
        assert not from_hbm[1][1, 1].any() and from_hbm[1][1, 0].any()


def test_other_blocks_change_the_pooled_sums_within_the_tolerance():
    positions, anchor, bounds, joined, want = _case("a chunk and a frame")
    frames = bounds[-1]
    pooled_want = [array[None] for array in pool_moments(*want)]
    for cut in ([0, frames], [0, 100, 300, frames], [0, 1, frames - 1, frames], [0, 16, 32, 48, frames]):
        flags = [1] * (len(cut) - 2) + [0]
        pooled = [array[None] for array in pool_moments(*moments_device(positions, anchor, cut, flags))]
        first, second = moment_differences(pooled, pooled_want)
        print(f"blocks {cut}: first {first:.2e}, second {second:.2e}")
        assert second <= TOLERANCE_SECOND and first <= TOLERANCE_FIRST


def _overlaps(a, b):
    return np.abs(np.einsum("mk,mk->m", a.reshape(len(a), -1), b.reshape(len(b), -1)))


@pytest.mark.parametrize("ensemble", [False, True])
def test_modes_on_the_device_are_the_modes_on_the_host(ensemble):
    positions, masses, _, _ = planted_run()
    if ensemble:
        run = TrajectoryEnsemble([Trajectory(positions, PLANTED_TIMESTEP), Trajectory(positions[::-1], PLANTED_TIMESTEP)])
        arguments = dict(blocks=2, temperature=300.0)
    else:
        run = Trajectory(positions, PLANTED_TIMESTEP)
        arguments = {}
    want = run.get_quasiharmonic_modes(LATTICE, masses, **arguments)
    got = run.get_quasiharmonic_modes(LATTICE, masses, on_device=True, **arguments)
    assert got.rank == want.rank == PLANTED_MODES
    np.testing.assert_array_equal(got.counts, want.counts)
    np.testing.assert_allclose(got.wavenumbers_steps, want.wavenumbers_steps, rtol=1e-9)
    np.testing.assert_allclose(got.phonons.wavenumbers, want.phonons.wavenumbers, rtol=1e-9)
    np.testing.assert_allclose(got.block_wavenumbers, want.block_wavenumbers, rtol=1e-9)
    assert _overlaps(got.vectors, want.vectors).min() >= 1.0 - 1e-9
    np.testing.assert_allclose(got.mean_positions, want.mean_positions, rtol=0, atol=1e-12)
