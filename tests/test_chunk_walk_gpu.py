"""The chunk walk both models' increment entries share (csrc/increments.hpp: walk_chunks), at the chunkings where the
loop can go wrong: one step in one chunk, a carry before every chunk, a short last chunk, and no carry at all (as many
steps per chunk as there are, and more).  Group and mode increments, with and without the rest channel, and for PotGNN
with a lattice per frame as well, so that the lattice rows are carried too.

The interpolation model's steps per chunk F are forced exactly through the workspace limit, and every chunking equals
the unchunked result byte for byte.  PotGNN's F is not read: the smallest power-of-two limit that is not refused holds
one step per chunk, twice that two or three, eight times that at least eight; its reverse pass accumulates with
atomics, so chunkings agree with the unchunked result to round-off, within test_repeat_and_chunking_agree's bars.
Needs a real MI355X: run with ``-m gpu``."""
import functools

import numpy as np
import pytest
import torch

from ramannoodle_amd.spectrum import mode_projectors
from tests.conftest import load_golden
from tests.helpers import product_model_from_golden
from tests.interp_cases import fixture

pytestmark = pytest.mark.gpu

FRAMES = 6
GRID = [(1, 1), (3, 1), (5, 2), (5, 5), (5, 8)]  # (steps, steps per chunk)
ENTRIES = ("group", "modes", "modes and rest")
TOLERANCE = {True: 1e-12, False: 1e-5}  # float64, float32: the bars of test_repeat_and_chunking_agree


@pytest.fixture(autouse=True)
def _no_default_device_mode():
    torch.set_default_device(None)
    yield


def _cuda(array):
    return torch.tensor(np.ascontiguousarray(array), dtype=torch.float64, device="cuda:0")


def _err(got, want):
    return np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)


def _modes(lattice, atoms, seed):
    rng = np.random.default_rng(seed)
    return mode_projectors(rng.normal(size=(3, atoms, 3)) * 0.05, lattice, np.ones(atoms))


def _run(model, entry, positions, modes, **options):
    if entry == "group":
        out = model.calc_group_increments_device(positions, "species", **options)
    else:
        out = model.calc_mode_increments_device(positions, modes[0], modes[1], rest=entry == "modes and rest", **options)
    return out.cpu().numpy()


# ----------------------------------------------------------------------------- the interpolation model
@functools.lru_cache(maxsize=None)
def _interp():
    case, g = fixture("interp_p1_small")
    return case.model(), _cuda(g["positions"][:FRAMES]), _modes(case.lattice, len(case.ref_positions), 45)


@functools.lru_cache(maxsize=None)
def _interp_whole(entry, steps):
    model, positions, modes = _interp()
    return _run(model, entry, positions[:steps + 1], modes)


def _interp_chunkings_are_bit_equal(steps, per_chunk):
    model, positions, modes = _interp()
    rows = 6 * 3 * model.num_atoms * 8
    per, carry = rows + 6 * model.num_dofs * 8, rows
    for entry in ENTRIES:
        limit = carry + per_chunk * per + (0 if entry == "group" else 2 * modes[0].nbytes)
        chunked = _run(model, entry, positions[:steps + 1], modes, workspace_limit=limit)
        np.testing.assert_array_equal(chunked, _interp_whole(entry, steps), err_msg=entry)


# ----------------------------------------------------------------------------- PotGNN
@functools.lru_cache(maxsize=None)
def _potgnn():
    g = load_golden("triclinic20")
    model = product_model_from_golden(g).eval()
    rng = np.random.default_rng(46)
    lattices = g["lattice"][None] * (1.0 + 0.002 * rng.normal(size=(FRAMES, 3, 3)))  # a cell that breathes and shears
    return model, _cuda(g["md/positions"][:FRAMES]), _cuda(lattices), _modes(g["lattice"], model.num_atoms, 47)


def _potgnn_run(entry, steps, float64, cells, **options):
    model, positions, lattices, modes = _potgnn()
    return _run(model, entry, positions[:steps + 1], modes, float64=float64,
                lattices=lattices[:steps + 1] if cells else None, **options)


@functools.lru_cache(maxsize=None)
def _potgnn_whole(entry, steps, float64, cells):
    return _potgnn_run(entry, steps, float64, cells)


@functools.lru_cache(maxsize=None)
def _one_step_limit(entry, float64, cells):
    """The smallest power-of-two workspace limit the entry does not refuse: one step per chunk."""
    limit = 1 << 16
    while True:
        try:
            _potgnn_run(entry, 1, float64, cells, workspace_limit=limit)
            return limit
        except MemoryError:
            limit <<= 1
            assert limit <= 1 << 32


def _potgnn_chunkings_agree_to_round_off(steps, per_chunk, float64, cells):
    multiple = {1: 1, 2: 2, 5: 8, 8: 16}[per_chunk]  # of the one-step limit: 1, 2..3, >= 8, >= 16 steps per chunk
    for entry in ENTRIES:
        whole = _potgnn_whole(entry, steps, float64, cells)
        channels = {"group": 3, "modes": 3, "modes and rest": 4}[entry] + cells  # (three species)
        assert whole.shape == (steps, channels, 3, 3) and np.all(np.isfinite(whole))
        limit = multiple * _one_step_limit(entry, float64, cells)
        chunked = _potgnn_run(entry, steps, float64, cells, workspace_limit=limit)
        error = _err(chunked, whole)
        print(f"{entry}, {steps} steps, {multiple} x the one-step limit: {error:.2e}")
        assert error < TOLERANCE[float64], entry


@pytest.mark.parametrize("steps,per_chunk", GRID)
@pytest.mark.parametrize("which", ["interpolation", "potgnn"])
def test_chunkings_agree_with_the_unchunked_result(which, steps, per_chunk):
    if which == "interpolation":
        _interp_chunkings_are_bit_equal(steps, per_chunk)
        return
    for float64 in (True, False):
        for cells in (False, True):  # (a lattice per frame: the lattice rows are carried too)
            _potgnn_chunkings_agree_to_round_off(steps, per_chunk, float64, cells)
