"""The kernels beside the EdgeBlock and the NodeBlock that mainly move bytes -- the pair kernel (csrc/kernels_c2_pairs.hip),
the node projections (csrc/kernels_gemm.hip: rowgemm_split_kernel) and the geometry kernel (csrc/kernels_agg.hip:
geom_rbf_pairs_kernel) -- at the smallest shapes at which their tiling can go wrong:

1. pair tiles (16 rows) that hold rows of two frames, and a last tile that is not full;
2. more pair tiles than the pair kernel's grid holds at once, so that every wave of it walks several;
3. node projections whose row count is no multiple of the 16-row tile;
4. geometry blocks (256 edges) that end inside a frame, the last one not full, and the padded columns of its rows.

Fixtures and bounds are those of tests/helpers.py, tests/test_sparse_graphs_gpu.py and tests/test_c2_pairs_gpu.py.
Needs a real MI355X: run with ``-m gpu``.
"""
import functools

import numpy as np
import pytest
import torch

from ramannoodle_amd import _lib
from tests.helpers import SPARSE_PROPERTIES
from tests.test_c2_pairs_gpu import PASSES, WIDTHS, _build
from tests.test_gpu_parity import REL, _rel_err
from tests.test_pair_table import _pairs
from tests.test_sparse_graphs_gpu import _standardised

pytestmark = pytest.mark.gpu

PAIR_TILE = 16    # rows of a pair-kernel tile and of a projection tile
GEOM_BLOCK = 256  # edges of a geometry workgroup


def _num_pairs(model):
    """NP of the model's graph, from the planner (``rn_potgnn_debug_plan_pairs``)."""
    ea, eb = (np.ascontiguousarray(x, dtype=np.int32) for x in model.ref_edge_indexes[1:3])
    types = np.ascontiguousarray(model.atom_type_map[np.asarray(model._ref_structure.atomic_numbers)], dtype=np.int32)
    shape = (model.num_atoms, model.num_edges, int(model._num_atom_types), 64, 64)
    return _pairs(_lib.load(), shape, ea, eb, types)[0]


@functools.lru_cache(maxsize=None)
def _oracle64_alpha(name, fn, fe, frames):
    from oracle import potgnn_oracle as O
    g, _, oracle = _build(name, fn, fe, frames)
    oracle64 = oracle.to(torch.float64)
    want = O.calc_polarizabilities(oracle64, g["pos_batch"], faithful=False)
    want.setflags(write=False)
    return want, oracle64


# ----------------------------------------------------------------------------- 1. pair tiles that straddle frames
@pytest.mark.parametrize("fn, fe", WIDTHS)
@pytest.mark.parametrize("name", ["hub17", "molecules33"])
def test_pair_tiles_that_straddle_frames(monkeypatch, name, fn, fe):
    """Five frames on pair rows (``RN_POTGNN_NODE_ATOM=1``): NP is 41 / 22, so every frame after the first starts inside a
    16-row tile and the last tile is not full.  EVERY frame evaluated alone is bit-identical to that frame in the batch, a
    second evaluation is bit-identical, and the standardised output is within the suite's ``REL`` of the float64 oracle."""
    monkeypatch.setenv("RN_POTGNN_NODE_ATOM", "1")
    frames = 5
    g, model, _ = _build(name, fn, fe, frames)
    num_pairs = _num_pairs(model)
    assert num_pairs == SPARSE_PROPERTIES[name]["E"] // 2
    assert (frames * num_pairs) % PAIR_TILE != 0, "the last tile must not be full"
    starts = [(s * num_pairs) % PAIR_TILE for s in range(1, frames)]
    assert all(starts), ("every later frame must start inside a tile", starts)
    pos = g["pos_batch"]
    want, oracle64 = _oracle64_alpha(name, fn, fe, frames)
    got = model.calc_polarizabilities(pos)
    flags = model.config_flags()
    assert flags["split_f16_pair_rows"] and flags["c2_per_atom_pair"], flags
    err = _rel_err(_standardised(got, oracle64), _standardised(want, oracle64))
    print(f"straddling pair tiles {name} {fn}/{fe}: NP {num_pairs}, frame starts mod 16 {starts}, device f32 vs oracle f64 {err:.2e}")
    assert err < REL, (name, fn, fe, err)
    model.set_profiling(1)
    np.testing.assert_array_equal(model.calc_polarizabilities(pos), got)
    assert model.kernel_times()["c2_pairs"][1] == PASSES
    model.set_profiling(0)
    for s in range(frames):
        np.testing.assert_array_equal(model.calc_polarizabilities(pos[s:s + 1])[0], got[s], err_msg=f"frame {s} alone")


# ----------------------------------------------------------------------------- 2. more tiles than the grid holds
def test_more_pair_tiles_than_the_grid_holds():
    """The benchmark's kind of cell (64 atoms, NP = 576: 36 tiles per frame) with enough frames that every wave of the pair
    kernel's grid (``launch_c2_pairs``: at most two workgroups of four waves per CU, a wave per tile) walks two tiles and
    a quarter of them a third, each with the next tile's rows requested under the current one's arithmetic (nine of this
    test's ten seconds are the CPU oracle of the whole batch: more rounds would only add to them).  The first, a middle and the
    last frame alone are bit-identical to the batch; the whole batch is within 1e-5 of the oracle, as in ``smoke()``."""
    from bench import make_workload
    from oracle import potgnn_oracle as O
    tiles_at_once = 2 * torch.cuda.get_device_properties(0).multi_processor_count * 4
    probe = make_workload(num_cells=(2, 2, 2), frames=1, hparams="perf", seed=5)["model"]()
    num_pairs = _num_pairs(probe)
    assert num_pairs == 576 and num_pairs % PAIR_TILE == 0
    per_frame = num_pairs // PAIR_TILE
    frames = -(-9 * tiles_at_once // (4 * per_frame))
    assert 4 * frames * per_frame >= 9 * tiles_at_once, (frames, per_frame, tiles_at_once)
    wl = make_workload(num_cells=(2, 2, 2), frames=frames, hparams="perf", seed=5)
    model = wl["model"](device=0)
    pos = wl["positions"]
    got = model.calc_polarizabilities(pos)
    flags = model.config_flags()
    assert flags["split_f16_pair_rows"] and flags["c2_per_atom_pair"], flags
    want = O.calc_polarizabilities(wl["oracle"](), pos, faithful=False)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{frames} frames x {per_frame} pair tiles, {tiles_at_once} tiles at once: max rel err vs oracle {err:.2e}")
    assert err < 1e-5, err
    for s in (0, frames // 2, frames - 1):
        np.testing.assert_array_equal(model.calc_polarizabilities(pos[s:s + 1])[0], got[s], err_msg=f"frame {s} alone")


# ----------------------------------------------------------------------------- 3. and 4. stages at tails
def _stages(monkeypatch, name, fn, fe, frames):
    """One forward on pair rows with snapshots (``RN_POTGNN_KEEP_STAGES=2``): (fixture dict, model, float32 oracle stages)."""
    from oracle import potgnn_oracle as O
    monkeypatch.setenv("RN_POTGNN_KEEP_STAGES", "2")
    monkeypatch.setenv("RN_POTGNN_NODE_ATOM", "1")
    g, model, oracle = _build(name, fn, fe, frames)
    pos = g["pos_batch"]
    s = pos.shape[0]
    model.eval()
    model.forward(torch.tensor(g["lattice"]).expand(s, 3, 3), torch.tensor(g["atomic_numbers"]).expand(s, -1), torch.tensor(pos))
    flags = model.config_flags()
    assert flags["split_f16_mfma"] and flags["split_f16_pair_rows"] and flags["atom_owning_node_block"], flags
    stages = {}
    O.forward(oracle, pos, faithful=False, stages=stages)
    return g, model, stages


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("fn, fe", WIDTHS)
def test_projection_tails(monkeypatch, fn, fe, frames):
    """``hub17``, one frame and three: 17 and 51 node rows, so the projections' last 16-row tile holds one row and three.
    Node and edge rows after each pass against the float32 oracle at atol 2e-5, as ``test_stages_on_pair_rows``."""
    assert (frames * SPARSE_PROPERTIES["hub17"]["N"]) % PAIR_TILE != 0
    _, model, stages = _stages(monkeypatch, "hub17", fn, fe, frames)
    for p in range(PASSES + 1):
        node_ref, edge_ref = stages[f"node{p}"].numpy(), stages[f"edge{p}"].numpy()
        node, edge = model.debug_stage(1, p), model.debug_stage(2, p)
        assert node.shape == node_ref.shape and edge.shape == edge_ref.shape, (p, node.shape, edge.shape)
        print(f"projection tails hub17 {fn}/{fe} x {frames} pass {p}: node {np.abs(node - node_ref).max():.2e} "
              f"edge {np.abs(edge - edge_ref).max():.2e}")
        np.testing.assert_allclose(node, node_ref, rtol=0, atol=2e-5, err_msg=f"node{p}")
        np.testing.assert_allclose(edge, edge_ref, rtol=0, atol=2e-5, err_msg=f"edge{p}")


@pytest.mark.parametrize("fn, fe", WIDTHS)
@pytest.mark.parametrize("name, frames", [("hub17", 5), ("molecules33", 7)])
def test_geometry_tails(monkeypatch, name, fn, fe, frames):
    """410 and 308 edge rows: one full 256-edge block that ends inside a frame and a last block that ends inside one of a
    wave's eight-row steps.  The stage-0 edge rows, decoded, against the oracle's ``edge0`` at atol 2e-5; in the rows as they
    lie in memory (eight f16 hi | eight f16 lo per eight columns) the columns >= Fe are exactly zero; the last frame alone
    gives bit-identical rows."""
    edges = SPARSE_PROPERTIES[name]["E"]
    total = frames * edges
    assert total > GEOM_BLOCK and total % GEOM_BLOCK != 0 and GEOM_BLOCK % edges != 0 and (total % GEOM_BLOCK) % 8 != 0
    g, model, stages = _stages(monkeypatch, name, fn, fe, frames)
    edge = model.debug_stage(2, 0)
    edge_ref = stages["edge0"].numpy()
    assert edge.shape == edge_ref.shape == (total, fe)
    print(f"geometry tails {name} {fn}/{fe} x {frames}: edge0 {np.abs(edge - edge_ref).max():.2e}")
    np.testing.assert_allclose(edge, edge_ref, rtol=0, atol=2e-5, err_msg="edge0")
    raw = model.debug_stage(4, 0)
    assert raw.shape == (total, 64)
    halves = raw.view(np.float16).reshape(total, 8, 2, 8).astype(np.float32)  # [row, group of eight columns, hi | lo, column]
    np.testing.assert_array_equal(halves.sum(axis=2).reshape(total, 64)[:, :fe], edge)
    pad = raw.view(np.uint16).reshape(total, 8, 2, 8).transpose(0, 1, 3, 2).reshape(total, 64, 2)[:, fe:]
    assert not pad.any(), "padded columns must be exact zeros, hi and lo"
    # the last frame alone: other blocks, other lanes, the same bits
    pos = g["pos_batch"][frames - 1:]
    model.forward(torch.tensor(g["lattice"]).expand(1, 3, 3), torch.tensor(g["atomic_numbers"]).expand(1, -1), torch.tensor(pos))
    np.testing.assert_array_equal(model.debug_stage(4, 0), raw[(frames - 1) * edges:])
