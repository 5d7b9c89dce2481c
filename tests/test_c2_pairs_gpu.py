"""The EdgeBlock's c2 branch once per atom pair (csrc/kernels_c2_pairs.hip + the ``C2G`` instantiation of the
role-specialised EdgeBlock), against the float64 oracle, with ``RN_POTGNN_C2_PAIRS`` on (the default) and off.

Graphs: ``hub17`` (edge-free atoms, a second 16-atom tile without rows), ``molecules33`` (destination edges without a
triplet), ``iso_dimer_iso`` (two edges, one pair), ``hub_cap64`` (a hub at the degree cap of the 64-wide kernels: the
planner gives it the unfused chain, which no knob of this file may disturb) and ``blob_gas`` (a complete 56-atom ball
among small molecules: the densest graph of tests/test_dense_graphs_gpu.py that the role-specialised EdgeBlock takes), at 64/64 and at the PAD widths 40/50, two passes; bounds and helpers are those of
tests/test_sparse_graphs_gpu.py.  Whether the pair kernel ran is read off its timer slot (``kernel_times()["c2_pairs"]``).
The pair kernel serves runs on split-f16 pair rows, which need the atom-owning NodeBlock; with in-degrees as uneven as
these graphs' the planner prefers the row-ordered one, so under default knobs most of them keep c2 inside the EdgeBlock
whatever the knob says.  Every case therefore runs a third time with ``RN_POTGNN_NODE_ATOM=1``, where the new kernels do
run on ``hub17`` and ``molecules33``; a rocksalt cell like the benchmark's takes them under default knobs.
Needs a real MI355X: run with ``-m gpu``.
"""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import DENSE_PROPERTIES, SPARSE_PROPERTIES, dense_fixture, sparse_fixture
from tests.test_gpu_parity import REL, _random_model, _rel_err
from tests.test_sparse_graphs_gpu import _standardised

pytestmark = pytest.mark.gpu

PASSES = 2
GRAPHS = ("hub17", "molecules33", "iso_dimer_iso", "hub_cap64", "blob_gas")
WIDTHS = ((64, 64), (40, 50))


def _build(name, fn, fe, frames):
    """(positions, product model, float32 oracle): built again per test, because a handle reads its knobs when it is created."""
    dense = name in DENSE_PROPERTIES
    g, cutoff = (dense_fixture if dense else sparse_fixture)(name, frames=frames)
    model, oracle = _random_model(g, cutoff, fn, fe, PASSES, seed=fn * 1000 + fe + GRAPHS.index(name))
    props = (DENSE_PROPERTIES if dense else SPARSE_PROPERTIES)[name]
    assert (model.num_atoms, model.num_edges, oracle.num_triplets) == tuple(props[k] for k in "NET")
    return g, model, oracle


@functools.lru_cache(maxsize=None)
def _reference(name, fn, fe, frames):
    """The float64 oracle's polarizabilities, mean and std of one case: computed once, shared by the knob's two values."""
    from oracle import potgnn_oracle as O
    g, _, oracle = _build(name, fn, fe, frames)
    oracle64 = oracle.to(torch.float64)
    want = O.calc_polarizabilities(oracle64, g["pos_batch"], faithful=False)
    want.setflags(write=False)
    return want, oracle64


def _check(name, fn, fe, frames, knob_on):
    g, model, _ = _build(name, fn, fe, frames)
    want, oracle64 = _reference(name, fn, fe, frames)
    pos = g["pos_batch"]
    got = model.calc_polarizabilities(pos)
    assert np.isfinite(got).all()
    err = _rel_err(_standardised(got, oracle64), _standardised(want, oracle64))
    print(f"c2 pairs {'on' if knob_on else 'off'} {name} {fn}/{fe} x {frames} frames: device f32 vs oracle f64 {err:.2e}")
    assert err < REL, (name, fn, fe, knob_on, err)
    flags = model.config_flags()
    # a second evaluation, with every launch timed: bit-identical, and the pair kernel ran once per pass -- or never
    model.set_profiling(1)
    np.testing.assert_array_equal(model.calc_polarizabilities(pos), got)
    launches = model.kernel_times()["c2_pairs"][1]
    model.set_profiling(0)
    served = flags["role_split_edge_block"] and flags["split_f16_pair_rows"] and flags["split_f16_mfma"]
    assert launches == (PASSES if knob_on and served else 0), (launches, flags)
    assert flags["c2_per_atom_pair"] == (launches > 0), (launches, flags)
    np.testing.assert_array_equal(model.calc_polarizabilities(pos[0:1])[0], got[0])
    return flags, launches


@pytest.mark.parametrize("knob, node_atom", [("1", None), ("0", None), ("1", "1")])
@pytest.mark.parametrize("fn, fe", WIDTHS)
@pytest.mark.parametrize("name", GRAPHS)
def test_parity_with_the_knob_on_and_off(monkeypatch, name, fn, fe, knob, node_atom):
    """Standardised output within the suite's ``REL`` of the float64 oracle, a second evaluation bit-identical, frame 0
    alone bit-identical to frame 0 of the batch; the role-specialised EdgeBlock is still what the handle reports, and the
    pair kernel ran exactly when the knob is on and the run is on pair rows."""
    monkeypatch.setenv("RN_POTGNN_C2_PAIRS", knob)
    if node_atom is not None:
        monkeypatch.setenv("RN_POTGNN_NODE_ATOM", node_atom)
    flags, launches = _check(name, fn, fe, 3 if name in DENSE_PROPERTIES else 5, knob == "1")
    print(f"   pair kernel launches {launches}, pair rows {flags['split_f16_pair_rows']}, atom-owning NodeBlock {flags['atom_owning_node_block']}")
    if name in ("hub17", "molecules33", "blob_gas"):
        assert flags["fused_edge_block"] and flags["role_split_edge_block"], flags
    if node_atom == "1" and name in ("hub17", "molecules33"):
        assert flags["split_f16_pair_rows"] and launches == PASSES, (flags, launches)


def test_default_knobs_take_the_pair_kernel_on_a_rocksalt_cell(monkeypatch):
    """The benchmark's kind of graph (64 atoms, 18 neighbours each, four passes) under default knobs: pair rows, so the
    pair kernel runs once per pass; the output within 1e-5 of the oracle, as in ``smoke()``."""
    from bench import make_workload
    from oracle import potgnn_oracle as O
    monkeypatch.delenv("RN_POTGNN_C2_PAIRS", raising=False)
    wl = make_workload(num_cells=(2, 2, 2), frames=6, hparams="perf", seed=5)
    model = wl["model"](device=0)
    got = model.calc_polarizabilities(wl["positions"])
    want = O.calc_polarizabilities(wl["oracle"](), wl["positions"], faithful=False)
    assert np.abs(got - want).max() / np.abs(want).max() < 1e-5
    flags = model.config_flags()
    assert flags["role_split_edge_block"] and flags["split_f16_pair_rows"], flags
    model.set_profiling(1)
    np.testing.assert_array_equal(model.calc_polarizabilities(wl["positions"]), got)
    assert model.kernel_times()["c2_pairs"][1] == wl["hparams"][2]
    model.set_profiling(0)
    np.testing.assert_array_equal(model.calc_polarizabilities(wl["positions"][0:1])[0], got[0])


@pytest.mark.parametrize("knob", ["1", "0"])
def test_more_frames_than_workgroup_slots(monkeypatch, knob):
    """``hub17`` with 300 frames on pair rows (``RN_POTGNN_NODE_ATOM=1``): the EdgeBlock's grid holds one workgroup per CU,
    so a workgroup serves two or three frames one after the other (the benchmark runs 286 per workgroup) -- its ring, its
    round counters and the pair rows of the next frame all carry over."""
    monkeypatch.setenv("RN_POTGNN_C2_PAIRS", knob)
    monkeypatch.setenv("RN_POTGNN_NODE_ATOM", "1")
    flags, launches = _check("hub17", 64, 64, 300, knob == "1")
    assert flags["role_split_edge_block"] and flags["split_f16_pair_rows"] and launches == (PASSES if knob == "1" else 0)


@pytest.mark.parametrize("knob", ["1", "0"])
@pytest.mark.parametrize("fn, fe", WIDTHS)
@pytest.mark.parametrize("name", ["hub17", "molecules33"])
def test_stages_on_pair_rows(monkeypatch, name, fn, fe, knob):
    """Node and edge rows after the embedding and after each pass against the float32 oracle, at the tolerance of
    ``test_stages_on_edge_free_atoms_and_triplet_less_edges`` (atol 2e-5), on the path the pair kernel serves.
    ``RN_POTGNN_KEEP_STAGES=1`` would put the run on float32 rows and so on the parent's kernels; ``=2`` snapshots the run
    as it is, on split-f16 pair rows, and ``debug_stage`` decodes them (x = hi + lo, exact to 2^-22 relative: 2.4e-7 for
    these tanh outputs, far inside the bound).  With the knob on the pair kernel and the ``C2G`` EdgeBlock made these rows,
    with it off the EdgeBlock alone: both meet the same bound."""
    from oracle import potgnn_oracle as O
    monkeypatch.setenv("RN_POTGNN_KEEP_STAGES", "2")
    monkeypatch.setenv("RN_POTGNN_NODE_ATOM", "1")
    monkeypatch.setenv("RN_POTGNN_C2_PAIRS", knob)
    g, model, oracle = _build(name, fn, fe, 5)
    pos = g["pos_batch"]
    s = pos.shape[0]
    model.eval()
    model.set_profiling(1)
    model.forward(torch.tensor(g["lattice"]).expand(s, 3, 3), torch.tensor(g["atomic_numbers"]).expand(s, -1), torch.tensor(pos))
    launches = model.kernel_times()["c2_pairs"][1]
    model.set_profiling(0)
    flags = model.config_flags()
    assert flags["role_split_edge_block"] and flags["split_f16_pair_rows"], flags
    assert flags["c2_per_atom_pair"] == (knob == "1") and launches == (PASSES if knob == "1" else 0), (flags, launches)
    stages = {}
    O.forward(oracle, pos, faithful=False, stages=stages)
    for p in range(PASSES + 1):
        node_ref, edge_ref = stages[f"node{p}"].numpy(), stages[f"edge{p}"].numpy()
        node, edge = model.debug_stage(1, p), model.debug_stage(2, p)
        assert node.shape == node_ref.shape and edge.shape == edge_ref.shape, (p, node.shape, edge.shape)
        print(f"stages on pair rows, c2 pairs {knob}, {name} {fn}/{fe} pass {p}: node {np.abs(node - node_ref).max():.2e} "
              f"edge {np.abs(edge - edge_ref).max():.2e}")
        np.testing.assert_allclose(node, node_ref, rtol=0, atol=2e-5, err_msg=f"node{p}")
        np.testing.assert_allclose(edge, edge_ref, rtol=0, atol=2e-5, err_msg=f"edge{p}")
