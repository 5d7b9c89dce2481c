"""The planner's atom-pair table (``GraphPlan::pair_of_edge`` / ``pair_a`` / ``pair_b``), host-only.

Edge d and its reverse ``rev_edge[d]`` share one pair: what depends on the unordered atom pair alone -- the EdgeBlock's c2
branch -- need be computed once per pair.  Read through ``rn_potgnn_debug_plan_pairs`` beside
``rn_potgnn_debug_plan`` (which has ``rev_edge``), on the graphs of ``tests/helpers.py: sparse_structures()``, on a dense
rocksalt cell, and on directed graphs in which many edges have no reverse.
"""
import ctypes

import numpy as np
import pytest

from ramannoodle_amd import _lib
from ramannoodle_amd.pmodel import graph as G
from tests.helpers import ragged_graph, sparse_structures
from tests.plan_worker import debug_plan
from tests.test_host_logic import _parse_plan


def _pairs(lib, shape, ea, eb, types, num_cus=256):
    """``rn_potgnn_debug_plan_pairs``: (NP, pair_of_edge, pair_a, pair_b), size query first."""
    n, e, k, fn, fe = shape
    cfg = _lib.Config(n, e, k, fn, fe, 2, -1.0, 0, 0)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    count = ctypes.c_size_t(0)
    rc = lib.rn_potgnn_debug_plan_pairs(ctypes.byref(cfg), p(ea), p(eb), p(types), num_cus, None, 0, ctypes.byref(count))
    assert rc == _lib.RN_ERR_INVALID_ARGUMENT and count.value >= 1 + e, lib.rn_potgnn_last_error(None)
    out = np.full(count.value, -7, dtype=np.int32)
    rc = lib.rn_potgnn_debug_plan_pairs(ctypes.byref(cfg), p(ea), p(eb), p(types), num_cus, p(out), out.size, ctypes.byref(count))
    assert rc == _lib.RN_OK, lib.rn_potgnn_last_error(None)
    num = int(out[0])
    assert out.size == 1 + e + 2 * num
    return num, out[1:1 + e], out[1 + e:1 + e + num], out[1 + e + num:]


def _graphs():
    from bench import rocksalt
    out = []
    for name, (lattice, positions, zs, cutoff) in sparse_structures().items():
        edges = G.radius_graph_pbc(lattice, positions, cutoff)
        tmap = G.atom_type_map(zs)
        out.append((name, edges[0], edges[1], tmap[np.asarray(zs)], int((tmap >= 0).sum())))
    lattice, positions, zs = rocksalt(2, 2, 2)  # 64 atoms, 18 neighbours each at the benchmark's cutoff
    edges = G.radius_graph_pbc(lattice, positions, 3.2)
    tmap = G.atom_type_map(zs)
    out.append(("rocksalt222", edges[0], edges[1], tmap[np.asarray(zs)], int((tmap >= 0).sum())))
    for seed in (0, 5):  # directed: most edges have no reverse
        ea, eb, types, k = ragged_graph(seed)
        out.append((f"ragged{seed}", ea, eb, types, k))
    return [(name, *(np.ascontiguousarray(x, dtype=np.int32) for x in (ea, eb, types)), k) for name, ea, eb, types, k in out]


GRAPHS = _graphs()


@pytest.mark.parametrize("case", GRAPHS, ids=[c[0] for c in GRAPHS])
def test_pair_table(case):
    name, ea, eb, types, k = case
    lib = _lib.load()
    n, e = len(types), len(ea)
    shape = (n, e, k, 64, 64)
    rev = _parse_plan(debug_plan(lib, shape, ea, eb, types, 256), n, e)["rev_edge"]
    num, of_edge, pa, pb = _pairs(lib, shape, ea, eb, types)
    # the reverse edge is the reverse edge
    has = rev >= 0
    np.testing.assert_array_equal(ea[rev[has]], eb[has])
    np.testing.assert_array_equal(eb[rev[has]], ea[has])
    if name.startswith("ragged"):
        assert (~has).sum() > e // 4, "the directed graphs are here for their edges without a reverse"
    else:
        assert has.all() and e % 2 == 0
    # an edge and its reverse share a pair; the pair's atoms are the edge's, in either order
    np.testing.assert_array_equal(of_edge[rev[has]], of_edge[has])
    assert of_edge.min() >= 0 and of_edge.max() == num - 1
    lo, hi = np.minimum(ea, eb), np.maximum(ea, eb)
    np.testing.assert_array_equal(np.minimum(pa, pb)[of_edge], lo)
    np.testing.assert_array_equal(np.maximum(pa, pb)[of_edge], hi)
    # one pair per edge that has no reverse of a lower id
    assert num == e - int(((rev >= 0) & (rev < np.arange(e))).sum())
    if not name.startswith("ragged"):
        assert num == e // 2
    # compact, in ascending order of the pair's lower edge id, with that edge's atoms
    first = np.full(num, e, dtype=np.int64)
    np.minimum.at(first, of_edge, np.arange(e))
    assert (first < e).all() and np.all(np.diff(first) > 0)
    np.testing.assert_array_equal(pa, ea[first])
    np.testing.assert_array_equal(pb, eb[first])
    # at most two edges per pair, and two only as (d, rev_edge[d])
    members = np.bincount(of_edge, minlength=num)
    assert members.min() >= 1 and members.max() <= 2
    alone = members[of_edge] == 1
    np.testing.assert_array_equal(alone, ~has)


def test_pair_table_is_deterministic_and_validated():
    """Two calls give the same table; the arguments are validated like those of ``rn_potgnn_debug_plan``."""
    lib = _lib.load()
    name, ea, eb, types, k = GRAPHS[3]
    shape = (len(types), len(ea), k, 64, 64)
    a, b = _pairs(lib, shape, ea, eb, types), _pairs(lib, shape, ea, eb, types)
    for x, y in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(x, y)
    p = lambda v: ctypes.c_void_p(v.ctypes.data)  # noqa: E731
    cfg = _lib.Config(len(types), len(ea), k, 64, 64, 2, -1.0, 0, 0)
    count, out = ctypes.c_size_t(0), np.zeros(8, dtype=np.int32)
    assert lib.rn_potgnn_debug_plan_pairs(ctypes.byref(cfg), None, p(eb), p(types), 256, p(out), out.size, ctypes.byref(count)) \
        == _lib.RN_ERR_INVALID_ARGUMENT
    assert lib.rn_potgnn_debug_plan_pairs(ctypes.byref(cfg), p(ea), p(eb), p(types), 0, p(out), out.size, ctypes.byref(count)) \
        == _lib.RN_ERR_INVALID_ARGUMENT
    swapped = ea[::-1].copy()  # no longer sorted by (a, b)
    assert lib.rn_potgnn_debug_plan_pairs(ctypes.byref(cfg), p(swapped), p(eb), p(types), 256, p(out), out.size,
                                          ctypes.byref(count)) == _lib.RN_ERR_INVALID_ARGUMENT
    assert b"sorted" in lib.rn_potgnn_last_error(None)
