"""Shared helpers for the tests (builders for product models from golden fixtures and
synthetic workloads)."""
import numpy as np

from ramannoodle_amd.pmodel import PotGNN
from ramannoodle_amd.structure import ReferenceStructure


def product_model_from_golden(g, mean=None, stddev=None, **kw):
    """Build the device PotGNN from a golden fixture's structure, hyper-parameters and
    state dict (the graph is rebuilt by the product's own host code); ``mean`` / ``stddev``
    override the fixture's de-standardisation tensors."""
    hp = g["hp"]
    ref = ReferenceStructure([int(z) for z in g["atomic_numbers"]], g["lattice"], g["positions"])
    model = PotGNN(ref, float(hp[0]), int(hp[1]), int(hp[2]), int(hp[3]), float(hp[4]),
                   float(hp[5]), g["mean"] if mean is None else mean, g["std"] if stddev is None else stddev, **kw)
    sd = {k[3:]: g[k] for k in g.files if k.startswith("sd/")}
    model.load_state_dict(sd)
    return model


# ----------------------------------------------------------------------------- sparse and tiny graphs
def sparse_structures():
    """name -> (lattice, fractional positions, atomic numbers, cutoff): five deterministic structures in a 14 A slightly
    triclinic box whose graphs have what the fixtures' graphs lack -- atoms without edges, atoms of degree 1, destination
    edges without a triplet, no triplet at all, fewer atoms than one 16-atom tile, one species, five species.
    ``SPARSE_PROPERTIES`` lists what each must have; tests/test_host_logic.py asserts it."""
    rng = np.random.default_rng(0)
    lattice = np.diag([14.0, 15.4, 12.6]) + 0.4 * rng.normal(size=(3, 3))

    def frac(cart):
        return (np.asarray(cart, dtype=np.float64) @ np.linalg.inv(lattice)) % 1.0

    out = {}
    out["dimer"] = (lattice, frac([[1, 1, 1], [2.2, 1, 1]]), [14, 14], 2.0)
    out["iso_dimer_iso"] = (lattice, frac([[7, 7, 7], [1, 1, 1], [2.2, 1.1, 1], [10, 3, 9]]), [8, 1, 8, 1], 2.0)
    out["chain5"] = (lattice, frac([[1 + 1.0 * i, 2 + 0.1 * i * i, 3] for i in range(5)]), [6, 1, 7, 8, 9], 1.25)
    # hub17: atom 0 isolated, atom 1 a hub with 14 shell atoms 2.0 A away, atom 16 isolated and alone in the second 16-atom tile
    shell = np.random.default_rng(3).normal(size=(14, 3))
    shell = 2.0 * shell / np.linalg.norm(shell, axis=1)[:, None] + 7.0
    out["hub17"] = (lattice, frac(np.vstack([[1, 1, 1], [7, 7, 7], shell, [12, 12, 1.5]])), [8, 22] + [8] * 14 + [22], 2.1)
    # molecules33: eleven bent three-atom molecules, 4 A and more apart
    rng, cart, zs = np.random.default_rng(4), [], []
    for m in range(11):
        o = np.array([1.5 + (m % 3) * 4.2, 1.5 + ((m // 3) % 3) * 4.5, 1.5 + (m // 9) * 4.0]) + 0.2 * rng.normal(size=3)
        cart += [o, o + [0.96, 0.05 * m, 0], o + [-0.24, 0.93, 0.03 * m]]
        zs += [8, 1, 1]
    out["molecules33"] = (lattice, frac(cart), zs, 1.2)
    return out


# N, E, T, species, atoms without an edge, destination edges without a triplet (tuple slot 5 of the triplets never names
# them: their c3 sum is empty), atoms of degree 1
SPARSE_PROPERTIES = {
    "dimer": dict(N=2, E=2, T=0, K=1, edge_free=0, triplet_less=2, degree_one=2),
    "iso_dimer_iso": dict(N=4, E=2, T=0, K=2, edge_free=2, triplet_less=2, degree_one=2),
    "chain5": dict(N=5, E=8, T=6, K=5, edge_free=0, triplet_less=2, degree_one=2),
    "hub17": dict(N=17, E=82, T=468, K=2, edge_free=2, triplet_less=0, degree_one=0),
    "molecules33": dict(N=33, E=44, T=22, K=2, edge_free=0, triplet_less=22, degree_one=22),
}


def sparse_fixture(name, frames=5, seed=0):
    """The fixture-like dict ``tests/test_gpu_parity.py: _random_model`` takes, for one of ``sparse_structures()``:
    ``pos_batch`` = the reference positions + N(0, 2e-3), seeded.  Returns (dict, cutoff)."""
    lattice, positions, zs, cutoff = sparse_structures()[name]
    rng = np.random.default_rng(1000 + seed)
    pos_batch = positions[None] + rng.normal(scale=2e-3, size=(frames,) + positions.shape)
    return {"lattice": lattice, "positions": positions, "atomic_numbers": np.asarray(zs), "pos_batch": pos_batch}, cutoff


# ----------------------------------------------------------------------------- graph plans (rn_potgnn_debug_plan)
PLAN_WIDTHS = ((5, 14), (16, 16), (20, 48), (32, 64), (64, 64), (50, 40), (64, 16), (128, 128))
PLAN_FIXTURES = ("triclinic20", "rocksalt64_parity", "rocksalt64_perf", "tio2_gnn_test")
# one process per entry: some knobs are read once per process
PLAN_KNOBS = ({}, {"FUSED": "0"}, {"NARROW": "0"}, {"EDGE_PS": "0"}, {"PS_BACK": "2"}, {"PS_GRAM": "1"}, {"NODE_ATOM": "0"},
              {"NODE_ATOM": "1"}, {"BWD_TILES": "0"}, {"TILE_KB": "32"}, {"WIDEN": "0"}, {"WIDEN": "1"})


def plan_group_name(knobs):
    return "default" if not knobs else "_".join(f"{k}={v}" for k, v in knobs.items())


def ragged_graph(seed):
    """A seeded directed graph with uneven degrees: every atom has 1 .. `hi` out-edges (hi up to 50) towards destinations
    drawn with very unequal weights, plus a ring a -> a + 1, so that in-degrees run from 1 to about 50 as well."""
    rng = np.random.default_rng(7000 + seed)
    n = int(rng.integers(20, 97))
    hi = min(int((6, 12, 25, 50)[seed % 4]), n - 2)
    weight = rng.random(n) ** float((1, 3, 6)[seed % 3])
    ea, eb = [], []
    for a in range(n):
        p = weight.copy()
        p[a] = 0
        others = rng.choice(n, size=int(rng.integers(1, hi + 1)), replace=False, p=p / p.sum())
        bs = np.unique(np.concatenate([others, [(a + 1) % n]]))
        ea += [a] * len(bs)
        eb += list(bs)
    types = rng.integers(0, 3, size=n)
    types[:3] = (0, 1, 2)
    return np.array(ea, dtype=np.int32), np.array(eb, dtype=np.int32), types.astype(np.int32), 3


def plan_cases(knobs):
    """(name, (N, E, K, Fn, Fe), edge_a, edge_b, atom_types) of every graph-plan case of one knob group: under default
    knobs the committed fixtures' graphs at the cutoffs and widths the GPU parity tests use, the benchmark's rocksalt cells
    at eight width pairs and 24 ragged graphs; under a knob variant the 64/64 and the 5/14 benchmark graph."""
    from bench import make_workload
    from ramannoodle_amd.pmodel import graph as G
    from tests.conftest import load_golden
    cases = []

    def add(name, ea, eb, types, k, fn, fe):
        ea, eb, types = (np.ascontiguousarray(x, dtype=np.int32) for x in (ea, eb, types))
        cases.append((name, (len(types), len(ea), int(k), int(fn), int(fe)), ea, eb, types))

    def bench_graph(cells):
        model = make_workload(num_cells=cells, frames=1)["model"]()
        types = model.atom_type_map[np.asarray(model._ref_structure.atomic_numbers)]
        return model.ref_edge_indexes[1], model.ref_edge_indexes[2], types, model._num_atom_types

    if knobs:
        ea, eb, types, k = bench_graph((4, 4, 2))
        for fn, fe in ((64, 64), (5, 14)):
            add(f"bench442_{fn}_{fe}", ea, eb, types, k, fn, fe)
        return cases
    for name in PLAN_FIXTURES:
        g = load_golden(name)
        edges = G.radius_graph_pbc(g["lattice"], g["positions"], float(g["hp"][0]))
        tmap = G.atom_type_map(g["atomic_numbers"])
        add(name, edges[0], edges[1], tmap[np.asarray(g["atomic_numbers"])], (tmap >= 0).sum(), g["hp"][1], g["hp"][2])
    for cells in ((2, 2, 2), (4, 2, 2), (4, 4, 2)):
        ea, eb, types, k = bench_graph(cells)
        for fn, fe in PLAN_WIDTHS:
            add("bench%d%d%d_%d_%d" % (*cells, fn, fe), ea, eb, types, k, fn, fe)
    for seed in range(24):
        ea, eb, types, k = ragged_graph(seed)
        fn, fe = (64, 64) if seed % 2 == 0 else PLAN_WIDTHS[(seed // 2) % len(PLAN_WIDTHS)]
        add(f"ragged{seed:02d}_{fn}_{fe}", ea, eb, types, k, fn, fe)
    return cases
