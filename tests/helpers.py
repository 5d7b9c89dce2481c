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
