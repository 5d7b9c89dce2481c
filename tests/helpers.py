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


# ----------------------------------------------------------------------------- dense and uneven graphs
DENSE_CUTOFF = 3.0
BLOB_RING_ATOMS = 66
BLOB_ATOMS = {"blob_gas": 56, "blob_ring": BLOB_RING_ATOMS}
BLOB_SEEDS = {"blob_gas": 11, "blob_ring": 12}
HUB_SEEDS = {"hub_cap128": 30, "hub_cap64": 88}  # (chosen for the gap around the cutoff: most seeds leave a pair within 1e-3 A of it)
HUB_SHELL = {"hub_cap128": 71, "hub_cap64": 147}  # the out-degree caps at FeP = 128 and at FeP = 64 (DESIGN.md "Limits")


def dense_structures():
    """name -> (lattice, fractional positions, atomic numbers, cutoff): four deterministic structures in the 14 A box of
    ``sparse_structures()`` at a cutoff of 3.0 A (under half the box: no pair wraps) whose graphs are dense and very uneven.
    ``blob_gas`` / ``blob_ring``: a ball of radius 1.4 A holding 56 / BLOB_RING_ATOMS atoms (a complete graph) among fourteen
    two- and three-atom molecules, the atom order shuffled so that every 16-atom group mixes the ball's degree with degree
    1 - 2; ``blob_ring`` is the smallest ball whose 64-wide plan keeps the fused path while the role-specialised
    EdgeBlock's ring refuses it.  ``hub_cap128`` / ``hub_cap64``: one atom at the centre of 71 / 147 atoms on a sphere of
    radius 2.95 A, in the middle of the atom order: its degree is exactly the largest the library accepts at a padded edge
    width of 128 / 64.  ``DENSE_PROPERTIES`` pins each graph; tests/test_host_logic.py asserts it, that the float32 and the
    float64 edge lists agree and that no pair distance lies within 1e-3 A of the cutoff."""
    lattice = sparse_structures()["dimer"][0]
    inverse = np.linalg.inv(lattice)
    centre = np.array([0.5, 0.5, 0.5]) @ lattice
    out = {}
    for name, ball in BLOB_ATOMS.items():
        rng = np.random.default_rng(BLOB_SEEDS[name])
        cart = []
        while len(cart) < ball:  # uniform in the ball, no two atoms closer than 0.4 A
            x = rng.uniform(-1.4, 1.4, size=3)
            if np.linalg.norm(x) <= 1.4 and all(np.linalg.norm(x - y) >= 0.4 for y in cart):
                cart.append(x)
        cart = [centre + x for x in cart]
        zs = [22] * ball
        # the molecules sit on the 3 x 3 x 3 grid of cell thirds whose centre site is the ball, on the twenty sites that
        # share no face with it: 6 A and more from the ball's centre, 4 A and more from each other
        sites = [(i, j, k) for i in range(3) for j in range(3) for k in range(3) if (i != 1) + (j != 1) + (k != 1) >= 2]
        for m, site in enumerate(sites[:14]):
            o = (np.array(site) / 3.0 + 1.0 / 6.0) @ lattice - [0.4, 0.4, 0.0]
            atoms = [o, o + [0.96, 0.04 * m, 0.0], o + [-0.24, 0.93, 0.02 * m]][:2 + m % 2]
            cart += atoms
            zs += [8, 1, 1][:len(atoms)]
        order = np.random.default_rng(13).permutation(len(zs))
        out[name] = (lattice, (np.array(cart)[order] @ inverse) % 1.0, [zs[i] for i in order], DENSE_CUTOFF)
    for name, shell in HUB_SHELL.items():
        # a golden-angle spiral over the sphere (neighbours 0.5 A and more apart), each point moved by N(0, 0.05) along it
        i = np.arange(shell) + 0.5
        polar, azimuth = np.arccos(1 - 2 * i / shell), np.pi * (1 + 5 ** 0.5) * i
        u = np.stack([np.sin(polar) * np.cos(azimuth), np.sin(polar) * np.sin(azimuth), np.cos(polar)], axis=1)
        u += np.random.default_rng(HUB_SEEDS[name]).normal(scale=0.05, size=u.shape)
        cart = centre + 2.95 * u / np.linalg.norm(u, axis=1)[:, None]
        half = shell // 2
        cart = np.vstack([cart[:half], [centre], cart[half:]])
        out[name] = (lattice, (cart @ inverse) % 1.0, [8] * half + [22] + [8] * (shell - half), DENSE_CUTOFF)
    return out


# N, E, T, smallest and largest degree: from the oracle's graph code (tests/test_host_logic.py compares)
DENSE_PROPERTIES = {
    "blob_gas": dict(N=91, E=3136, T=166362, min_degree=1, max_degree=55),
    "blob_ring": dict(N=101, E=4346, T=274602, min_degree=1, max_degree=65),
    "hub_cap128": dict(N=72, E=1400, T=28582, min_degree=17, max_degree=71),
    "hub_cap64": dict(N=148, E=5754, T=229990, min_degree=35, max_degree=147),
}


def dense_fixture(name, frames=3, seed=0):
    """``sparse_fixture`` for one of ``dense_structures()``."""
    lattice, positions, zs, cutoff = dense_structures()[name]
    rng = np.random.default_rng(2000 + seed)
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


# ----------------------------------------------------------------------------- packed weights (rn_potgnn_debug_pack_weights)
def state_dict_sizes(k, fn, fe, passes):
    """(name, element count) of every tensor of a PotGNN state dict, in state-dict order, written out independently of the
    library's table (csrc/weight_layout.hip): node blocks of all passes first, then the edge blocks, then the readout."""
    out = [("emb", k * fn), ("W2", fn * fn), ("b2", fn), ("W4", fn * fn), ("b4", fn), ("offset", fe)]
    for p in range(passes):
        out += [(f"{p}/c1_w", 2 * fn * (fn + fe)), (f"{p}/c1_b", 2 * fn), (f"{p}/c1n_g", 2 * fn), (f"{p}/c1n_b", 2 * fn),
                (f"{p}/fin_g", fn), (f"{p}/fin_b", fn)]
    for p in range(passes):
        out += [(f"{p}/c2_w", 2 * fe * fn), (f"{p}/c2_b", 2 * fe), (f"{p}/c3_w", 2 * fe * (3 * fn + 2 * fe)), (f"{p}/c3_b", 2 * fe)]
        out += [(f"{p}/{n}", 2 * fe) for n in ("c2n1_g", "c2n1_b", "c3n1_g", "c3n1_b")]
        out += [(f"{p}/{n}", fe) for n in ("c2n2_g", "c2n2_b", "c3n2_g", "c3n2_b")]
    out += [("W0", fe * fe), ("b0", fe), ("bn_w", fe), ("bn_b", fe), ("bn_rm", fe), ("bn_rv", fe), ("W3", fe * fe), ("b3", fe),
            ("W5", 12 * fe), ("b5", 12)]
    return out


STATE_DICT_BUFFERS = ("offset", "bn_rm", "bn_rv")  # not parameters: Gaussian offsets, BatchNorm running statistics
WEIGHT_SHAPES = ((1, 1, 1, 1), (3, 5, 14, 2), (2, 16, 16, 1), (2, 20, 40, 2), (2, 8, 64, 1), (3, 64, 64, 4), (1, 100, 128, 1))


def state_dict_slices(k, fn, fe, passes):
    sizes = state_dict_sizes(k, fn, fe, passes)
    starts = np.concatenate([[0], np.cumsum([n for _, n in sizes])])
    return {name: slice(int(a), int(b)) for (name, _), a, b in zip(sizes, starts[:-1], starts[1:])}


def weight_layout_cases():
    """(name, (K, Fn, Fe, P), float32 state-dict blob): seeded normal blobs at WEIGHT_SHAPES, then at (2, 64, 64, 2) a tame
    blob on which the split-f16 range guard and the folded gate both hold ("flags_base": weights 0.1 N(0,1), LayerNorm
    gammas and the running variance near 1) and three variants that each flip one decision."""
    cases = []
    for i, shape in enumerate(WEIGHT_SHAPES):
        n = sum(size for _, size in state_dict_sizes(*shape))
        cases.append(("normal_%d_%d_%d_%d" % shape, shape, np.random.default_rng(100 + i).normal(size=n).astype(np.float32)))
    shape = (2, 64, 64, 2)
    at = state_dict_slices(*shape)
    base = (0.1 * np.random.default_rng(200).normal(size=max(s.stop for s in at.values()))).astype(np.float32)
    for name, s in at.items():
        if name.endswith("_g") or name in ("bn_w", "bn_rv"):
            base[s] = 1.0 + np.abs(base[s])
    cases.append(("flags_base", shape, base))
    inf = base.copy()
    inf[at["1/c2_w"].start + 77] = np.inf  # a non-finite weight: the range guard refuses
    cases.append(("flags_c2_inf", shape, inf))
    wide = base.copy()
    wide[at["W0"]] *= 1e3  # |h1| <= ~5e3, |h2| <= ~5e3 * 5e3: beyond the 3e4 bound, the handle falls back
    wide[at["W3"]] *= 1e3
    cases.append(("flags_readout_bound", shape, wide))
    gamma = base.copy()
    gamma[at["1/c3n1_g"].start + 64 + 5] = 1e-6  # a real core-half gamma of pass 1 the loop cannot divide by
    cases.append(("flags_small_gamma", shape, gamma))
    return cases
