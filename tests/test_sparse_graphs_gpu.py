"""Every kernel family on sparse and tiny graphs, forward and reverse.

The fixtures' graphs are dense: hardly any parity test meets an atom without edges, an atom of degree 1, a destination
edge whose triplet sum is empty, a graph without triplets, fewer atoms than one 16-atom tile, one species or five.
``tests/helpers.py: sparse_structures()`` has five structures that do (tests/test_host_logic.py pins their graphs);
here the narrow kernels (exact 5/14, masked 13/9), the wide fused kernels (64/64, PAD 40/50) under each kernel choice,
the 24/20 and 40/100 widths, the float64 paths, the reverse-mode Jacobian, the training step in float64 and float32 and
the input gradients run on them against the float64 oracle.  Where a float32 bound depends on how well float32 can do at
all on such a graph (a dimer's output hangs on two rows), it is three times the float32 oracle's own distance from the
float64 oracle, computed in the test, and never below the suite's fixed bar.  Needs a real MI355X: run with ``-m gpu``.
"""
import numpy as np
import pytest
import torch

from tests.helpers import SPARSE_PROPERTIES, sparse_fixture
from tests.test_gpu_parity import REL, _random_model, _rel_err
from tests.test_input_gradients import _device_grads, _err, _inputs, _oracle_grads
from tests.test_input_gradients import _no_default_device_mode  # noqa: F401  (autouse: no default-device mode in here)

pytestmark = pytest.mark.gpu

NAMES = list(SPARSE_PROPERTIES)
NARROW = ((5, 14), (13, 9))
PASSES = 2


def _case(name, fn, fe, frames=5):
    """(fixture-like dict, product model, float32 oracle, float64 oracle) of one structure at one width pair."""
    g, cutoff = sparse_fixture(name, frames=frames)
    model, oracle = _random_model(g, cutoff, fn, fe, PASSES, seed=fn * 1000 + fe + NAMES.index(name))
    assert (model.num_atoms, model.num_edges, oracle.num_triplets) == tuple(SPARSE_PROPERTIES[name][k] for k in "NET")
    return g, model, oracle, oracle.to(torch.float64)


def _graph(oracle):
    """(atoms without an edge, destination edges without a triplet) of the frozen graph."""
    n, e = oracle.num_atoms, oracle.num_edges
    degree = np.bincount(oracle.edges[1].numpy(), minlength=n)
    per_edge = np.bincount(oracle.trip[5].numpy(), minlength=e)
    return np.flatnonzero(degree == 0), np.flatnonzero(per_edge == 0)


def _standardised(alpha, oracle):
    return (np.asarray(alpha) - oracle.mean) / oracle.std


def _forward_check(model, oracle64, pos, what):
    from oracle import potgnn_oracle as O
    got = model.calc_polarizabilities(pos)
    assert np.isfinite(got).all(), what
    want = O.calc_polarizabilities(oracle64, pos, faithful=False)
    err = _rel_err(_standardised(got, oracle64), _standardised(want, oracle64))
    print(f"forward {what}: device f32 vs oracle f64 {err:.2e}")
    assert err < REL, (what, err)
    np.testing.assert_array_equal(model.calc_polarizabilities(pos), got, err_msg=str(what))
    np.testing.assert_array_equal(model.calc_polarizabilities(pos[0:1])[0], got[0], err_msg=str(what))
    return got


# ----------------------------------------------------------------------------- a. forward
@pytest.mark.parametrize("fn, fe", [(5, 14), (13, 9), (64, 64), (40, 50), (24, 20), (40, 100), (8, 20)])
@pytest.mark.parametrize("name", NAMES)
def test_forward_against_the_float64_oracle(name, fn, fe):
    """Two passes at the exact narrow instantiation, a masked narrow one, the default wide path, its PAD instantiation,
    24/20 (padded 32/32, which the planner widens onto the 64-wide fused kernels), and the unfused chain at 40/100
    (padded 64/128) and 8/20 (padded 16/32): standardised output within 1e-5 of the float64 oracle, a second evaluation
    bit-identical, frame 0 alone bit-identical to frame 0 of the batch."""
    g, model, _, oracle64 = _case(name, fn, fe)
    _forward_check(model, oracle64, g["pos_batch"], (name, fn, fe))
    flags = model.config_flags()
    if (fn, fe) in NARROW:
        assert flags["narrow_kernels"]
    if (fn, fe) in ((64, 64), (40, 50)):
        assert flags["fused_edge_block"]
    if (fn, fe) in ((40, 100), (8, 20)):
        assert not flags["fused_edge_block"] and not flags["narrow_kernels"]


# ----------------------------------------------------------------------------- b. kernel choices at 64/64
@pytest.mark.parametrize("knob, value, flag, state", [
    (None, None, None, None),
    ("RN_POTGNN_EDGE_PS", "0", "role_split_edge_block", False),
    ("RN_POTGNN_NODE_ATOM", "0", "atom_owning_node_block", False),
    ("RN_POTGNN_NODE_ATOM", "1", "atom_owning_node_block", True),
    ("RN_POTGNN_FUSED", "0", "fused_edge_block", False),
])
@pytest.mark.parametrize("name", ["hub17", "molecules33", "iso_dimer_iso"])
def test_wide_kernel_choices_against_the_float64_oracle(monkeypatch, name, knob, value, flag, state):
    """64/64 under default knobs, without the role-specialised EdgeBlock, with the row-ordered and with the atom-owning
    NodeBlock, and on the unfused chain.  Under default knobs the role-specialised EdgeBlock must be what runs on hub17
    (edge-free atoms, a second 16-atom tile without rows) and molecules33 (22 destination edges without a triplet)."""
    if knob is not None:
        monkeypatch.setenv(knob, value)
    g, model, _, oracle64 = _case(name, 64, 64)
    _forward_check(model, oracle64, g["pos_batch"], (name, knob, value))
    flags = model.config_flags()
    if knob is None:
        assert flags["fused_edge_block"]
        if name in ("hub17", "molecules33"):
            assert flags["role_split_edge_block"], flags
    else:
        assert flags[flag] == state, flags


# ----------------------------------------------------------------------------- c. stages
@pytest.mark.parametrize("fn, fe", [(64, 64), (5, 14)])
@pytest.mark.parametrize("name", ["hub17", "molecules33"])
def test_stages_on_edge_free_atoms_and_triplet_less_edges(monkeypatch, name, fn, fe):
    """Node and edge rows after the embedding and after each pass against the float32 oracle (atol 2e-5).  No output
    depends on the node row of an atom without edges -- its NodeBlock sum is empty, LayerNorm of the zero row is
    ``final_norm.bias``, the row becomes tanh(node + bias) -- so only this comparison sees it; the rows of destination
    edges without a triplet take ``c3_norm_2.bias`` the same way.  Both sets are compared again on their own."""
    from oracle import potgnn_oracle as O
    monkeypatch.setenv("RN_POTGNN_KEEP_STAGES", "1")
    g, model, oracle, _ = _case(name, fn, fe)
    pos = g["pos_batch"]
    s, n, e = pos.shape[0], model.num_atoms, model.num_edges
    model.eval()
    model.forward(torch.tensor(g["lattice"]).expand(s, 3, 3), torch.tensor(g["atomic_numbers"]).expand(s, -1), torch.tensor(pos))
    stages = {}
    O.forward(oracle, pos, faithful=False, stages=stages)
    free, bare = _graph(oracle)
    assert len(free) == SPARSE_PROPERTIES[name]["edge_free"] and len(bare) == SPARSE_PROPERTIES[name]["triplet_less"]
    free_rows = (np.arange(s)[:, None] * n + free[None, :]).reshape(-1)
    bare_rows = (np.arange(s)[:, None] * e + bare[None, :]).reshape(-1)
    for p in range(PASSES + 1):
        node_ref, edge_ref = stages[f"node{p}"].numpy(), stages[f"edge{p}"].numpy()
        if p > 0 and len(free):  # (what the oracle itself gives an atom without edges)
            bias = oracle.sd[f"_node_blocks.{p - 1}.final_norm.bias"].numpy()
            np.testing.assert_allclose(node_ref[free_rows], np.tanh(stages[f"node{p - 1}"].numpy()[free_rows] + bias), atol=1e-6)
        node, edge = model.debug_stage(1, p), model.debug_stage(2, p)
        assert node.shape == node_ref.shape and edge.shape == edge_ref.shape, (p, node.shape, edge.shape)
        np.testing.assert_allclose(node, node_ref, rtol=0, atol=2e-5, err_msg=f"node{p}")
        np.testing.assert_allclose(edge, edge_ref, rtol=0, atol=2e-5, err_msg=f"edge{p}")
        np.testing.assert_allclose(node[free_rows], node_ref[free_rows], rtol=0, atol=2e-5,
                                   err_msg=f"node{p}: rows of the atoms without edges {free.tolist()}")
        np.testing.assert_allclose(edge[bare_rows], edge_ref[bare_rows], rtol=0, atol=2e-5,
                                   err_msg=f"edge{p}: rows of the destination edges without a triplet {bare.tolist()}")


# ----------------------------------------------------------------------------- d. float64 evaluation
@pytest.mark.parametrize("fn, fe", [(5, 14), (64, 64)])
@pytest.mark.parametrize("name", NAMES)
def test_float64_evaluation_against_the_float64_oracle(name, fn, fe):
    """The kernels instantiated for ``double``, at the tolerance of ``test_calc_polarizabilities_in_float64`` (5e-8), on
    the polarizabilities and on their standardised part."""
    from oracle import potgnn_oracle as O
    g, model, _, oracle64 = _case(name, fn, fe)
    pos = g["pos_batch"]
    got = model.calc_polarizabilities(pos, dtype=torch.float64)
    want = O.calc_polarizabilities(oracle64, pos, faithful=False)
    err = _rel_err(_standardised(got, oracle64), _standardised(want, oracle64))
    print(f"float64 forward {name} {fn}/{fe}: device f64 vs oracle f64 {err:.2e} (standardised), {_rel_err(got, want):.2e}")
    assert np.isfinite(got).all()
    assert _rel_err(got, want) < 5e-8 and err < 5e-8, (name, fn, fe, err)
    np.testing.assert_array_equal(model.calc_polarizabilities(pos, dtype=torch.float64), got)


# ----------------------------------------------------------------------------- e. reverse-mode Jacobian
@pytest.mark.parametrize("fn, fe", [(5, 14), (64, 64), (24, 20), (8, 20)])
@pytest.mark.parametrize("name", NAMES)
def test_reverse_mode_jacobian_against_autograd(name, fn, fe):
    """d(vec6)/d(r) through two passes (8/20: the unfused chain at padded 16/32): float64 within 1e-9 of autograd through the float64 oracle; float32 within
    max(5e-5, 3 x the float32 oracle's own distance from it); translation invariant; the rows of atoms without edges are
    exactly zero."""
    from oracle import potgnn_oracle as O
    g, model, oracle, oracle64 = _case(name, fn, fe)
    pos = g["pos_batch"][1]
    want = O.jacobian(oracle64, pos)
    scale = np.abs(want).max()
    assert np.isfinite(want).all() and scale > 0
    d_ref = np.abs(O.jacobian(oracle, pos) - want).max() / scale
    got64 = model.alpha_jacobian(pos, float64=True)
    got32 = model.alpha_jacobian(pos, float64=False)
    d64, d32 = np.abs(got64 - want).max() / scale, np.abs(got32 - want).max() / scale
    print(f"jacobian {name} {fn}/{fe}: device f64 {d64:.2e}, device f32 {d32:.2e}, oracle f32 {d_ref:.2e} (of max |J|, vs oracle f64)")
    assert np.isfinite(got64).all() and np.isfinite(got32).all()
    assert d64 < 1e-9, d64
    assert d32 < max(5e-5, 3 * d_ref), (d32, d_ref)
    assert np.abs(got64.sum(axis=1)).max() < 1e-9 * scale
    free, _ = _graph(oracle)
    assert len(free) == SPARSE_PROPERTIES[name]["edge_free"]
    assert np.all(got64[:, free, :] == 0) and np.all(got32[:, free, :] == 0)


# ----------------------------------------------------------------------------- f. training gradients
NO_TRIPLET_ZERO_GRADIENTS = sorted(
    [f"_edge_blocks.{p}.{k}" for p in range(PASSES)
     for k in ("c3_linear.weight", "c3_linear.bias", "c3_norm_1.weight", "c3_norm_1.bias", "c3_norm_2.weight")]
    + ["_to_polarizability_embedding.0.bias"])  # (the bias in front of BatchNorm never has a gradient)


@pytest.mark.parametrize("name, fn, fe", [(name, fn, fe) for name in NAMES for fn, fe in ((5, 14), (64, 64))]
                         + [("molecules33", 24, 20)])
def test_training_gradients_against_autograd(name, fn, fe):
    """One training step on four frames with random targets.  float64 device step against float64 autograd through the
    oracle (outputs and loss 1e-9, every parameter 1e-8 of its largest gradient).  float32 step against the float64
    device gradients: per parameter within max(2e-4, 3 x the float32 oracle's distance from the float64 oracle for that
    parameter) of the parameter's largest gradient.  A parameter without a gradient -- on a graph without triplets all of
    ``c3_linear``, ``c3_norm_1`` and ``c3_norm_2.weight`` -- comes back below 1e-6 from both; ``c3_norm_2.bias`` has one
    on every graph (every destination edge adds to it, with or without triplets).  BatchNorm running statistics of the
    float32 step against ``F.batch_norm`` in the oracle."""
    from oracle import potgnn_oracle as O
    g, model, oracle, oracle64 = _case(name, fn, fe, frames=4)
    pos = g["pos_batch"]
    targets = np.random.default_rng(8).normal(size=(4, 6))
    o_out, o_loss, o_grads = O.train_gradients(oracle64, pos, targets)
    _, _, o_grads32 = O.train_gradients(oracle, pos, targets)
    assert all(np.isfinite(v).all() for v in o_grads.values())
    zero = sorted(k for k, v in o_grads.items() if np.abs(v).max() < 1e-12)
    if SPARSE_PROPERTIES[name]["T"] == 0:
        assert zero == NO_TRIPLET_ZERO_GRADIENTS
    else:
        assert zero == ["_to_polarizability_embedding.0.bias"]
    checked = set()  # (c3_norm_2.bias is among the parameters compared below, never among the skipped ones)
    assert not any(k.endswith("c3_norm_2.bias") for k in zero)

    out64, loss64, grads64 = model.train_gradients_f64(pos, targets)
    np.testing.assert_allclose(out64, o_out, rtol=0, atol=1e-9 * np.abs(o_out).max())
    assert loss64 == pytest.approx(o_loss, rel=1e-9)
    worst64 = 0.0
    for key, ref in o_grads.items():
        scale = np.abs(ref).max()
        assert np.isfinite(grads64[key]).all(), key
        assert np.abs(grads64[key] - ref).max() < 1e-8 * scale + 1e-12, key
        if key in zero:
            assert np.abs(grads64[key]).max() < 1e-6, key
        else:
            worst64 = max(worst64, np.abs(grads64[key] - ref).max() / scale)

    model.train()
    before = {k: v.clone() for k, v in oracle.sd.items() if "running" in k}
    lat = torch.tensor(g["lattice"], dtype=torch.float32).expand(4, 3, 3)
    zs = torch.tensor(g["atomic_numbers"]).expand(4, -1)
    out = model.forward(lat, zs, torch.tensor(pos, dtype=torch.float32))
    torch.nn.MSELoss()(out, torch.tensor(targets, dtype=torch.float32)).backward()
    np.testing.assert_allclose(out.detach().numpy(), o_out, rtol=0, atol=2e-5 * np.abs(o_out).max())
    worst32, worst_ref, failed = 0.0, 0.0, []
    for key, p in model.named_parameters():
        got = p.grad.numpy()
        assert np.isfinite(got).all(), key
        if key in zero:
            assert np.abs(got).max() < 1e-6, key
            continue
        scale = np.abs(grads64[key]).max()
        d_dev = np.abs(got - grads64[key]).max() / scale
        d_ref = np.abs(o_grads32[key] - o_grads[key]).max() / np.abs(o_grads[key]).max()
        checked.add(key)
        worst32, worst_ref = max(worst32, d_dev), max(worst_ref, d_ref)
        if not d_dev < max(2e-4, 3 * d_ref):
            failed.append((key, d_dev, d_ref))
    print(f"training gradients {name} {fn}/{fe}: device f64 vs oracle f64 {worst64:.1e}; vs device f64: device f32 {worst32:.1e}; "
          f"oracle f32 vs oracle f64 {worst_ref:.1e} (max over parameters of max|diff| / max|grad|)")
    assert not failed, failed
    assert all(f"_edge_blocks.{p}.c3_norm_2.bias" in checked for p in range(PASSES))
    # running statistics: torch's own update on the oracle's float32 rows in front of BatchNorm
    stages = {}
    O.forward(oracle, pos, faithful=False, stages=stages, train=True)
    pre = "_to_polarizability_embedding."
    mean, var = before[pre + "1.running_mean"].clone(), before[pre + "1.running_var"].clone()
    torch.nn.functional.batch_norm(O.lin(oracle.sd, pre + "0", stages[f"edge{PASSES}"]), mean, var, None, None, True, 0.1, 1e-5)
    sd = model.state_dict()
    np.testing.assert_allclose(sd[pre + "1.running_mean"].numpy(), mean.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(sd[pre + "1.running_var"].numpy(), var.numpy(), rtol=1e-5, atol=1e-6)
    assert int(sd[pre + "1.num_batches_tracked"]) == 1


# ----------------------------------------------------------------------------- g. input gradients
def _oracle_grads_f32(oracle, pos, lat, zs, v):
    """``tests/test_input_gradients.py: _oracle_grads`` through the float32 oracle: how far float32 autograd itself is from
    the float64 one."""
    from oracle import potgnn_oracle as O
    x = torch.tensor(pos, dtype=torch.float32, requires_grad=True)
    L = torch.tensor(lat, dtype=torch.float32, requires_grad=True)
    out = O.forward(oracle, x, faithful=False, grad=True, lattices=L, atomic_numbers=zs)
    (out * torch.as_tensor(v, dtype=torch.float32)).sum().backward()
    return x.grad.numpy().astype(np.float64), L.grad.numpy().astype(np.float64)


@pytest.mark.parametrize("fn, fe", [(5, 14), (64, 64)])
@pytest.mark.parametrize("name", ["hub17", "molecules33"])
def test_input_gradients_against_autograd(name, fn, fe):
    """pos.grad and lattice.grad of a random cotangent in evaluation mode, a strained lattice per frame: float64 model
    within 1e-9, float32 model within max(5e-5, 3 x the float32 oracle's own distance) of autograd through the float64
    oracle; pos.grad of an atom without edges is exactly zero."""
    g, model, oracle, _ = _case(name, fn, fe)
    model.eval()
    pos, lat, zs = _inputs(g, model, 3, strained=True)
    v = np.random.default_rng(5).standard_normal((3, 6))
    want_pos, want_lat = _oracle_grads(oracle, pos, lat, zs, v)
    ref_pos, ref_lat = _oracle_grads_f32(oracle, pos, lat, zs, v)
    free, _ = _graph(oracle)
    _, gp32, gl32 = _device_grads(model, pos, lat, zs, v)
    model.double()
    _, gp64, gl64 = _device_grads(model, pos, lat, zs, v)
    print(f"input gradients {name} {fn}/{fe}: positions device f64 {_err(gp64, want_pos):.2e}, device f32 {_err(gp32, want_pos):.2e}, "
          f"oracle f32 {_err(ref_pos, want_pos):.2e}; lattice device f64 {_err(gl64, want_lat):.2e}, device f32 "
          f"{_err(gl32, want_lat):.2e}, oracle f32 {_err(ref_lat, want_lat):.2e}")
    for got in (gp32, gl32, gp64, gl64):
        assert torch.isfinite(got).all()
    assert _err(gp64, want_pos) < 1e-9 and _err(gl64, want_lat) < 1e-9
    assert _err(gp32, want_pos) < max(5e-5, 3 * _err(ref_pos, want_pos))
    assert _err(gl32, want_lat) < max(5e-5, 3 * _err(ref_lat, want_lat))
    assert len(free) == SPARSE_PROPERTIES[name]["edge_free"]
    assert np.all(gp32.numpy()[:, free, :] == 0) and np.all(gp64.numpy()[:, free, :] == 0)
