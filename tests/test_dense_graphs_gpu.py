"""Every kernel family on dense and very uneven graphs, up to the degree caps, forward and reverse.

tests/test_sparse_graphs_gpu.py covers graphs with too little in them; ``tests/helpers.py: dense_structures()`` has four
with a lot: a complete 56-atom ball among two- and three-atom molecules (degree 55 beside degree 1 in every 16-atom group:
the atom-owning NodeBlock refused, no reverse partition at 64 wide), the smallest such ball the role-specialised
EdgeBlock's ring refuses while the fused path stays on, and two hubs whose degree is exactly the largest the library
accepts at a padded edge width of 128 and of 64 (one-atom tiles sized to the limit of the CU's LDS in float64; above 128
rows the narrow kernels' four-wave form).  tests/test_host_logic.py pins the graphs, asserts those planner branches by
name and that every kernel of every plan fits the CU; here the kernels run, against the float64 oracle, with the bounds
of the sparse file.  Nothing above a cap reaches a device: those cases are host-side refusals.  Needs a real MI355X: run
with ``-m gpu``.
"""
import numpy as np
import pytest
import torch

from ramannoodle_amd import _lib
from tests.helpers import DENSE_PROPERTIES, dense_fixture
from tests.test_gpu_parity import REL, _random_model, _rel_err
from tests.test_host_logic import _dense_plan
from tests.test_input_gradients import _device_grads, _err, _inputs, _oracle_grads
from tests.test_input_gradients import _no_default_device_mode  # noqa: F401  (autouse: no default-device mode in here)
from tests.test_sparse_graphs_gpu import _forward_check, _oracle_grads_f32, _standardised

pytestmark = pytest.mark.gpu

NAMES = list(DENSE_PROPERTIES)
PASSES = 2


def _case(name, fn, fe, frames=3):
    """(fixture-like dict, product model, float32 oracle, float64 oracle) of one structure at one width pair."""
    g, cutoff = dense_fixture(name, frames=frames)
    model, oracle = _random_model(g, cutoff, fn, fe, PASSES, seed=fn * 1000 + fe + NAMES.index(name))
    assert (model.num_atoms, model.num_edges, oracle.num_triplets) == tuple(DENSE_PROPERTIES[name][k] for k in "NET")
    return g, model, oracle, oracle.to(torch.float64)


def _flags_match_the_plan(model, name, fn, fe):
    flags, plan = model.config_flags(), _dense_plan(_lib.load(), name, fn, fe)
    assert flags["fused_edge_block"] == bool(plan["use_fused"]), (flags, name, fn, fe)
    assert flags["role_split_edge_block"] == bool(plan["use_fused"] and plan["use_ps"]), (flags, name, fn, fe)
    assert flags["narrow_kernels"] == bool(plan["use_narrow"]), (flags, name, fn, fe)
    assert flags["atom_owning_node_block"] == bool(plan["use_fused"] and plan["use_node_fused"] and plan["na_num"] > 0), (flags, name, fn, fe)
    return flags


# ----------------------------------------------------------------------------- a. forward
@pytest.mark.parametrize("name, fn, fe", [(name, fn, fe) for name in NAMES
                                          for fn, fe in ((5, 14), (13, 9), (64, 64), (40, 50), (24, 20), (8, 20))]
                         + [(name, fn, fe) for name in ("blob_gas", "hub_cap128") for fn, fe in ((40, 100), (64, 128))])
def test_forward_against_the_float64_oracle(name, fn, fe):
    """Two passes on three frames: standardised output within 1e-5 of the float64 oracle, a second evaluation bit-identical,
    frame 0 alone bit-identical to frame 0 of the batch, and the kernel family the handle reports is the one the host-only
    plan names -- on ``blob_ring`` at 64 wide the fused path without the role-specialised EdgeBlock, no knob set.  40/100
    and 64/128 (padded 64/128, cap 71) take the ball of 56 and the hub of 71 only: the other two are refused there."""
    g, model, _, oracle64 = _case(name, fn, fe)
    _forward_check(model, oracle64, g["pos_batch"], (name, fn, fe))
    flags = _flags_match_the_plan(model, name, fn, fe)
    if name == "blob_ring" and (fn, fe) in ((64, 64), (40, 50), (24, 20)):
        assert flags["fused_edge_block"] and not flags["role_split_edge_block"]
    if (fn, fe) in ((5, 14), (13, 9)):
        assert flags["narrow_kernels"]


# ----------------------------------------------------------------------------- b. kernel choices at 64/64
@pytest.mark.parametrize("knob, value, flag, state", [
    ("RN_POTGNN_EDGE_PS", "0", "role_split_edge_block", False),
    ("RN_POTGNN_NODE_ATOM", "0", "atom_owning_node_block", False),
    ("RN_POTGNN_NODE_ATOM", "1", "atom_owning_node_block", True),
    ("RN_POTGNN_FUSED", "0", "fused_edge_block", False),
])
@pytest.mark.parametrize("name", ["blob_gas", "blob_ring"])
def test_wide_kernel_choices_against_the_float64_oracle(monkeypatch, name, knob, value, flag, state):
    """64/64 without the role-specialised EdgeBlock, with the row-ordered and with the (here refused by default)
    atom-owning NodeBlock -- rounds of 55 or 65 in-edges beside atoms with one --, and on the unfused chain."""
    monkeypatch.setenv(knob, value)
    g, model, _, oracle64 = _case(name, 64, 64)
    _forward_check(model, oracle64, g["pos_batch"], (name, knob, value))
    assert model.config_flags()[flag] == state, model.config_flags()


# ----------------------------------------------------------------------------- c. stages
@pytest.mark.parametrize("fn, fe", [(64, 64), (5, 14)])
@pytest.mark.parametrize("name", ["blob_gas", "hub_cap64"])
def test_stages_row_by_row(monkeypatch, name, fn, fe):
    """Node and edge rows after the embedding and after each pass against the float32 oracle (atol 2e-5): an error shows
    at its row -- a molecule's atom of degree 1 beside the ball's of degree 55, or the hub's one-atom tile of 147 rows."""
    from oracle import potgnn_oracle as O
    monkeypatch.setenv("RN_POTGNN_KEEP_STAGES", "1")
    g, model, oracle, _ = _case(name, fn, fe, frames=2)
    pos = g["pos_batch"]
    s = pos.shape[0]
    model.eval()
    model.forward(torch.tensor(g["lattice"]).expand(s, 3, 3), torch.tensor(g["atomic_numbers"]).expand(s, -1), torch.tensor(pos))
    stages = {}
    O.forward(oracle, pos, faithful=False, stages=stages)
    degree = np.bincount(oracle.edges[1].numpy(), minlength=model.num_atoms)
    for p in range(PASSES + 1):
        node_ref, edge_ref = stages[f"node{p}"].numpy(), stages[f"edge{p}"].numpy()
        node, edge = model.debug_stage(1, p), model.debug_stage(2, p)
        assert node.shape == node_ref.shape and edge.shape == edge_ref.shape, (p, node.shape, edge.shape)
        worst = np.abs(node - node_ref).max(axis=1).reshape(s, -1).max(axis=0)
        print(f"stages {name} {fn}/{fe} pass {p}: node rows {worst.max():.1e} (atom {worst.argmax()}, degree {degree[worst.argmax()]}), "
              f"edge rows {np.abs(edge - edge_ref).max():.1e}")
        np.testing.assert_allclose(node, node_ref, rtol=0, atol=2e-5, err_msg=f"node{p}")
        np.testing.assert_allclose(edge, edge_ref, rtol=0, atol=2e-5, err_msg=f"edge{p}")


# ----------------------------------------------------------------------------- d. float64 evaluation
@pytest.mark.parametrize("name, fn, fe", [(name, fn, fe) for name in NAMES for fn, fe in ((64, 64), (5, 14))] + [("hub_cap128", 64, 128)])
def test_float64_evaluation_against_the_float64_oracle(name, fn, fe):
    """The kernels instantiated for ``double`` within 1e-9 of the float64 oracle, on the polarizabilities and on their
    standardised part.  ``hub_cap64`` at 64/64 and ``hub_cap128`` at 64/128 are the tiles at the cap: 163008 and 162320 of
    the CU's 163840 bytes."""
    from oracle import potgnn_oracle as O
    g, model, _, oracle64 = _case(name, fn, fe)
    pos = g["pos_batch"]
    got = model.calc_polarizabilities(pos, dtype=torch.float64)
    want = O.calc_polarizabilities(oracle64, pos, faithful=False)
    err = _rel_err(_standardised(got, oracle64), _standardised(want, oracle64))
    print(f"float64 forward {name} {fn}/{fe}: device f64 vs oracle f64 {err:.2e} (standardised), {_rel_err(got, want):.2e}")
    assert np.isfinite(got).all()
    assert _rel_err(got, want) < 1e-9 and err < 1e-9, (name, fn, fe, err)
    np.testing.assert_array_equal(model.calc_polarizabilities(pos, dtype=torch.float64), got)


# ----------------------------------------------------------------------------- e. reverse-mode Jacobian
@pytest.mark.parametrize("fn, fe", [(5, 14), (64, 64), (24, 20), (8, 20)])
@pytest.mark.parametrize("name", ["blob_gas", "hub_cap128", "hub_cap64"])
def test_reverse_mode_jacobian_against_autograd(name, fn, fe):
    """d(vec6)/d(r) in float64 within 1e-9 of autograd through the float64 oracle (of the largest entry), translation
    invariant.  At 64 wide these graphs have no reverse partition (the forward tiles serve, one atom each at the cap); at
    the narrow widths they have one."""
    from oracle import potgnn_oracle as O
    g, model, _, oracle64 = _case(name, fn, fe)
    plan = _dense_plan(_lib.load(), name, fn, fe)
    if plan["FeP"] == 64:
        assert len(plan["bt"][0]) == 0, (name, fn, fe, plan["bt"][1])
    if (fn, fe) == (5, 14):
        assert len(plan["bt"][0]) > 0, (name, fn, fe)
    pos = g["pos_batch"][1]
    want = O.jacobian(oracle64, pos)
    scale = np.abs(want).max()
    assert np.isfinite(want).all() and scale > 0
    got64 = model.alpha_jacobian(pos, float64=True)
    d64 = np.abs(got64 - want).max() / scale
    print(f"jacobian {name} {fn}/{fe}: device f64 {d64:.2e} (of max |J|, vs oracle f64)")
    assert np.isfinite(got64).all()
    assert d64 < 1e-9, d64
    assert np.abs(got64.sum(axis=1)).max() < 1e-9 * scale


# ----------------------------------------------------------------------------- f. training gradients
@pytest.mark.parametrize("fn, fe", [(5, 14), (64, 64)])
@pytest.mark.parametrize("name", ["blob_gas", "hub_cap128"])
def test_training_gradients_against_autograd(name, fn, fe):
    """One training step on two frames with random targets.  float64 device step against float64 autograd through the
    oracle: outputs, loss and every parameter within 1e-9 (of the parameter's largest gradient).  float32 step against the
    float64 device gradients: per parameter within max(2e-4, 3 x the float32 oracle's own distance from the float64 oracle
    for that parameter)."""
    from oracle import potgnn_oracle as O
    g, model, oracle, oracle64 = _case(name, fn, fe, frames=2)
    pos = g["pos_batch"]
    targets = np.random.default_rng(8).normal(size=(2, 6))
    o_out, o_loss, o_grads = O.train_gradients(oracle64, pos, targets)
    _, _, o_grads32 = O.train_gradients(oracle, pos, targets)
    assert all(np.isfinite(v).all() for v in o_grads.values())
    zero = sorted(k for k, v in o_grads.items() if np.abs(v).max() < 1e-12)
    assert zero == ["_to_polarizability_embedding.0.bias"]  # (the bias in front of BatchNorm never has a gradient)

    out64, loss64, grads64 = model.train_gradients_f64(pos, targets)
    np.testing.assert_allclose(out64, o_out, rtol=0, atol=1e-9 * np.abs(o_out).max())
    assert loss64 == pytest.approx(o_loss, rel=1e-9)
    worst64 = 0.0
    for key, ref in o_grads.items():
        scale = np.abs(ref).max()
        assert np.isfinite(grads64[key]).all(), key
        if key in zero:
            assert np.abs(grads64[key]).max() < 1e-6, key
            continue
        worst64 = max(worst64, np.abs(grads64[key] - ref).max() / scale)
        assert np.abs(grads64[key] - ref).max() < 1e-9 * scale, (key, np.abs(grads64[key] - ref).max() / scale)

    model.train()
    lat = torch.tensor(g["lattice"], dtype=torch.float32).expand(2, 3, 3)
    zs = torch.tensor(g["atomic_numbers"]).expand(2, -1)
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
        worst32, worst_ref = max(worst32, d_dev), max(worst_ref, d_ref)
        if not d_dev < max(2e-4, 3 * d_ref):
            failed.append((key, d_dev, d_ref))
    print(f"training gradients {name} {fn}/{fe}: device f64 vs oracle f64 {worst64:.1e}; vs device f64: device f32 {worst32:.1e}; "
          f"oracle f32 vs oracle f64 {worst_ref:.1e} (max over parameters of max|diff| / max|grad|)")
    assert not failed, failed


# ----------------------------------------------------------------------------- g. input gradients
@pytest.mark.parametrize("fn, fe", [(5, 14), (64, 64)])
@pytest.mark.parametrize("name", ["blob_gas", "hub_cap128"])
def test_input_gradients_against_autograd(name, fn, fe):
    """pos.grad and lattice.grad of a random cotangent in evaluation mode, a strained lattice per frame: float64 model
    within 1e-9, float32 model within max(5e-5, 3 x the float32 oracle's own distance) of autograd through the float64
    oracle."""
    g, model, oracle, _ = _case(name, fn, fe)
    model.eval()
    pos, lat, zs = _inputs(g, model, 2, strained=True)
    v = np.random.default_rng(5).standard_normal((2, 6))
    want_pos, want_lat = _oracle_grads(oracle, pos, lat, zs, v)
    ref_pos, ref_lat = _oracle_grads_f32(oracle, pos, lat, zs, v)
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
