"""Gradients of ``PotGNN.forward`` with respect to the fractional positions and the lattice.

Evaluation mode (``rn_potgnn_forward_vjp_device``: taped forward + one reverse pass per chunk of frames) and training mode
(the step's own reverse pass, ``rn_potgnn_train_backward_inputs(_device)``), against torch autograd through the float64
oracle (which normalises its unit vectors out of place), ``alpha_jacobian``, central differences of the float64 device
forward and ``torch.autograd.gradcheck``.  Needs a real MI355X: run with ``-m gpu``.
"""
import numpy as np
import pytest
import torch

from tests.conftest import load_golden
from tests.helpers import product_model_from_golden
from tests.test_gpu_parity import _random_model

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_default_device_mode():
    """Start from torch's initial state: no default-device mode.  (An earlier module may leave
    ``torch.set_default_device("cpu")`` behind, a mode under which ``torch.as_tensor`` moves CUDA tensors to the host.)"""
    torch.set_default_device(None)
    yield


def _product_case(name):
    from oracle import potgnn_oracle as O
    g = load_golden(name)
    model = product_model_from_golden(g)
    oracle = O.model_from_arrays(g)
    oracle.coefficient = model.gauss_coefficient
    return g, model, oracle


def _case(case, cutoff=None, fn=None, fe=None, passes=2):
    """(fixture, product model in evaluation mode, float32 oracle with the same weights)."""
    if cutoff is None:
        g, model, oracle = _product_case(case)
    else:
        g = load_golden(case)
        model, oracle = _random_model(g, cutoff, fn, fe, passes, seed=fn * 131 + fe)
    return g, model.eval(), oracle


def _inputs(g, model, s, strained=False, mixed=False, seed=3):
    rng = np.random.default_rng(seed)
    base = g["pos_batch"]
    pos = base[rng.integers(0, len(base), size=s)] + rng.normal(scale=2e-3, size=(s,) + base.shape[1:])
    lat = np.broadcast_to(np.asarray(g["lattice"], dtype=np.float64), (s, 3, 3)).copy()
    if strained:  # a general small strain per frame: L (I + eps)
        lat = lat @ (np.eye(3) + 0.02 * rng.standard_normal((s, 3, 3)))
    zs = np.broadcast_to(np.asarray(g["atomic_numbers"]), (s, model.num_atoms)).copy()
    if mixed:  # swap the species of two atoms of different species in every frame but the first
        first = int(np.flatnonzero(zs[0] != zs[0, 0])[0])
        zs[1:, [0, first]] = zs[1:, [first, 0]]
    return pos, lat, zs


def _oracle_grads(oracle, pos, lat, zs, v, train=False, targets=None):
    """(d/dpos, d/dlat) of v . out (or of the MSE loss against ``targets``) by autograd through the float64 oracle."""
    from oracle import potgnn_oracle as O
    o64 = oracle.to(torch.float64)
    x = torch.tensor(pos, dtype=torch.float64, requires_grad=True)
    L = torch.tensor(lat, dtype=torch.float64, requires_grad=True)
    out = O.forward(o64, x, faithful=False, grad=True, train=train, lattices=L, atomic_numbers=zs)
    if targets is None:
        (out * torch.as_tensor(v, dtype=torch.float64)).sum().backward()
    else:
        torch.nn.functional.mse_loss(out, torch.as_tensor(targets, dtype=torch.float64)).backward()
    return x.grad.numpy(), L.grad.numpy()


def _device_grads(model, pos, lat, zs, v, where="cpu", dtype=torch.float64):
    pos_t = torch.tensor(pos, dtype=dtype, device=where, requires_grad=True)
    lat_t = torch.tensor(lat, dtype=dtype, device=where, requires_grad=True)
    out = model(lat_t, torch.tensor(zs, device=where), pos_t)
    assert out.requires_grad
    out.backward(torch.as_tensor(v, dtype=out.dtype, device=out.device))
    return out, pos_t.grad, lat_t.grad


def _err(got, want):
    return np.abs(np.asarray(got) - want).max() / max(np.abs(want).max(), 1e-30)


CASES = [
    ("triclinic20", None, None, None),      # the product model (narrow widths)
    ("tio2_notebook", 5.0, 5, 14),          # 47 neighbours per atom, documented widths
    ("tio2_notebook", 5.0, 64, 64),         # 47 neighbours per atom, fused kernels
    ("rocksalt64_parity", 3.2, 50, 40),
    ("triclinic20", 3.4, 40, 100),          # unfused chain at padded width 128
]


@pytest.mark.parametrize("case, cutoff, fn, fe", CASES)
def test_eval_gradients_against_oracle_autograd(case, cutoff, fn, fe):
    """pos.grad and lattice.grad of a random cotangent: float64 model within 1e-9, float32 model within 5e-5 of the
    float64 oracle's autograd; per-sample strained lattices and mixed species on the product case."""
    g, model, oracle = _case(case, cutoff, fn, fe)
    per_sample = cutoff is None
    pos, lat, zs = _inputs(g, model, 3, strained=per_sample, mixed=per_sample)
    v = np.random.default_rng(5).standard_normal((3, 6))
    want_pos, want_lat = _oracle_grads(oracle, pos, lat, zs, v)
    _, gp32, gl32 = _device_grads(model, pos, lat, zs, v)
    assert gp32.dtype == torch.float64 and gp32.device.type == "cpu" and gl32.shape == (3, 3, 3)
    assert _err(gp32, want_pos) < 5e-5, _err(gp32, want_pos)
    assert _err(gl32, want_lat) < 5e-5, _err(gl32, want_lat)
    model.double()
    _, gp64, gl64 = _device_grads(model, pos, lat, zs, v)
    assert _err(gp64, want_pos) < 1e-9, _err(gp64, want_pos)
    assert _err(gl64, want_lat) < 1e-9, _err(gl64, want_lat)
    # translating every atom together changes nothing
    assert np.abs(gp64.numpy().sum(axis=1)).max() < 1e-9 * np.abs(want_pos).max()


@pytest.mark.parametrize("case, cutoff, fn, fe", [CASES[0], CASES[2]])
def test_one_hot_cotangents_reproduce_alpha_jacobian(case, cutoff, fn, fe):
    """Six copies of one frame with the six one-hot cotangents give the rows of ``alpha_jacobian(float64=True)``."""
    g, model, _ = _case(case, cutoff, fn, fe)
    model.double()
    pos = np.repeat(g["pos_batch"][1][None], 6, axis=0)
    lat = np.broadcast_to(np.asarray(g["lattice"], dtype=np.float64), (6, 3, 3)).copy()
    zs = np.broadcast_to(np.asarray(g["atomic_numbers"]), (6, model.num_atoms)).copy()
    _, gp, _ = _device_grads(model, pos, lat, zs, np.eye(6))
    jac = model.alpha_jacobian(g["pos_batch"][1], float64=True)
    assert np.abs(gp.numpy() - jac).max() < 1e-12 * np.abs(jac).max(), _err(gp.numpy(), jac)


def test_chunking_and_repeated_backward():
    """S = 11 through a handle whose work chunk is 4 frames agrees with one chunk; two identical backward calls agree."""
    from ramannoodle_amd.pmodel import PotGNN
    g, model, _ = _case("tio2_notebook", 5.0, 5, 14)
    small = PotGNN(model._ref_structure, 5.0, 5, 14, 2, 0.0, 5.0, model._mean_polarizability,
                   model._stddev_polarizability, max_chunk_structures=4)
    small.load_state_dict(model.state_dict())
    model.double()
    small.eval().double()
    pos, lat, zs = _inputs(g, model, 11, strained=True)
    v = np.random.default_rng(8).standard_normal((11, 6))
    _, gp1, gl1 = _device_grads(model, pos, lat, zs, v)
    _, gp2, gl2 = _device_grads(model, pos, lat, zs, v)
    _, gp4, gl4 = _device_grads(small, pos, lat, zs, v)
    for a, b in ((gp1, gp4), (gl1, gl4), (gp1, gp2), (gl1, gl2)):
        assert _err(a.numpy(), b.numpy()) < 1e-13, _err(a.numpy(), b.numpy())


def test_lattice_gradient_matches_strain_central_differences():
    """Clamped-ion strain derivative: sum_ij (lattice.grad)_ij (L E)_ij against central differences of the float64 device
    forward on L (I +- h E), fractional positions fixed."""
    g, model, _ = _case("triclinic20", 3.4, 40, 100)
    model.double()
    pos, lat, zs = _inputs(g, model, 2, strained=True, seed=11)
    v = np.random.default_rng(12).standard_normal((2, 6))
    _, _, gl = _device_grads(model, pos, lat, zs, v)
    rng = np.random.default_rng(13)
    h = 1e-6  # (the Gaussian basis at Fe = 100 is 0.05 A wide: h = 1e-5 leaves an O(h^2) error of 1e-6)
    for _ in range(3):
        E = rng.standard_normal((3, 3))
        want = float(np.einsum("sij,sij->", gl.numpy(), lat @ E))
        with torch.no_grad():
            plus = model(torch.tensor(lat @ (np.eye(3) + h * E)), torch.tensor(zs), torch.tensor(pos)).numpy()
            minus = model(torch.tensor(lat @ (np.eye(3) - h * E)), torch.tensor(zs), torch.tensor(pos)).numpy()
        fd = float(np.sum(v * (plus - minus)) / (2 * h))
        assert abs(fd - want) < 1e-6 * max(abs(want), 1e-12), (fd, want)


def test_gradcheck_positions_and_lattice():
    """``torch.autograd.gradcheck`` on a small float64 model, with respect to positions and lattice."""
    g, model, _ = _case("triclinic20", 3.0, 16, 12)
    model.double()
    pos, lat, zs = _inputs(g, model, 2, strained=True, seed=21)
    zs_t = torch.tensor(zs)

    def fn(p, L):
        return model(L, zs_t, p)

    p = torch.tensor(pos, dtype=torch.float64, requires_grad=True)
    L = torch.tensor(lat, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(fn, (p, L), eps=1e-6, atol=1e-6, rtol=1e-4, nondet_tol=1e-12)


def test_cuda_inputs_stay_on_device_and_respect_the_stream():
    """CUDA inputs give CUDA gradients (an expanded lattice gets the sum); a cotangent written on the current stream behind
    a long kernel is read only after that kernel (the backward is ordered on that stream)."""
    from tests.test_async_entries import _check_window, _open_window
    g, model, _ = _case("tio2_notebook", 5.0, 64, 64)
    pos, _, zs = _inputs(g, model, 4)
    v = np.random.default_rng(2).standard_normal((4, 6))
    lat0 = torch.tensor(np.asarray(g["lattice"], dtype=np.float64))
    want_p, want_l = [], []
    for where in ("cpu", "cuda"):
        base = lat0.clone().to(where).requires_grad_(True)
        p = torch.tensor(pos, device=where, requires_grad=True)
        out = model(base.expand(4, 3, 3), torch.tensor(zs, device=where), p)
        assert out.device.type == where
        out.backward(torch.tensor(v, dtype=out.dtype, device=where))
        assert p.grad.device.type == where and base.grad.device.type == where and base.grad.shape == (3, 3)
        want_p.append(p.grad.cpu().numpy())
        want_l.append(base.grad.cpu().numpy())
    # (a float32 model: the reverse pass accumulates with float atomics, so two backward calls agree to rounding)
    np.testing.assert_allclose(want_p[1], want_p[0], rtol=0, atol=1e-5 * np.abs(want_p[0]).max())
    np.testing.assert_allclose(want_l[1], want_l[0], rtol=0, atol=1e-5 * np.abs(want_l[0]).max())

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        p = torch.tensor(pos, device="cuda", requires_grad=True)
        out = model(lat0.cuda().expand(4, 3, 3), torch.tensor(zs, device="cuda"), p)
        cot = torch.zeros_like(out)
    start, end = _open_window(stream)
    with torch.cuda.stream(stream):
        cot.copy_(torch.tensor(v, dtype=out.dtype, device="cuda"))  # behind the sleep
        out.backward(cot)
        got = p.grad.clone()
    torch.cuda.synchronize()
    _check_window(start, end, 1.0)
    np.testing.assert_allclose(got.cpu().numpy(), want_p[1], rtol=0, atol=1e-5 * np.abs(want_p[1]).max())


def _same_as_plain_step(plain, with_inputs, plain_again, what):
    """The parameter gradients of a step with input gradients are those of the plain step.  The reverse pass sums the
    LayerNorm / BatchNorm parameter gradients with float atomics, so even two plain steps agree there only to rounding:
    those must agree within that noise; every other gradient that two plain steps reproduce bit for bit must come out
    bit for bit."""
    spread = float((plain_again - plain).abs().max())
    diff = float((with_inputs - plain).abs().max())
    atomics = "norm" in what or what.startswith("_to_polarizability_embedding.1.") or what == "device gradient buffer"
    if spread == 0.0 and not atomics:
        assert diff == 0.0, (what, diff)
    else:
        assert diff <= max(4.0 * spread, 1e-5 * float(plain.abs().max())), (what, diff, spread)


def _train_case():
    from tests.test_gpu_parity import _load_train_case
    from oracle import potgnn_oracle as O
    g, model, lat, zs, pos = _load_train_case()
    oracle = O.model_from_arrays(g)
    oracle.coefficient = model.gauss_coefficient
    return g, model, oracle, lat, zs, pos


@pytest.mark.parametrize("where", ["cpu", "cuda"])
def test_training_step_input_gradients(where):
    """Training mode, host arrays path: parameter gradients bit-identical with and without positions.requires_grad;
    positions.grad and lattice.grad against oracle autograd with batch-statistics BatchNorm."""
    g, model, oracle, lat, zs, pos = _train_case()
    targets = torch.tensor(g["train/target"])
    model.train()
    grads = []
    for want_inputs in (False, True, False):
        model.zero_grad()
        p = pos.clone().to(where).requires_grad_(want_inputs)
        L = lat.clone().to(where).requires_grad_(want_inputs)
        loss = torch.nn.MSELoss()(model(L, zs.to(where), p), targets.to(where))
        loss.backward()
        if want_inputs:
            p_in, L_in = p, L
        grads.append({k: q.grad.detach().cpu().clone() for k, q in model.named_parameters()})
    for k in grads[0]:
        _same_as_plain_step(grads[0][k], grads[1][k], grads[2][k], k)
    p, L = p_in, L_in
    assert p.grad.device.type == where and p.grad.dtype == torch.float32 and L.grad.shape == lat.shape
    want_pos, want_lat = _oracle_grads(oracle, pos.numpy(), lat.numpy(), zs.numpy(), None, train=True,
                                       targets=g["train/target"])
    assert _err(p.grad.cpu().numpy(), want_pos) < 1.5e-4, _err(p.grad.cpu().numpy(), want_pos)
    assert _err(L.grad.cpu().numpy(), want_lat) < 1.5e-4, _err(L.grad.cpu().numpy(), want_lat)


@pytest.mark.parametrize("where", ["cpu", "cuda"])
def test_device_adam_step_input_gradients(where):
    """``DeviceAdam`` (gradients in HBM): host tensors take ``_TrainStep``, CUDA tensors ``_TrainStepOnDevice``; the
    device gradient buffer is bit-identical with and without positions.requires_grad, positions.grad matches autograd."""
    from ramannoodle_amd.pmodel import DeviceAdam
    g, model, oracle, lat, zs, pos = _train_case()
    targets = torch.tensor(g["train/target"])
    DeviceAdam(model, lr=1e-3)
    model.train()
    grads = []
    for want_inputs in (False, True, False):
        q = pos.clone().to(where).requires_grad_(want_inputs)
        loss = torch.nn.MSELoss()(model(lat.to(where), zs.to(where), q), targets.to(where))
        loss.backward()
        torch.cuda.synchronize()
        if want_inputs:
            p = q
        grads.append(model.device_gradients().clone())
    _same_as_plain_step(grads[0], grads[1], grads[2], "device gradient buffer")
    assert p.grad.device.type == where
    want_pos, _ = _oracle_grads(oracle, pos.numpy(), lat.numpy(), zs.numpy(), None, train=True,
                                targets=g["train/target"])
    assert _err(p.grad.cpu().numpy(), want_pos) < 1.5e-4, _err(p.grad.cpu().numpy(), want_pos)


def test_no_grad_paths_unchanged_and_double_backward_raises():
    """Without an input requiring grad, or under ``torch.no_grad()``, ``forward`` takes the plain evaluation: the same bits
    and no graph; the value with input gradients is the same bits too; a second backward through it raises."""
    for dtype in (torch.float32, torch.float64):
        g, model, _ = _case("tio2_notebook", 5.0, 5, 14)
        if dtype == torch.float64:
            model.double()
        pos, lat, zs = _inputs(g, model, 3, strained=True)
        for where in ("cpu", "cuda"):
            args = (torch.tensor(lat, device=where), torch.tensor(zs, device=where), torch.tensor(pos, device=where))
            plain = model(*args)
            assert not plain.requires_grad and plain.grad_fn is None
            p = args[2].clone().requires_grad_(True)
            with torch.no_grad():
                quiet = model(args[0], args[1], p)
            assert not quiet.requires_grad
            traced = model(args[0], args[1], p)
            assert traced.requires_grad
            for other in (quiet, traced.detach()):
                assert torch.equal(other, plain)
            (gp,) = torch.autograd.grad(traced, p, torch.ones_like(traced), create_graph=True)
            with pytest.raises(RuntimeError):
                gp.sum().backward()


def test_eval_backward_voids_a_pending_training_step():
    """An evaluation-mode backward reuses lane 0 and the tape: the backward of a training step whose forward ran before it
    raises ``ValueError``."""
    g, model, _, lat, zs, pos = _train_case()
    model.train()
    pending = model(lat, zs, pos)
    model.eval()
    p = pos.clone().double().requires_grad_(True)
    model(lat.double(), zs, p).sum().backward()
    assert p.grad is not None
    with pytest.raises(ValueError, match="preceding train_forward"):
        pending.sum().backward()
