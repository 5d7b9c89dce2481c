"""The to-device entry (``calc_polarizabilities_to_device``) returns with its copies and kernels still enqueued.  These
tests hold a stream open with a bounded spin kernel (``torch.cuda._sleep``) so that the call's work is still pending
when the next thing happens, and check that

* the call waits for work queued earlier on the caller's stream (a reader of the ``out`` it is about to overwrite);
* every other entry point of the handle can be called right behind it, with no synchronisation in between, without
  disturbing its result or its own;
* a caller's ``out`` tensor is validated before anything reaches the library.

Every "want" value comes from synchronous calls made beforehand; the entries are deterministic, so comparisons are
bit-exact, except where a reverse pass sums with atomics (Jacobian, analytic Raman tensors, the gradients of a training
step): those agree to round-off.  The float32 results themselves are anchored to the golden fixture or the float64
oracle.  Each test runs its sequence once: no loops, no retries.  Two models: ``rocksalt64_parity`` at 64 / 64 (the wide
role-split kernels) and ``tio2_notebook`` at its own 5 / 14 (the narrow kernels)."""
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from tests.conftest import ROOT, load_golden
from tests.helpers import product_model_from_golden

pytestmark = pytest.mark.gpu

REL = 1e-5
CASES = ["rocksalt64_parity", "tio2_notebook"]


def _rel_err(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@functools.lru_cache(maxsize=None)
def _sleep_cycles():
    """``torch.cuda._sleep`` cycles for about 150 ms on this device (at most 500 ms), timed once with CUDA events."""
    torch.cuda.synchronize()
    torch.cuda._sleep(1000)  # (loads the kernel)
    probe, rates = 2_000_000, []
    for _ in range(2):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        torch.cuda._sleep(probe)
        end.record()
        end.synchronize()
        rates.append(probe / max(start.elapsed_time(end), 1e-3))  # cycles per ms
    return int(min(150.0 * rates[-1], 500.0 * min(rates)))


def _open_window(stream):
    """Queue the sleep on ``stream``; the events around it tell afterwards how long it held the stream."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        start.record()
        torch.cuda._sleep(_sleep_cycles())
        end.record()
    return start, end


def _check_window(start, end, eval_ms):
    """The window proves something only if it stayed open far longer than the evaluation takes."""
    slept = start.elapsed_time(end)
    assert slept <= 2000.0, f"the sleep held the stream {slept:.0f} ms"
    assert slept >= 10.0 * eval_ms, f"the sleep held the stream {slept:.1f} ms, an evaluation takes {eval_ms:.2f} ms"
    return slept


def _sync_eval_ms(model, pos):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.calc_polarizabilities(pos)
    return 1e3 * (time.perf_counter() - t0)


def _case(name):
    """(model, posA, posB) with posA's float32 result anchored to the fixture / the float64 oracle."""
    from oracle import potgnn_oracle as O
    g = load_golden(name)
    posA = np.ascontiguousarray(g["pos_batch"], dtype=np.float64)
    rng = np.random.default_rng(7)
    posB = np.ascontiguousarray((posA[::-1] + 1e-2 * rng.standard_normal(posA.shape)) % 1.0)
    if name == "rocksalt64_parity":
        from tests.test_gpu_parity import _random_model
        model, oracle = _random_model(g, 3.2, 64, 64, 2, seed=64 * 13 + 64)
        got = model.calc_polarizabilities(posA[:2])
        want = O.calc_polarizabilities(oracle, posA[:2], faithful=False)
        assert _rel_err((got - oracle.mean) / oracle.std, (want - oracle.mean) / oracle.std) < REL
        assert model.config_flags()["role_split_edge_block"]
    else:
        model = product_model_from_golden(g)
        assert _rel_err(model.calc_polarizabilities(posA), g["f32/alpha"]) < REL
        assert model.config_flags()["narrow_kernels"]
    return model, posA, posB, g


# ----------------------------------------------------------------------------- (a) the caller's stream
@pytest.mark.parametrize("where", ["side_stream", "default_stream"])
@pytest.mark.parametrize("case", CASES)
def test_to_device_waits_for_earlier_work_on_the_callers_stream(case, where):
    """A reader of ``out`` queued on the caller's stream before the call (here ``out.clone()`` behind the sleep, as the
    previous all-gather of a sharded run would be) sees the old values: the call's kernels wait for it."""
    model, posA, posB, _ = _case(case)
    wantA, wantB = model.calc_polarizabilities(posA), model.calc_polarizabilities(posB)
    out = model.calc_polarizabilities_to_device(posA)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), wantA)
    eval_ms = _sync_eval_ms(model, posA)
    stream = torch.cuda.Stream() if where == "side_stream" else torch.cuda.default_stream()
    start, end = _open_window(stream)
    with torch.cuda.stream(stream):
        snap = out.clone()
        again = model.calc_polarizabilities_to_device(posB, out=out)
    torch.cuda.synchronize()
    slept = _check_window(start, end, eval_ms)
    assert again is out
    np.testing.assert_array_equal(snap.cpu().numpy(), wantA, err_msg=(
        f"a reader queued before the call saw the call's result (sleep {slept:.0f} ms, evaluation {eval_ms:.2f} ms)"))
    np.testing.assert_array_equal(out.cpu().numpy(), wantB)


# ----------------------------------------------------------------------------- (b) entries behind an unfinished call
def _lattices(model, s, strained):
    lat = np.broadcast_to(np.asarray(model._ref_structure.lattice, dtype=np.float64), (s, 3, 3)).copy()
    if strained:
        lat *= 1.0 + 0.01 * np.arange(1, s + 1)[:, None, None]
    return torch.tensor(lat)


def _species(model, s, swapped):
    zs = np.broadcast_to(np.asarray(model._ref_structure.atomic_numbers), (s, model.num_atoms)).copy()
    if swapped:
        first = int(np.flatnonzero(zs[0] != zs[0, 0])[0])  # an atom of the other species
        zs[1:, [0, first]] = zs[1:, [first, 0]]
    return torch.tensor(zs)


def _forward(model, pos, strained=False, swapped=False):
    s = pos.shape[0]
    return model.forward(_lattices(model, s, strained), _species(model, s, swapped), torch.tensor(pos)).numpy()


def _raman_args(pos):
    disp = np.random.default_rng(3).standard_normal((max(1, pos.shape[0] // 2),) + pos.shape[1:])
    return pos[0], disp / np.linalg.norm(disp, axis=(1, 2), keepdims=True)


def _async(model, pos):
    out = np.empty((pos.shape[0], 3, 3), dtype=np.float64)
    model.calc_polarizabilities_async(pos, out)
    model.wait()
    return out


def _device(model, pos):
    out = model.calc_polarizabilities_device(torch.tensor(pos, device=torch.device("cuda", model.device_index)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _train_step(model, opt, pos):
    """One step of device-resident training from host tensors: taped forward, backward, ``DeviceAdam``."""
    model.train()
    s = pos.shape[0]
    out = model.forward(_lattices(model, s, False), _species(model, s, False), torch.tensor(pos))
    loss = (out.double() ** 2).mean()
    loss.backward()
    opt.step()
    opt.zero_grad()
    model.eval()
    return out.detach().numpy(), float(loss.detach())


# name -> (call(model, pos), exact).  "_f64" runs the model with float64 parameters (the forward in double).
FOLLOW_UPS = {
    "calc_polarizabilities": (lambda m, p: m.calc_polarizabilities(p), True),
    "calc_polarizabilities_f64": (lambda m, p: m.calc_polarizabilities(p, dtype=torch.float64), True),
    "forward": (lambda m, p: _forward(m, p), True),
    "forward_lattices": (lambda m, p: _forward(m, p, strained=True), True),
    "forward_species": (lambda m, p: _forward(m, p, swapped=True), True),
    "forward_f64": (lambda m, p: _forward(m, p), True),
    "forward_lattices_f64": (lambda m, p: _forward(m, p, strained=True), True),
    "forward_species_f64": (lambda m, p: _forward(m, p, swapped=True), True),
    "raman_tensors": (lambda m, p: m.calc_raman_tensors(*_raman_args(p)), True),
    "raman_tensors_analytic": (lambda m, p: m.calc_raman_tensors(*_raman_args(p), method="analytic"), False),
    "alpha_jacobian": (lambda m, p: m.alpha_jacobian(p[0], float64=False), False),
    "calc_polarizabilities_async": (_async, True),
    "calc_polarizabilities_device": (_device, True),
    "training_step": (None, None),
}
HOST_F32_OFF = "calc_polarizabilities[RN_POTGNN_HOST_F32=0]"


def _prime(model, pos, follow_up, opt=None):
    """One call of each entry the sequence uses, on a larger batch than the sequence's: no device buffer grows (and no
    hipFree synchronises the device) inside the window."""
    big = np.concatenate([pos, pos])
    model.calc_polarizabilities_to_device(big)
    model.calc_polarizabilities(big)
    if follow_up == "training_step":
        lr = opt.param_groups[0]["lr"]
        opt.param_groups[0]["lr"] = 0.0  # (moments, mask and step staging are set up; the weights stay as they are)
        _train_step(model, opt, big)
        opt.param_groups[0]["lr"] = lr
    else:
        FOLLOW_UPS[follow_up][0](model, big)
    torch.cuda.synchronize()


def _behind_unfinished(case, follow_up):
    """On a side stream: the sleep, then ``out = to_device(posA)`` (whose kernels now wait behind the sleep).  Then, on
    torch's default stream and with nothing synchronised, the follow-up with other positions.  Both results must be
    what each gives on a quiet handle."""
    from ramannoodle_amd.pmodel import DeviceAdam
    model, posA, posB, _ = _case(case)
    if follow_up.endswith("_f64"):
        model.double()
    opt = DeviceAdam(model, lr=1e-4) if follow_up == "training_step" else None
    _prime(model, posB, follow_up, opt)
    wantA = model.calc_polarizabilities(posA)
    eval_ms = _sync_eval_ms(model, posA)
    if follow_up == "training_step":
        twin, _, _, _ = _case(case)
        twin_opt = DeviceAdam(twin, lr=1e-4)
        _prime(twin, posB, follow_up, twin_opt)
        twin.calc_polarizabilities_to_device(posA)
        torch.cuda.synchronize()
        want_vec6, want_loss = _train_step(twin, twin_opt, posB)
        want_state = {k: v.detach().clone() for k, v in twin.state_dict().items()}
    else:
        call, exact = FOLLOW_UPS[follow_up]
        want = call(model, posB)
    side = torch.cuda.Stream()
    start, end = _open_window(side)
    with torch.cuda.stream(side):
        out = model.calc_polarizabilities_to_device(posA)
    if follow_up == "training_step":
        got_vec6, got_loss = _train_step(model, opt, posB)
    else:
        got = call(model, posB)
    torch.cuda.synchronize()
    slept = _check_window(start, end, eval_ms)
    np.testing.assert_array_equal(out.cpu().numpy(), wantA, err_msg=(
        f"the unfinished to-device call was disturbed by {follow_up} (sleep {slept:.0f} ms, evaluation {eval_ms:.2f} ms)"))
    if follow_up == "training_step":
        np.testing.assert_array_equal(got_vec6, want_vec6)
        assert got_loss == want_loss
        # (the weight gradients are summed with atomics, and where a gradient is mathematically zero Adam integrates that
        #  rounding noise divided by its own size: the two steps agree to the size of a step, lr)
        for key, ref in want_state.items():
            got_w = model.state_dict()[key].cpu().numpy()
            assert np.isfinite(got_w).all(), key
            np.testing.assert_allclose(got_w, ref.cpu().numpy(), rtol=0, atol=2 * opt.param_groups[0]["lr"], err_msg=key)
    elif exact:
        np.testing.assert_array_equal(got, want)
    else:
        assert np.isfinite(got).all() and _rel_err(got, want) < 1e-6, follow_up


@pytest.mark.parametrize("follow_up", list(FOLLOW_UPS) + [HOST_F32_OFF])
@pytest.mark.parametrize("case", CASES)
def test_host_entries_behind_an_unfinished_to_device_call(case, follow_up):
    """Every entry point right behind an unsynchronised ``calc_polarizabilities_to_device``.  The host entries fill
    their device buffers with blocking copies on the null stream, which do not wait for the handle's non-blocking
    streams: none of those buffers may be one the unfinished call still reads.  ``RN_POTGNN_HOST_F32=0`` (float64
    positions through the synchronous host entry) is read once per process: that case runs in a child process."""
    if follow_up != HOST_F32_OFF:
        _behind_unfinished(case, follow_up)
        return
    env = dict(os.environ, RN_POTGNN_HOST_F32="0")
    code = ("from tests.test_async_entries import _behind_unfinished; "
            f"_behind_unfinished({case!r}, 'calc_polarizabilities'); print('child ok')")
    child = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert child.returncode == 0 and "child ok" in child.stdout, child.stdout[-3000:] + child.stderr[-3000:]


# ----------------------------------------------------------------------------- (c) the caller's out tensor
def test_out_is_validated_before_any_library_call():
    """Both device entries write ``S * 9`` float64 values through ``out``'s pointer: a float32, non-contiguous, host,
    other-device or wrongly shaped ``out`` raises ``ValueError`` before any C call and stays untouched; a contiguous
    leading slice of a larger tensor (what ``bench.py`` passes) is accepted and nothing past it is written."""
    g = load_golden("tio2_notebook")
    posA = np.ascontiguousarray(g["pos_batch"], dtype=np.float64)
    s = posA.shape[0]
    dev = torch.device("cuda", 0)

    def sentinel(shape, dtype=torch.float64, device=dev):
        return torch.full(shape, -7.0, dtype=dtype, device=device)

    bad = {"float32": sentinel((s, 3, 3), torch.float32), "transposed": sentinel((s, 3, 3)).transpose(1, 2),
           "host": sentinel((s, 3, 3), device="cpu"), "short": sentinel((s - 1, 3, 3)), "long": sentinel((s + 1, 3, 3))}
    assert not bad["transposed"].is_contiguous()
    if torch.cuda.device_count() >= 2:
        bad["other_device"] = sentinel((s, 3, 3), device=torch.device("cuda", 1))
    fresh = product_model_from_golden(g, device=0)
    positions = torch.tensor(posA, device=dev)
    for kind, out in bad.items():
        with pytest.raises(ValueError, match="out"):
            fresh.calc_polarizabilities_to_device(posA, out=out)
        with pytest.raises(ValueError, match="out"):
            fresh.calc_polarizabilities_device(positions, out=out)
        assert fresh._handle is None, kind
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()), kind
    want = fresh.calc_polarizabilities(posA)
    assert _rel_err(want, g["f32/alpha"]) < REL
    for method in ("to_device", "device"):
        big = sentinel((s + 3, 3, 3))
        if method == "to_device":
            fresh.calc_polarizabilities_to_device(posA, out=big[:s])
        else:
            fresh.calc_polarizabilities_device(positions, out=big[:s])
        torch.cuda.synchronize()
        np.testing.assert_array_equal(big[:s].cpu().numpy(), want, err_msg=method)
        assert bool((big[s:] == -7.0).all()), method
