"""Atom-group increments, partial Raman tensors and partial MD spectra on the GPU.

``rn_potgnn_group_increments_device`` against torch autograd through the float64 oracle (trapezoid rule on the host),
its third-order convergence against float64 polarizability differences, frozen groups, agreement across calls and
chunkings, ordering behind the caller's stream and argument checks; ``rn_potgnn_partial_raman_tensors`` against the
analytic tensors and the finite-difference spectra of masked displacements (the reference's masking); and
``rn_md_raman_partial(_device)`` against the host definition.  Needs a real MI355X: run with ``-m gpu``."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ramannoodle_amd import _lib
from ramannoodle_amd.dynamics import Phonons, Trajectory
from ramannoodle_amd.spectrum import (DevicePartialMDRamanSpectrum, MDRamanSpectrum, PartialMDRamanSpectrum,
                                      PartialPhononRamanSpectrum, PhononRamanSpectrum, group_labels, polarized_weights)
from tests.conftest import load_golden
from tests.helpers import product_model_from_golden
from tests.test_gpu_parity import _random_model

pytestmark = pytest.mark.gpu

_VEC_TO_TENSOR = np.array([[0, 3, 4], [3, 1, 5], [4, 5, 2]])


@pytest.fixture(autouse=True)
def _no_default_device_mode():
    torch.set_default_device(None)
    yield


@functools.lru_cache(maxsize=None)
def _triclinic():
    g = load_golden("triclinic20")
    return g, product_model_from_golden(g).eval()


def _err(got, want):
    return np.abs(np.asarray(got) - want).max() / max(np.abs(want).max(), 1e-300)


def _oracle_increments(oracle, std, pos, labels, groups):
    """Trapezoid increments (S-1,G,3,3) from d alpha / dx by autograd through the float64 oracle."""
    from oracle import potgnn_oracle as O
    o64 = oracle.to(torch.float64)
    x = torch.tensor(pos, dtype=torch.float64, requires_grad=True)
    out = O.forward(o64, x, faithful=False, grad=True)
    jac = np.stack([torch.autograd.grad(out[:, c].sum(), x, retain_graph=True)[0].numpy() for c in range(6)], axis=1)
    jac_alpha = np.asarray(std)[None, :, :, None, None] * jac[:, _VEC_TO_TENSOR]  # (S,3,3,N,3)
    step = pos[1:] - pos[:-1]
    dx = step - np.round(step)
    out = np.zeros((len(pos) - 1, groups, 3, 3))
    for g in range(groups):
        mask = labels == g
        mean = 0.5 * (jac_alpha[:-1][..., mask, :] + jac_alpha[1:][..., mask, :])
        out[:, g] = np.einsum("tabnk,tnk->tab", mean, dx[:, mask])
    return out


def _device(model, pos, groups, float64=True, **kw):
    positions = torch.tensor(pos, dtype=torch.float64, device="cuda:0")
    return model.calc_group_increments_device(positions, groups, float64=float64, **kw).cpu().numpy()


def test_increments_match_oracle_on_the_md_fixture():
    from oracle import potgnn_oracle as O
    g, model = _triclinic()
    oracle = O.model_from_arrays(g)
    oracle.coefficient = model.gauss_coefficient
    pos = g["md/positions"]
    labels, count = group_labels("species", g["atomic_numbers"])
    want = _oracle_increments(oracle, g["std"], pos, labels, count)
    got64 = model.calc_group_increments(pos, "species")
    assert got64.shape == (len(pos) - 1, 3, 3, 3)
    assert _err(got64, want) < 1e-9, _err(got64, want)
    got32 = model.calc_group_increments(pos, "species", float64=False)
    assert _err(got32, want) < 5e-5, _err(got32, want)
    # the increments of all groups add up to those of one group
    whole = model.calc_group_increments(pos, np.zeros(model.num_atoms, dtype=np.int32))
    assert _err(got64.sum(axis=1), whole[:, 0]) < 1e-12


def test_increments_match_oracle_on_a_random_model():
    g = load_golden("tio2_notebook")
    model, oracle = _random_model(g, 5.0, 64, 64, 2, seed=64 * 131 + 64)
    model.eval()
    rng = np.random.default_rng(5)
    pos = g["positions"][None] + rng.normal(scale=3e-3, size=(6,) + g["positions"].shape)
    pos = pos - np.floor(pos)
    labels = rng.integers(0, 4, size=model.num_atoms).astype(np.int32)
    labels[:4] = np.arange(4)
    want = _oracle_increments(oracle, model._stddev_polarizability, pos, labels, 4)
    got64 = model.calc_group_increments(pos, labels)
    assert _err(got64, want) < 1e-9, _err(got64, want)
    got32 = model.calc_group_increments(pos, labels, float64=False)
    assert _err(got32, want) < 5e-5, _err(got32, want)


def test_third_order_convergence():
    from bench import md_frames
    g, model = _triclinic()
    errors = []
    for dt, frames in ((4.0, 33), (2.0, 65)):  # the same 128 fs
        pos = md_frames(np.random.default_rng(11), g["lattice"], g["positions"], frames, dt_fs=dt)
        incr = model.calc_group_increments(pos, "species")
        alpha = model.calc_polarizabilities(pos, dtype=torch.float64)
        errors.append(np.abs(incr.sum(axis=1) - np.diff(alpha, axis=0)).max())
    assert errors[1] > 1e-11, errors  # far above float64 round-off
    assert errors[0] / errors[1] >= 6.0, errors


def test_frozen_group_is_exactly_zero():
    from bench import md_frames
    g, model = _triclinic()
    pos = md_frames(np.random.default_rng(3), g["lattice"], g["positions"], 40)
    labels, count = group_labels("species", g["atomic_numbers"])
    frozen = labels == 2
    pos[:, frozen] = pos[0, frozen]
    incr = model.calc_group_increments(pos, labels)
    assert np.all(incr[:, 2] == 0.0)
    assert np.abs(incr[:, :2]).max() > 0
    on_dev = DevicePartialMDRamanSpectrum(torch.tensor(incr, device="cuda:0"), 1.0)
    for spectrum in (on_dev, PartialMDRamanSpectrum(incr, 1.0)):
        _, partial = spectrum.measure()
        assert np.all(partial[2] == 0.0) and np.all(partial[:, 2] == 0.0)
        assert np.abs(partial[:2, :2]).max() > 0


def test_repeat_and_chunking_agree():
    """The contraction is summed in a fixed order without atomics; the Jacobian rows come from the existing reverse
    pass, whose EdgeBlock backward accumulates cotangents with atomics, so repeats and chunkings agree to round-off."""
    g, model = _triclinic()
    pos = g["md/positions"]
    for float64, tol in ((True, 1e-12), (False, 1e-5)):
        first = _device(model, pos, "species", float64)
        assert _err(_device(model, pos, "species", float64), first) < tol
        # the smallest power-of-two workspace one step fits in: many chunks
        chunked, limit = None, 1 << 16
        while chunked is None:
            try:
                chunked = _device(model, pos, "species", float64, workspace_limit=limit)
            except MemoryError:
                limit <<= 1
                assert limit <= 1 << 32
        assert _err(chunked, first) < tol
        assert _err(_device(model, pos, "species", float64, workspace_limit=3 * limit), first) < tol


def test_device_increments_wait_on_the_callers_stream():
    g, model = _triclinic()
    pos = g["md/positions"]
    want = _device(model, pos, "species")
    host = torch.tensor(pos, dtype=torch.float64).pin_memory()
    positions = torch.zeros(pos.shape, dtype=torch.float64, device="cuda:0")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        torch.cuda._sleep(50_000_000)
        positions.copy_(host, non_blocking=True)
        out = model.calc_group_increments_device(positions, "species")
        spectrum = DevicePartialMDRamanSpectrum(out, 1.0)
        wavenumbers, partial = spectrum.measure()
    stream.synchronize()
    got = out.cpu().numpy()
    assert _err(got, want) < 1e-12
    _, expect = PartialMDRamanSpectrum(got, 1.0).measure(device=0)
    np.testing.assert_array_equal(partial, expect)
    assert len(wavenumbers) == partial.shape[-1]


def _increments(steps, groups, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(steps)[:, None, None, None]
    freq = 1 + np.arange(groups * 9).reshape(1, groups, 3, 3) % 23
    incr = 0.05 * rng.normal(size=(steps, groups, 3, 3)) + np.cos(0.01 * t * freq)
    return incr + np.swapaxes(incr, 2, 3)


def _configurations(k, seed):
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    return rng.normal(size=(k, 3)), rng.normal(size=(k, 3)), Rotation.random(k, random_state=seed).as_matrix()


@pytest.mark.parametrize("steps,groups,k", [(2, 1, 1), (3, 2, 64), (257, 16, 1), (2000, 16, 64), (199_999, 2, 1),
                                            (200_000, 1, 64)])
def test_device_partial_spectra_match_host(steps, groups, k):
    incr = _increments(steps, groups, seed=steps + groups)
    spectrum = PartialMDRamanSpectrum(incr, 1.5)
    w_host, i_host = spectrum.measure()
    w_dev, i_dev = spectrum.measure(device=0)
    np.testing.assert_array_equal(w_dev, w_host)
    if i_host.size:
        assert _err(i_dev, i_host) < 1e-10
    e_i, e_s, rotations = _configurations(k, seed=k)
    _, p_host = spectrum.measure_polarized(e_i, e_s, rotations)
    _, p_dev = spectrum.measure_polarized(e_i, e_s, rotations, device=0)
    assert p_dev.shape == (k, groups, groups, len(w_host))
    if p_host.size:
        assert _err(p_dev, p_host) < 1e-10
    np.testing.assert_array_equal(p_dev, np.swapaxes(p_dev, 1, 2))


def test_single_group_matches_md_spectrum():
    incr = _increments(4001, 1, seed=9)
    alpha = np.concatenate([np.zeros((1, 3, 3)), np.cumsum(incr[:, 0], axis=0)])
    w_md, i_md = MDRamanSpectrum(alpha, 1.0).measure(device=0)
    w, partial = DevicePartialMDRamanSpectrum(torch.tensor(incr, device="cuda:0"), 1.0).measure()
    np.testing.assert_array_equal(w, w_md)
    assert _err(partial[0, 0], i_md) < 1e-10


def test_partial_raman_tensors_and_masking():
    g, model = _triclinic()
    ref, disp, wavenumbers = g["positions"], g["ph/displacements"], g["ph/wavenumbers"]
    partial = model.calc_partial_raman_tensors(ref, disp, "species")
    assert partial.shape == (len(disp), 3, 3, 3)
    analytic = model.calc_raman_tensors(ref, disp, method="analytic")
    assert _err(partial.sum(axis=1), analytic) < 1e-12
    phonons = Phonons(ref, wavenumbers, disp)
    spectrum = phonons.get_partial_raman_spectrum(model, "species")
    assert isinstance(spectrum, PartialPhononRamanSpectrum)
    _, intensities = spectrum.measure()
    labels, _ = group_labels("species", g["atomic_numbers"])
    for grp in range(3):
        masked = disp * (labels == grp)[None, :, None]
        _, want = PhononRamanSpectrum(wavenumbers, model.calc_raman_tensors(ref, masked)).measure()
        assert _err(intensities[grp, grp], want) < 1e-5, (grp, _err(intensities[grp, grp], want))


def test_trajectory_entry_points():
    g, model = _triclinic()
    traj = Trajectory(g["md/positions"], float(g["md/timestep"]))
    on_host = traj.get_partial_raman_spectrum(model, "species")
    on_dev = traj.get_partial_raman_spectrum(model, "species", on_device=True)
    assert isinstance(on_host, PartialMDRamanSpectrum) and isinstance(on_dev, DevicePartialMDRamanSpectrum)
    assert _err(on_dev.increments, on_host.increments) < 1e-12
    _, i_dev = on_dev.measure(laser_correction=True, bose_einstein_correction=True)
    _, i_host = on_host.measure(laser_correction=True, bose_einstein_correction=True)
    assert _err(i_dev, i_host) < 1e-10
    # the sum rule holds to round-off against the cumulative sum of the increments ...
    total = on_host.measure()[1].sum(axis=(0, 1))
    cumulative = np.concatenate([np.zeros((1, 3, 3)), np.cumsum(on_host.increments.sum(axis=1), axis=0)])
    assert _err(total, MDRamanSpectrum(cumulative, traj.timestep).measure()[1]) < 1e-12
    # ... and within the trapezoid error of the model's own series (fractional steps up to 0.01 here: about 1 %)
    alpha = model.calc_polarizabilities(traj.positions_ts, dtype=torch.float64)
    _, whole = MDRamanSpectrum(alpha, traj.timestep).measure()
    assert _err(total, whole) < 5e-2
    with pytest.raises(ValueError):
        traj.get_partial_raman_spectrum(model, np.zeros(5, dtype=np.int32))


def test_out_is_validated():
    g, model = _triclinic()
    positions = torch.tensor(g["md/positions"][:4], device="cuda:0")
    for bad in (torch.empty((3, 3, 3, 3), dtype=torch.float32, device="cuda:0"),
                torch.empty((4, 3, 3, 3), dtype=torch.float64, device="cuda:0"),
                torch.empty((3, 3, 3, 3), dtype=torch.float64),
                torch.empty((3, 3, 3, 6), dtype=torch.float64, device="cuda:0")[..., :3]):
        with pytest.raises(ValueError):
            model.calc_group_increments_device(positions, "species", out=bad)
    out = torch.full((3, 3, 3, 3), np.nan, dtype=torch.float64, device="cuda:0")
    assert model.calc_group_increments_device(positions, "species", out=out) is out
    assert torch.isfinite(out).all()


def test_c_entries_refuse_bad_arguments():
    g, model = _triclinic()
    lib = _lib.load()
    handle = model._ensure_handle()
    n = model.num_atoms
    pos = torch.tensor(g["md/positions"][:4], device="cuda:0")
    out = torch.zeros((3, 3, 9), dtype=torch.float64, device="cuda:0")
    labels, _ = group_labels("species", g["atomic_numbers"])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def incr(s, lab, groups, p=C.c_void_p(pos.data_ptr()), o=C.c_void_p(out.data_ptr())):
        lab = None if lab is None else C.c_void_p(lab.ctypes.data)
        return lib.rn_potgnn_group_increments_device(handle, p, s, lab, groups, 1, 0, o, stream)

    bad = labels.copy()
    bad[0] = 3
    negative = labels.copy()
    negative[0] = -1
    for rc in (incr(1, labels, 3), incr(0, labels, 3), incr(4, labels, 0), incr(4, labels, 17), incr(4, bad, 3),
               incr(4, negative, 3), incr(4, labels, 4), incr(4, None, 3), incr(4, labels, 3, p=None),
               incr(4, labels, 3, o=None)):
        assert rc == _lib.RN_ERR_INVALID_ARGUMENT
    assert lib.rn_potgnn_group_increments_device(None, C.c_void_p(pos.data_ptr()), 4, C.c_void_p(labels.ctypes.data),
                                                 3, 1, 0, C.c_void_p(out.data_ptr()), stream) == \
        _lib.RN_ERR_INVALID_ARGUMENT
    assert incr(4, labels, 3) == _lib.RN_OK

    ref = np.ascontiguousarray(g["positions"])
    disp = np.ascontiguousarray(g["ph/displacements"])
    raman = np.zeros((len(disp), 3, 9))

    def tensors(lab, groups, d=disp, r=raman):
        return lib.rn_potgnn_partial_raman_tensors(handle, C.c_void_p(ref.ctypes.data),
                                                   None if d is None else C.c_void_p(d.ctypes.data), len(disp),
                                                   None if lab is None else C.c_void_p(lab.ctypes.data), groups,
                                                   None if r is None else C.c_void_p(r.ctypes.data))

    for rc in (tensors(labels, 0), tensors(labels, 17), tensors(bad, 3), tensors(None, 3), tensors(labels, 3, d=None),
               tensors(labels, 3, r=None)):
        assert rc == _lib.RN_ERR_INVALID_ARGUMENT
    assert tensors(labels, 3) == _lib.RN_OK

    weights, _ = polarized_weights([1, 0, 0], [0, 1, 0])
    inc = np.zeros((9, 2, 9))
    spec = np.zeros((1, 3, 4))

    def md(steps, groups, i=inc, w=weights, o=spec, bins=4):
        return lib.rn_md_raman_partial(None if i is None else C.c_void_p(i.ctypes.data), steps, groups,
                                       None if w is None else C.c_void_p(w.ctypes.data), 1, 0, 0,
                                       None if o is None else C.c_void_p(o.ctypes.data), bins)

    for rc in (md(1, 2, bins=0), md(9, 0), md(9, 17), md(9, 2, i=None), md(9, 2, w=None), md(9, 2, o=None),
               md(9, 2, bins=5)):
        assert rc == _lib.RN_ERR_INVALID_ARGUMENT
    assert md(9, 2) == _lib.RN_OK
    assert n == 20
