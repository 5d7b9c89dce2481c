"""Variable-cell MD on the GPU: a lattice per frame through the evaluation entries, the cell channel of the atom-group
increments, and the way from an XDATCAR with a header per configuration to spectra.

Expected values come from the reference fixture with strained cells (``triclinic20_r2``: ``lat/*``) and from the float64
oracle, which takes ``lattices=`` with ``grad=True``.  Tolerances are the project's: ``REL`` of ``test_gpu_parity.py``;
1e-9 (float64), 5e-5 (float32), 1e-12 (repeats) and the convergence ratio 6 of ``test_partial_spectra_gpu.py``.
Needs a real MI355X: run with ``-m gpu``."""
import functools
import os

import numpy as np
import pytest
import torch

from ramannoodle_amd import _lib
from ramannoodle_amd.dynamics import Trajectory, TrajectoryEnsemble
from ramannoodle_amd.io.vasp.xdatcar import XdatcarReader, read_trajectory, stream_polarizabilities
from ramannoodle_amd.spectrum import MDRamanSpectrum, group_labels
from tests.conftest import load_golden
from tests.helpers import product_model_from_golden
from tests.test_async_entries import _check_window, _open_window, _sync_eval_ms
from tests.test_gpu_parity import REL, _random_model

pytestmark = pytest.mark.gpu

_VEC_TO_TENSOR = np.array([[0, 3, 4], [3, 1, 5], [4, 5, 2]])
NPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xdatcar_cells", "npt.XDATCAR")

# the strain of the tests below: L_t = L0 (I + eps_t), eps_t[i][j] = AMP[i][j] sin(2 pi t / PER[i][j] + 0.3), t in fs;
# inside the +-3 % the reference fixture was strained by
AMP = np.array([[.010, .004, -.003], [.004, -.008, .005], [-.003, .005, .006]])
PER = np.array([[310., 470., 390.], [470., 260., 530.], [390., 530., 350.]])


@pytest.fixture(autouse=True)
def _no_default_device_mode():
    torch.set_default_device(None)
    yield


@functools.lru_cache(maxsize=None)
def _triclinic():
    g = load_golden("triclinic20")
    return g, load_golden("triclinic20_r2"), product_model_from_golden(g).eval()


def _strained(lattice, frames, dt):
    t = (np.arange(frames) * dt)[:, None, None]
    return lattice[None] @ (np.eye(3)[None] + AMP[None] * np.sin(2 * np.pi * t / PER[None] + 0.3))


@functools.lru_cache(maxsize=None)
def _series(dt, frames):
    """(positions, lattices) of the MD series: bench.md_frames with seed 11 in the strained cells."""
    from bench import md_frames
    g, _, _ = _triclinic()
    pos = md_frames(np.random.default_rng(11), g["lattice"], g["positions"], frames, dt_fs=dt)
    return pos, _strained(g["lattice"], frames, dt)


def _seven():
    """Seven frames with seven different lattices."""
    pos, lat = _series(4.0, 33)
    return np.ascontiguousarray(pos[3:31:4]), np.ascontiguousarray(lat[3:31:4])


def _cuda(array):
    return torch.tensor(np.ascontiguousarray(array), dtype=torch.float64, device="cuda:0")


def _err(got, want):
    return np.abs(np.asarray(got) - want).max() / max(np.abs(want).max(), 1e-300)


# ----------------------------------------------------------------------------- 1. the reference fixture
def test_strained_cells_match_the_reference_fixture():
    g, r, model = _triclinic()
    pos, lat = r["lat/positions"], r["lat/lattices"]
    fixed = model.calc_polarizabilities(pos)
    for dtype, key in ((None, "lat/forward"), (torch.float64, "lat/forward64")):
        want = r[key][:, _VEC_TO_TENSOR] * g["std"] + g["mean"]
        got = model.calc_polarizabilities(pos, dtype=dtype, lattices=lat)
        scale = np.abs(want).max()
        print(f"{key}: miss {np.abs(got - want).max() / scale:.3e} of the largest entry")
        assert got.shape == (len(pos), 3, 3) and got.dtype == np.float64
        assert np.abs(got - want).max() < REL * scale
    got = model.calc_polarizabilities(pos, lattices=lat)
    np.testing.assert_array_equal(lat[0], g["lattice"])  # frame 0 carries the reference lattice
    assert np.abs(got[0] - fixed[0]).max() < REL * scale
    # the others really differ: measured as test_gpu_parity.py measures it for `forward`, on the standardised 6-vectors and
    # their largest entry (the de-standardised tensors are mostly the mean, which no lattice moves)
    moved = np.abs((got[1:] - fixed[1:]) / g["std"]).max()
    print(f"strained frames move the standardised tensor by {moved:.3e}, its largest entry is {np.abs(r['lat/forward']).max():.3e}")
    assert moved > 1e3 * REL * np.abs(r["lat/forward"]).max()


# ----------------------------------------------------------------------------- 2. lattices=None is the old call
def test_no_lattices_is_the_fixed_cell_call_bit_for_bit():
    g, _, model = _triclinic()
    pos = g["pos_batch"]
    d_pos = _cuda(pos)
    for dtype in (None, torch.float64):
        np.testing.assert_array_equal(model.calc_polarizabilities(pos, dtype=dtype, lattices=None),
                                      model.calc_polarizabilities(pos, dtype=dtype))
        np.testing.assert_array_equal(model.calc_polarizabilities_device(d_pos, dtype=dtype, lattices=None, synchronize=True).cpu(),
                                      model.calc_polarizabilities_device(d_pos, dtype=dtype, synchronize=True).cpu())
    np.testing.assert_array_equal(model.calc_polarizabilities(pos, progress=True, lattices=None), model.calc_polarizabilities(pos))
    np.testing.assert_array_equal(model.calc_polarizabilities_to_device(pos, lattices=None).cpu(),
                                  model.calc_polarizabilities_to_device(pos).cpu())
    # the C entries with a null pointer are the fixed-cell entries
    lib, handle = _lib.load(), model._ensure_handle()
    want = model.calc_polarizabilities(pos)
    out = np.empty_like(want)
    assert lib.rn_potgnn_calc_polarizabilities_cells(handle, pos.ctypes.data, None, len(pos), 0, out.ctypes.data) == 0
    np.testing.assert_array_equal(out, want)
    d_out = torch.empty((len(pos), 3, 3), dtype=torch.float64, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.rn_potgnn_calc_polarizabilities_cells_to_device(handle, pos.ctypes.data, None, len(pos), d_out.data_ptr(), stream) == 0
    np.testing.assert_array_equal(d_out.cpu().numpy(), want)
    d_out.zero_()
    assert lib.rn_potgnn_forward_cells_device(handle, d_pos.data_ptr(), None, len(pos), 0, d_out.data_ptr(), stream, 1) == 0
    np.testing.assert_array_equal(d_out.cpu().numpy(), want)
    # the increments: the same shape and, as repeats of that entry agree (its reverse pass accumulates with atomics), 1e-12
    md = g["md/positions"][:9]
    first = model.calc_group_increments(md, "species")
    again = model.calc_group_increments(md, "species", lattices=None)
    assert again.shape == first.shape == (8, 3, 3, 3)
    assert _err(again, first) < 1e-12
    labels, count = group_labels("species", g["atomic_numbers"])
    d_md, d_incr = _cuda(md), torch.empty((8, count, 3, 3), dtype=torch.float64, device="cuda:0")
    assert lib.rn_potgnn_group_increments_cells_device(handle, d_md.data_ptr(), None, 9, labels.ctypes.data, count, 1, 0,
                                                       d_incr.data_ptr(), stream) == 0
    assert _err(d_incr.cpu().numpy(), first) < 1e-12


# ----------------------------------------------------------------------------- 3. pieces and chunks
def test_pieces_and_chunks_keep_every_frames_own_lattice(monkeypatch):
    """A lattice pointer that does not advance with the positions gives frame k the lattice of frame 0 of its piece."""
    g, _, model = _triclinic()
    pos, lat = _seven()
    assert len({tuple(l.ravel()) for l in lat}) == 7
    single = {dtype: np.concatenate([model.calc_polarizabilities(pos[k:k + 1], dtype=dtype, lattices=lat[k:k + 1])
                                     for k in range(7)]) for dtype in (None, torch.float64)}
    assert np.abs(single[None] - model.calc_polarizabilities(pos)).max() > 10 * REL * np.abs(single[None]).max()  # the cells matter
    np.testing.assert_array_equal(model.calc_polarizabilities(pos, lattices=lat), single[None])
    monkeypatch.setenv("RN_POTGNN_HOST_PIECE", "2")  # four pieces: 2 + 2 + 2 + 1
    np.testing.assert_array_equal(model.calc_polarizabilities(pos, lattices=lat), single[None])
    np.testing.assert_array_equal(model.calc_polarizabilities_to_device(pos, lattices=lat).cpu().numpy(), single[None])
    monkeypatch.delenv("RN_POTGNN_HOST_PIECE")
    chunked = product_model_from_golden(g, max_chunk_structures=3).eval()  # chunks of 3 + 3 + 1 on the lanes
    d_pos, d_lat = _cuda(pos), _cuda(lat)
    for dtype in (None, torch.float64):
        np.testing.assert_array_equal(chunked.calc_polarizabilities(pos, dtype=dtype, lattices=lat), single[dtype])
        np.testing.assert_array_equal(
            chunked.calc_polarizabilities_device(d_pos, dtype=dtype, lattices=d_lat, synchronize=True).cpu().numpy(), single[dtype])
    np.testing.assert_array_equal(chunked.calc_polarizabilities_to_device(pos, lattices=lat).cpu().numpy(), single[None])
    np.testing.assert_array_equal(chunked.calc_polarizabilities(pos, lattices=lat, progress=True), single[None])


# ----------------------------------------------------------------------------- 4. the three forms
def test_host_to_device_and_device_forms_agree_bit_for_bit():
    _, _, model = _triclinic()
    pos, lat = _series(4.0, 33)
    posB, latB = np.ascontiguousarray(pos[::-1]), np.ascontiguousarray(lat[::-1])
    wantA, wantB = model.calc_polarizabilities(pos, lattices=lat), model.calc_polarizabilities(posB, lattices=latB)
    assert np.abs(wantA - wantB[::-1]).max() == 0 and np.abs(wantA - wantB).max() > 0
    out = model.calc_polarizabilities_to_device(pos, lattices=lat)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), wantA)
    on_device = model.calc_polarizabilities_device(_cuda(pos), lattices=_cuda(lat), synchronize=True)
    np.testing.assert_array_equal(on_device.cpu().numpy(), wantA)
    # queued behind a long reader of `out` on torch's stream: the reader sees the old values, `out` ends with the new
    torch.cuda.synchronize()
    eval_ms = _sync_eval_ms(model, pos)
    stream = torch.cuda.Stream()
    start, end = _open_window(stream)
    with torch.cuda.stream(stream):
        snap = out.clone()
        again = model.calc_polarizabilities_to_device(posB, out=out, lattices=latB)
        behind = model.calc_polarizabilities_device(_cuda(posB), lattices=_cuda(latB))  # and the device form behind that
    torch.cuda.synchronize()
    slept = _check_window(start, end, eval_ms)
    assert again is out
    np.testing.assert_array_equal(snap.cpu().numpy(), wantA, err_msg=f"a reader queued before the call saw its result (sleep {slept:.0f} ms)")
    np.testing.assert_array_equal(out.cpu().numpy(), wantB)
    np.testing.assert_array_equal(behind.cpu().numpy(), wantB)


# ----------------------------------------------------------------------------- 5. increments against autograd
@functools.lru_cache(maxsize=None)
def _oracle_increments():
    """Trapezoid increments (S-1,G+1,3,3) of the 33-frame series from d alpha / dx at each frame's own lattice and
    d alpha / dL, by autograd through the float64 oracle; the last channel is the cell."""
    from oracle import potgnn_oracle as O
    g, _, model = _triclinic()
    oracle = O.model_from_arrays(g)
    oracle.coefficient = model.gauss_coefficient
    pos, lat = _series(4.0, 33)
    labels, groups = group_labels("species", g["atomic_numbers"])
    x = torch.tensor(pos, dtype=torch.float64, requires_grad=True)
    cells = torch.tensor(lat, dtype=torch.float64, requires_grad=True)
    out = O.forward(oracle.to(torch.float64), x, faithful=False, grad=True, lattices=cells)
    grads = [torch.autograd.grad(out[:, c].sum(), (x, cells), retain_graph=True) for c in range(6)]
    std = np.asarray(g["std"])[None, :, :, None, None]
    jac_x = std * np.stack([gx.numpy() for gx, _ in grads], axis=1)[:, _VEC_TO_TENSOR]  # (S,3,3,N,3)
    jac_l = std * np.stack([gl.numpy() for _, gl in grads], axis=1)[:, _VEC_TO_TENSOR]  # (S,3,3,3,3)
    step = pos[1:] - pos[:-1]
    dx = step - np.round(step)
    want = np.zeros((len(pos) - 1, groups + 1, 3, 3))
    for k in range(groups):
        mask = labels == k
        want[:, k] = np.einsum("tabnk,tnk->tab", 0.5 * (jac_x[:-1][..., mask, :] + jac_x[1:][..., mask, :]), dx[:, mask])
    want[:, groups] = np.einsum("tabij,tij->tab", 0.5 * (jac_l[:-1] + jac_l[1:]), np.diff(lat, axis=0))
    return want


@pytest.mark.parametrize("float64,tol", [(True, 1e-9), (False, 5e-5)])
def test_increments_with_cell_channel_match_autograd(float64, tol):
    _, _, model = _triclinic()
    pos, lat = _series(4.0, 33)
    want = _oracle_increments()
    got = model.calc_group_increments(pos, "species", float64=float64, lattices=lat)
    assert got.shape == want.shape == (32, 4, 3, 3)
    for channel in range(4):
        print(f"float64={float64} channel {channel}: miss {_err(got[:, channel], want[:, channel]):.3e}, "
              f"size {np.abs(want[:, channel]).max():.3e}")
    assert np.abs(want[:, 3]).max() > 0.02 * np.abs(want[:, :3]).max()  # the cell's share is no rounding matter
    for channel in range(4):
        assert _err(got[:, channel], want[:, channel]) < tol, channel
    assert _err(got, want) < tol


# ----------------------------------------------------------------------------- 6. third-order convergence
def test_all_channels_add_up_to_the_polarizability_steps_at_third_order():
    """Without the cell channel the coarse miss is about 4e-4 and does not shrink with the step: the ratio test can
    pass only with a correct channel (float64 oracle alone: misses 1.33e-5 and 2.02e-6, ratio 6.58)."""
    _, _, model = _triclinic()
    errors, atoms_only = [], []
    for dt, frames in ((4.0, 33), (2.0, 65)):  # the same 128 fs
        pos, lat = _series(dt, frames)
        incr = model.calc_group_increments(pos, "species", lattices=lat)
        alpha = model.calc_polarizabilities(pos, dtype=torch.float64, lattices=lat)
        errors.append(np.abs(incr.sum(axis=1) - np.diff(alpha, axis=0)).max())
        atoms_only.append(np.abs(incr[:, :-1].sum(axis=1) - np.diff(alpha, axis=0)).max())
    print(f"misses {errors[0]:.3e} (4 fs) {errors[1]:.3e} (2 fs), ratio {errors[0] / errors[1]:.2f}; atoms alone {atoms_only}")
    assert errors[1] > 1e-11, errors  # far above float64 round-off
    assert errors[0] / errors[1] >= 6.0, errors


# ----------------------------------------------------------------------------- 7. exact zeros, the fixed-cell entry, chunking
def test_exact_zeros_and_agreement_with_the_fixed_cell_entry():
    g, _, model = _triclinic()
    pos, lat = _series(4.0, 33)
    constant = np.broadcast_to(g["lattice"], lat.shape).copy()
    incr = model.calc_group_increments(pos, "species", lattices=constant)
    assert np.all(incr[:, 3] == 0.0)
    assert _err(incr[:, :3], model.calc_group_increments(pos, "species")) < 1e-12
    still = np.broadcast_to(pos[0], pos.shape).copy()
    incr = model.calc_group_increments(still, "species", lattices=lat)
    assert np.all(incr[:, :3] == 0.0)
    assert np.all(np.abs(incr[:, 3]).max(axis=(1, 2)) > 0)
    # the smallest power-of-two workspace one step fits in: many chunks, the lattice rows carried over their boundaries
    d_pos, d_lat = _cuda(pos), _cuda(lat)
    first = model.calc_group_increments_device(d_pos, "species", lattices=d_lat).cpu().numpy()
    chunked, limit = None, 1 << 16
    while chunked is None:
        try:
            chunked = model.calc_group_increments_device(d_pos, "species", lattices=d_lat, workspace_limit=limit).cpu().numpy()
        except MemoryError:
            limit <<= 1
            assert limit <= 1 << 32
    assert _err(chunked, first) < 1e-12
    assert _err(chunked[:, 3], first[:, 3]) < 1e-12
    three = model.calc_group_increments_device(d_pos, "species", lattices=d_lat, workspace_limit=3 * limit).cpu().numpy()
    assert _err(three, first) < 1e-12
    out = torch.empty((32, 4, 3, 3), dtype=torch.float64, device="cuda:0")
    assert model.calc_group_increments_device(d_pos, "species", lattices=d_lat, out=out) is out
    assert _err(out.cpu().numpy(), first) < 1e-12


# ----------------------------------------------------------------------------- 8. from the file to the spectra
@functools.lru_cache(maxsize=None)
def _npt_model():
    with XdatcarReader(NPT) as reader:
        positions, lattices = reader.read(), reader.read_lattices()
    fixture = {"lattice": lattices[0], "positions": positions[0] % 1.0, "atomic_numbers": np.array([22, 8, 8])}
    model, _ = _random_model(fixture, 4.85, 16, 16, 2, seed=5)  # (Ti-O at 2.9 and 4.6 A inside, O-O at 5.1 A outside)
    return model.eval()


def test_from_an_npt_file_to_the_spectra():
    model = _npt_model()
    assert model.num_edges == 4
    trajectory = read_trajectory(NPT, 2.0)
    pos, lat = trajectory.positions_ts, trajectory.lattice_ts
    assert lat.shape == (5, 3, 3)
    alpha = model.calc_polarizabilities(pos, lattices=lat)
    assert np.abs(alpha - model.calc_polarizabilities(pos)).max() > 10 * REL * np.abs(alpha).max()  # the cells matter
    wavenumbers, intensities = trajectory.get_raman_spectrum(model).measure()
    want_w, want_i = MDRamanSpectrum(alpha, 2.0).measure()
    np.testing.assert_array_equal(wavenumbers, want_w)
    np.testing.assert_array_equal(intensities, want_i)
    _, on_device = trajectory.get_raman_spectrum(model, on_device=True).measure()
    assert _err(on_device, want_i) < 1e-10
    np.testing.assert_array_equal(stream_polarizabilities(model, NPT, chunk_frames=2), alpha)
    # the partial spectra: the cell is one more group, and the spectrum classes take it as it comes
    device = trajectory.get_partial_raman_spectrum(model, "species", on_device=True)
    host = trajectory.get_partial_raman_spectrum(model, "species")
    w_dev, p_dev = device.measure()
    w_host, p_host = host.measure()
    assert p_dev.shape == (3, 3, len(want_w)) and p_host.shape == p_dev.shape
    np.testing.assert_array_equal(w_dev, w_host)
    assert _err(p_dev, p_host) < 1e-10
    assert np.abs(p_host[2, 2]).max() > 0  # the cell's own spectrum
    # an ensemble joins the lattices as it joins the frames
    ensemble = TrajectoryEnsemble([trajectory, Trajectory(pos[::-1], 2.0, lat[::-1])])
    np.testing.assert_array_equal(model.calc_polarizabilities(ensemble._positions_ts, lattices=ensemble._lattice_ts)[5:], alpha[::-1])
    _, e_host = ensemble.get_partial_raman_spectrum(model, "species").measure()
    _, e_dev = ensemble.get_partial_raman_spectrum(model, "species", on_device=True).measure()
    assert e_host.shape == p_host.shape and _err(e_dev, e_host) < 1e-10
    _, e_all = ensemble.get_raman_spectrum(model).measure()
    _, e_all_dev = ensemble.get_raman_spectrum(model, on_device=True).measure()
    assert _err(e_all_dev, e_all) < 1e-10


# ----------------------------------------------------------------------------- 9. bad arguments
def test_bad_lattices_are_refused_before_any_device_work():
    g, _, model = _triclinic()
    pos, lat = _seven()
    d_pos, d_lat = _cuda(pos), _cuda(lat)
    want = model.calc_polarizabilities(pos, lattices=lat)
    nan, singular = lat.copy(), lat.copy()
    nan[4, 1, 2] = np.nan
    singular[5, 2] = 0.0  # (a determinant of exactly zero)
    dependent = lat.copy()
    dependent[5, 2] = dependent[5, 0] - 2 * dependent[5, 1]  # (and one of zero up to rounding)
    sixteen = (np.arange(model.num_atoms) % 16).astype(np.int32)
    for call in (lambda L: model.calc_polarizabilities(pos, lattices=L),
                 lambda L: model.calc_polarizabilities(pos, lattices=L, dtype=torch.float64),
                 lambda L: model.calc_polarizabilities(pos, lattices=L, progress=True),
                 lambda L: model.calc_polarizabilities_to_device(pos, lattices=L),
                 lambda L: model.calc_group_increments(pos, "species", lattices=L)):
        with pytest.raises(ValueError, match="wrong shape"):
            call(lat[:6])
        with pytest.raises(ValueError, match="wrong shape"):
            call(lat.reshape(7, 9))
        with pytest.raises(ValueError, match=r"(frame 4|\[4\]) has a non-finite entry"):
            call(nan)
        with pytest.raises(ValueError, match=r"(frame 5|\[5\]) is singular"):
            call(singular)
        with pytest.raises(ValueError, match=r"(frame 5|\[5\]) is singular"):
            call(dependent)
    for call in (lambda L: model.calc_polarizabilities_device(d_pos, lattices=L),
                 lambda L: model.calc_group_increments_device(d_pos, "species", lattices=L)):
        with pytest.raises(ValueError, match="wrong shape"):
            call(d_lat[:6])
        with pytest.raises(ValueError, match="contiguous float64 device tensor"):
            call(lat)
        with pytest.raises(ValueError, match="contiguous float64 device tensor"):
            call(d_lat.float())
    with pytest.raises(ValueError, match="at most 15 atom groups"):
        model.calc_group_increments_device(d_pos, sixteen, lattices=d_lat)
    assert model.calc_group_increments_device(d_pos, sixteen).shape == (6, 16, 3, 3)  # without lattices 16 groups are fine
    fifteen = (np.arange(model.num_atoms) % 15).astype(np.int32)
    assert model.calc_group_increments_device(d_pos, fifteen, lattices=d_lat).shape == (6, 16, 3, 3)
    with pytest.raises(ValueError, match="lattice_ts"):
        Trajectory(pos, 1.0, nan)
    # the C entries
    lib, handle = _lib.load(), model._ensure_handle()
    out = np.full((7, 3, 3), 7.0)
    d_out = torch.full((7, 3, 3), 7.0, dtype=torch.float64, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    for bad, text in ((nan, b"lattice of frame 4 has a non-finite entry"), (singular, b"lattice of frame 5 is singular")):
        for use_float64 in (0, 1):
            assert lib.rn_potgnn_calc_polarizabilities_cells(handle, pos.ctypes.data, bad.ctypes.data, 7, use_float64,
                                                             out.ctypes.data) == _lib.RN_ERR_INVALID_ARGUMENT
            assert text in lib.rn_potgnn_last_error(handle)
        assert lib.rn_potgnn_calc_polarizabilities_cells_to_device(handle, pos.ctypes.data, bad.ctypes.data, 7, d_out.data_ptr(),
                                                                   stream) == _lib.RN_ERR_INVALID_ARGUMENT
        assert text in lib.rn_potgnn_last_error(handle)
    d_incr = torch.full((6, 17, 3, 3), 7.0, dtype=torch.float64, device="cuda:0")
    assert lib.rn_potgnn_group_increments_cells_device(handle, d_pos.data_ptr(), d_lat.data_ptr(), 7, sixteen.ctypes.data, 16, 1, 0,
                                                       d_incr.data_ptr(), stream) == _lib.RN_ERR_INVALID_ARGUMENT
    assert b"G outside 1..15" in lib.rn_potgnn_last_error(handle)
    assert lib.rn_potgnn_group_increments_cells_device(handle, d_pos.data_ptr(), d_lat.data_ptr(), 1, sixteen.ctypes.data, 2, 1, 0,
                                                       d_incr.data_ptr(), stream) == _lib.RN_ERR_INVALID_ARGUMENT
    assert lib.rn_potgnn_forward_cells_device(handle, None, d_lat.data_ptr(), 7, 0, d_out.data_ptr(), stream, 1) == _lib.RN_ERR_INVALID_ARGUMENT
    # nothing was written, nothing is pending, and the next call is right
    torch.cuda.synchronize()
    assert np.all(out == 7.0) and bool((d_out == 7.0).all()) and bool((d_incr == 7.0).all())
    np.testing.assert_array_equal(model.calc_polarizabilities(pos, lattices=lat), want)
