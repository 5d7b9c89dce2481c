"""The interpolation model on the GPU (``csrc/kernels_interp.hip``, ``include/rn_interp.h``).

Parity with what the reference recorded (``tests/golden/make_golden_interp.py``) at 1e-10 of the case's largest
``|alpha|``, the tolerance ``test_mode_vdos_gpu.py`` uses for the same float64 matrix instruction; the device against
``evaluate_host`` at the edges of the kernel's tiles (16 frames x 64 DOFs x 32 columns of 3N); bit-identical repeats;
the Jacobian; closure of the group and mode increments; chunking; the spectra of ``dynamics.py`` end to end; and the
argument checks of the C entries.

Tolerances left to this file: a linear model's analytic and finite-difference Raman tensors differ by the rounding of
two polarizabilities (2^-52 |alpha| each, a few of them summed) divided by delta = 1e-3, that is a few 1e-12 of
|alpha| ~ 30 against tensors of order 0.1 to 1: 1e-9 of the largest tensor.  The spectra use the tolerances of
``test_gpu_parity.py`` (1e-5 of the scale, rtol 5e-5 for the phonon intensities) and the sum rules those of
``test_partial_spectra_gpu.py`` / ``test_mode_raman_gpu.py`` (1e-10 per row).  Needs a real MI355X: run with ``-m gpu``."""
import ctypes as C

import numpy as np
import pytest
import torch

from ramannoodle_amd import _lib
from ramannoodle_amd.dynamics import Phonons, Trajectory, TrajectoryEnsemble
from ramannoodle_amd.spectrum import mode_projectors
from tests.interp_cases import FIXTURES, fixture, mask_of, seeded_case, seeded_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_default_device_mode():
    torch.set_default_device(None)
    yield


def _cuda(array):
    return torch.tensor(np.ascontiguousarray(array), dtype=torch.float64, device="cuda:0")


def _err(got, want):
    return np.abs(np.asarray(got) - want).max() / np.abs(want).max()


# ----------------------------------------------------------------------------- parity with the reference
@pytest.mark.parametrize("name", FIXTURES)
def test_parity_with_the_reference(name):
    case, g = fixture(name)
    model = case.model()
    positions, want, want_masked = g["positions"], g["alpha"], g["alpha_masked"]
    host = model.calc_polarizabilities(positions)
    device = model.calc_polarizabilities_device(_cuda(positions)).cpu().numpy()
    masked_model = model.get_masked_model(list(g["masked"]))
    masked = masked_model.calc_polarizabilities(positions)
    masked_device = masked_model.calc_polarizabilities_device(_cuda(positions)).cpu().numpy()
    errors = [_err(host, want), _err(device, want), _err(masked, want_masked), _err(masked_device, want_masked)]
    print(f"{name}: host entry {errors[0]:.2e}, device entry {errors[1]:.2e}, masked {errors[2]:.2e} / {errors[3]:.2e}")
    assert host.shape == want.shape == (len(positions), 3, 3)
    assert max(errors) <= 1e-10
    np.testing.assert_array_equal(host, device)
    # the mask set in place, and cleared again
    model.mask = mask_of(g)
    assert _err(model.calc_polarizabilities(positions), want_masked) <= 1e-10
    model.unmask()
    np.testing.assert_array_equal(model.calc_polarizabilities(positions), host)


# ----------------------------------------------------------------------------- tile edges, model variants
@pytest.mark.parametrize("frames,atoms,dofs", [(1, 1, 1), (16, 32, 64), (17, 5, 15), (33, 67, 130)])
def test_tile_edges_against_the_host_definition(frames, atoms, dofs):
    case = seeded_case(100 * frames + dofs, atoms, dofs)
    positions = seeded_frames(case, frames, frames)
    want = case.host(positions)
    got = case.model().calc_polarizabilities_device(_cuda(positions)).cpu().numpy()
    print(f"({frames},{atoms},{dofs}): {_err(got, want):.2e}")
    assert _err(got, want) <= 1e-10


@pytest.mark.parametrize("frames", [8192 + 5, 16384 + 3])
def test_wider_workgroups_of_long_calls(frames):
    """From 8192 (16384) frames on a workgroup takes two (four) tiles of 16 frames (``launch_alpha``): the same bits as
    the one-tile kernel, on a model small enough that the host reference takes a fraction of a second."""
    case = seeded_case(51, 5, 15)
    positions = seeded_frames(case, frames, frames, sigma=0.02)
    model = case.model()
    d_positions = _cuda(positions)
    got = model.calc_polarizabilities_device(d_positions).cpu().numpy()
    assert _err(got, case.host(positions)) <= 1e-10
    for first in (0, 4096, frames - 21):  # (the last rows: a workgroup with a remainder of frames)
        narrow = model.calc_polarizabilities_device(d_positions[first:first + 21].contiguous()).cpu().numpy()
        np.testing.assert_array_equal(narrow, got[first:first + 21])
    if frames > 16384:
        _, want = case.host(positions[-40:], jacobian=True)
        rows = model.calc_jacobian_device(d_positions)[-40:].cpu().numpy()
        assert _err(rows, want) <= 1e-10


@pytest.mark.parametrize("variant", ["one_piece", "orders_5_and_1", "asymmetric"])
def test_model_variants(variant):
    if variant == "one_piece":
        case = seeded_case(31, 6, 18, orders=(3,), points=4)
        assert np.all(np.diff(case.tables.piece_offsets) == 1)
    elif variant == "orders_5_and_1":
        case = seeded_case(32, 6, 17, orders=(5, 1))
        assert set(case.tables.orders) == {1, 5}
    else:
        case = seeded_case(33, 6, 10, symmetric=False)
    positions = seeded_frames(case, 34, 21, sigma=0.03)  # (some amplitudes beyond the knots)
    want = case.host(positions)
    got = case.model().calc_polarizabilities(positions)
    assert _err(got, want) <= 1e-10
    if variant == "asymmetric":
        assert np.abs(got - got.transpose(0, 2, 1)).max() > 1e-6


def test_repeats_and_frame_counts_are_bit_identical():
    case, g = fixture("interp_p1_tiles")
    model = case.model()
    positions = _cuda(g["positions"])
    first = model.calc_polarizabilities_device(positions).cpu().numpy()
    np.testing.assert_array_equal(model.calc_polarizabilities_device(positions).cpu().numpy(), first)
    head = model.calc_polarizabilities_device(positions[:16].contiguous()).cpu().numpy()
    np.testing.assert_array_equal(head, first[:16])
    out = torch.full((35, 3, 3), np.nan, dtype=torch.float64, device="cuda:0")
    assert model.calc_polarizabilities_device(positions, out=out) is out
    np.testing.assert_array_equal(out.cpu().numpy(), first)
    with pytest.raises(ValueError):
        model.calc_polarizabilities_device(positions, out=out[:34])
    with pytest.raises(ValueError):
        model.calc_polarizabilities_device(positions, lattices=positions)


# ----------------------------------------------------------------------------- Jacobian
@pytest.mark.parametrize("name", FIXTURES)
def test_jacobian_against_the_host(name):
    case, g = fixture(name)
    assert case.breakpoint_gap(g["positions"], orders=(1,)) > 1e-9  # (a precondition on the inputs: a kink is a jump of s')
    _, want = case.host(g["positions"], jacobian=True)
    model = case.model()
    got = model.calc_jacobian_device(_cuda(g["positions"])).cpu().numpy()
    print(f"{name}: Jacobian {_err(got, want):.2e}")
    assert got.shape == want.shape and _err(got, want) <= 1e-10
    np.testing.assert_array_equal(model.calc_jacobian_device(_cuda(g["positions"])).cpu().numpy(), got)
    masked = model.get_masked_model(list(g["masked"]))
    _, want = case.host(g["positions"], mask=mask_of(g), jacobian=True)
    assert _err(masked.calc_jacobian_device(_cuda(g["positions"])).cpu().numpy(), want) <= 1e-10


# ----------------------------------------------------------------------------- closure
def _modes_of(case, seed, count):
    rng = np.random.default_rng(seed)
    atoms = len(case.ref_positions)
    return mode_projectors(rng.normal(size=(count, atoms, 3)) * 0.05, case.lattice, np.ones(atoms))


def test_closure_of_a_linear_model():
    case = seeded_case(41, atoms=9, dofs=20, linear=True)
    assert np.all(np.diff(case.tables.piece_offsets) == 1) and np.all(case.tables.orders == 1)
    model = case.model()
    positions = seeded_frames(case, 42, 19)
    alpha = case.host(positions)
    scale = np.abs(alpha).max()
    labels = np.arange(9) % 3
    groups = model.calc_group_increments(positions, labels)
    assert groups.shape == (18, 3, 3, 3)
    assert np.abs(groups.sum(axis=1) - np.diff(alpha, axis=0)).max() <= 1e-10 * scale
    disp, proj = _modes_of(case, 43, 5)
    modes = model.calc_mode_increments(positions, disp, proj, rest=True)
    assert modes.shape == (18, 6, 3, 3)
    assert np.abs(modes.sum(axis=1) - np.diff(alpha, axis=0)).max() <= 1e-10 * scale
    assert np.abs(modes[:, -1]).max() > 1e-6 * scale  # (five modes of 27 leave a rest)
    without = model.calc_mode_increments(positions, disp, proj, rest=False)
    np.testing.assert_array_equal(without, modes[:, :5])
    displacements = np.random.default_rng(44).normal(size=(4, 9, 3)) * 0.05
    analytic = model.calc_raman_tensors(case.ref_positions, displacements, method="analytic")
    finite = model.calc_raman_tensors(case.ref_positions, displacements)
    print(f"linear model: analytic vs finite differences {_err(analytic, finite):.2e}")
    assert _err(analytic, finite) <= 1e-9
    partial = model.calc_partial_raman_tensors(case.ref_positions, displacements, labels)
    assert partial.shape == (4, 3, 3, 3) and _err(partial.sum(axis=1), analytic) <= 1e-12


def test_closure_of_the_cubic_fixture_is_third_order():
    case, g = fixture("interp_p1_small")
    model = case.model()
    base = g["positions"][0]
    pieces = lambda x: case.pieces(x[None])[0].tolist()  # noqa: E731
    for seed in range(200):  # a direction along which the full step crosses no breakpoint (host only: an input choice)
        direction = np.random.default_rng(seed).normal(size=base.shape) * 0.0015
        if pieces(base) == pieces(base + direction) and np.all(np.abs(base + direction - 0.5) < 0.5):
            break
    else:
        raise AssertionError("no direction without a breakpoint crossing")
    errors = []
    for step in (1.0, 0.5):
        frames = np.stack([base, base + step * direction])
        alpha = case.host(frames)
        incr = model.calc_group_increments(frames, "species")
        errors.append(np.abs(incr.sum(axis=1)[0] - (alpha[1] - alpha[0])).max())
    print(f"cubic fixture: closure error {errors[0]:.3e} at h, {errors[1]:.3e} at h/2, ratio {errors[0] / errors[1]:.2f}")
    assert errors[1] > 1e-11 * np.abs(alpha).max()  # (above round-off, or the ratio says nothing)
    assert errors[0] / errors[1] >= 6.0


def test_chunking_does_not_change_the_increments():
    case, g = fixture("interp_p1_small")
    model = case.model()
    positions = _cuda(g["positions"])
    rows, derivatives = 6 * 21 * 8, 6 * 19 * 8
    limit = rows + 10 * (rows + derivatives)  # ten steps per chunk: four chunks for 39 steps
    whole = model.calc_group_increments_device(positions, "species").cpu().numpy()
    chunked = model.calc_group_increments_device(positions, "species", workspace_limit=limit).cpu().numpy()
    np.testing.assert_array_equal(chunked, whole)
    disp, proj = _modes_of(case, 45, 4)
    whole = model.calc_mode_increments_device(positions, disp, proj).cpu().numpy()
    chunked = model.calc_mode_increments_device(positions, disp, proj,
                                                workspace_limit=limit + 2 * disp.nbytes).cpu().numpy()
    np.testing.assert_array_equal(chunked, whole)
    with pytest.raises(MemoryError):
        model.calc_group_increments_device(positions, "species", workspace_limit=rows)


# ----------------------------------------------------------------------------- end to end
def test_spectra_end_to_end_against_the_reference():
    case, g = fixture("interp_p1_small")
    model = case.model()
    trajectory = Trajectory(g["positions"], float(g["md/timestep"]))
    wavenumbers, intensities = trajectory.get_raman_spectrum(model, on_device=True).measure()
    np.testing.assert_allclose(wavenumbers, g["md/wavenumbers"], rtol=1e-12)
    scale = np.abs(g["md/int_raw"]).max()
    print(f"MD spectrum vs the reference: {np.abs(intensities - g['md/int_raw']).max() / scale:.2e}")
    assert np.abs(intensities - g["md/int_raw"]).max() <= 1e-5 * scale
    _, on_host = trajectory.get_raman_spectrum(model).measure()
    assert np.abs(on_host - g["md/int_raw"]).max() <= 1e-5 * scale
    phonons = Phonons(g["ref_positions"], g["ph/wavenumbers"], g["ph/displacements"])
    spectrum = phonons.get_raman_spectrum(model)
    assert _err(spectrum.raman_tensors, g["ph/raman_tensors"]) < 1e-5
    np.testing.assert_allclose(spectrum.measure()[1], g["ph/int_raw"], rtol=5e-5, atol=1e-5 * g["ph/int_raw"].max())
    corrected = spectrum.measure(laser_correction=True, laser_wavelength=532, bose_einstein_correction=True,
                                 temperature=300)[1]
    np.testing.assert_allclose(corrected, g["ph/int_corr"], rtol=5e-5, atol=1e-5 * g["ph/int_corr"].max())


def test_decomposed_spectra_sum_to_the_whole():
    case, g = fixture("interp_p1_small")
    model = case.model()
    timestep = float(g["md/timestep"])
    trajectory = Trajectory(g["positions"], timestep)
    phonons = Phonons(g["ref_positions"], g["ph/wavenumbers"], g["ph/displacements"])
    one = trajectory.get_partial_raman_spectrum(model, np.zeros(7, dtype=np.int32), on_device=True).measure()[1][0, 0]
    # atom groups: the pair spectra sum to the one-group spectrum
    partial = trajectory.get_partial_raman_spectrum(model, "species", on_device=True)
    wavenumbers, pairs = partial.measure()
    groups = len(set(g["atomic_numbers"].tolist()))
    assert pairs.shape == (groups, groups, len(wavenumbers))
    assert np.abs(pairs.sum(axis=(0, 1)) - one).max() <= 1e-10 * np.abs(one).max()
    on_host = trajectory.get_partial_raman_spectrum(model, "species")
    assert _err(on_host.increments, partial.increments) < 1e-12
    # phonon modes and the rest: the last row is the sum of the channels
    modes = trajectory.get_mode_raman_spectrum(model, phonons, on_device=True)
    assert modes.num_channels == len(g["ph/wavenumbers"]) + 1
    _, rows = modes.measure()
    assert np.abs(rows[-1] - one).max() <= 1e-10 * np.abs(one).max()
    bands = np.array([[0.0, 2 * wavenumbers[-1]]])
    _, matrix = modes.measure_interference(bands)
    assert matrix.shape == (1, modes.num_channels, modes.num_channels)
    assert abs(matrix.sum() - rows[-1].sum()) <= 1e-10 * np.abs(matrix).max()
    # phonons by atom group: the partial tensors sum to the analytic ones
    by_group = phonons.get_partial_raman_spectrum(model, "species")
    analytic = model.calc_raman_tensors(g["ref_positions"], g["ph/displacements"], method="analytic")
    assert _err(by_group.partial_raman_tensors.sum(axis=1), analytic) <= 1e-12
    # an ensemble of the two halves: one batched evaluation, the runs never joined
    cut = 22
    ensemble = TrajectoryEnsemble([Trajectory(g["positions"][:cut], timestep), Trajectory(g["positions"][cut:], timestep)])
    on_dev, on_cpu = ensemble.get_raman_spectrum(model, on_device=True), ensemble.get_raman_spectrum(model)
    _, dev_rows = on_dev.measure_segments(12, 3)
    _, cpu_rows = on_cpu.measure_segments(12, 3)
    assert _err(dev_rows, cpu_rows) <= 1e-10
    assert ensemble.get_partial_raman_spectrum(model, "species", on_device=True).run_lengths == [cut, 40 - cut]
    assert ensemble.get_mode_raman_spectrum(model, phonons, on_device=True).run_lengths == [cut, 40 - cut]


# ----------------------------------------------------------------------------- the C entries
def test_c_entries_refuse_bad_arguments():
    lib = _lib.load()
    case, g = fixture("interp_p1_small")
    model = case.model()
    tables = case.tables
    lattice, ref, alpha_ref = (np.ascontiguousarray(g[k], dtype=np.float64) for k in ("lattice", "ref_positions", "alpha_ref"))
    basis = np.ascontiguousarray(case.basis, dtype=np.float64)
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

    def create(atoms=7, dofs=19, orders=tables.orders, offsets=tables.piece_offsets, lattice_ptr=ptr(lattice)):
        handle = C.c_void_p()
        rc = lib.rn_interp_create(atoms, lattice_ptr, ptr(ref), ptr(alpha_ref), dofs, ptr(basis), ptr(offsets),
                                  ptr(tables.breakpoints), ptr(orders), ptr(tables.coefficients), 0, C.byref(handle))
        assert rc == _lib.RN_OK or not handle.value
        return rc, handle

    invalid = _lib.RN_ERR_INVALID_ARGUMENT
    assert create(lattice_ptr=None)[0] == invalid
    assert create(dofs=0)[0] == invalid and create(atoms=0)[0] == invalid
    for bad in (0, 6):
        orders = tables.orders.copy()
        orders[4] = bad
        assert create(orders=orders)[0] == invalid
        assert b"DOF 4" in lib.rn_interp_last_error(None)
    offsets = tables.piece_offsets.copy()
    offsets[3] = offsets[2]
    assert create(offsets=offsets)[0] == invalid
    rc, handle = create()
    assert rc == _lib.RN_OK and lib.rn_interp_is_symmetric(handle) == 1
    try:
        positions = _cuda(g["positions"])
        pos, out = C.c_void_p(positions.data_ptr()), C.c_void_p(torch.empty(40 * 6 * 21, dtype=torch.float64, device="cuda:0").data_ptr())
        labels = np.zeros(7, dtype=np.int32)
        disp = np.zeros((2, 7, 3))
        assert lib.rn_interp_forward_device(handle, None, 40, out, None) == invalid
        assert lib.rn_interp_forward_device(handle, pos, 40, None, None) == invalid
        assert lib.rn_interp_forward_device(handle, pos, 0, out, None) == invalid
        assert lib.rn_interp_forward_device(None, pos, 40, out, None) == invalid
        assert lib.rn_interp_jacobian_device(handle, pos, 0, out, None) == invalid
        assert lib.rn_interp_calc_polarizabilities(handle, None, 3, None) == invalid
        assert lib.rn_interp_calc_polarizabilities(handle, None, -1, None) == invalid
        assert lib.rn_interp_calc_polarizabilities(handle, None, 0, None) == _lib.RN_OK
        assert lib.rn_interp_set_mask(handle, None) == invalid
        assert lib.rn_interp_group_increments_device(handle, pos, 1, ptr(labels), 1, 0, out, None) == invalid
        assert lib.rn_interp_group_increments_device(handle, pos, 40, None, 1, 0, out, None) == invalid
        for groups in (0, 17):
            assert lib.rn_interp_group_increments_device(handle, pos, 40, ptr(labels), groups, 0, out, None) == invalid
        assert lib.rn_interp_group_increments_device(handle, pos, 40, ptr(labels), 2, 0, out, None) == invalid  # an empty group
        assert b"empty group" in lib.rn_interp_last_error(handle)
        assert lib.rn_interp_mode_increments_device(handle, pos, 1, ptr(disp), ptr(disp), 2, 1, 0, out, None) == invalid
        assert lib.rn_interp_mode_increments_device(handle, pos, 40, ptr(disp), None, 2, 1, 0, out, None) == invalid
        assert lib.rn_interp_mode_increments_device(handle, pos, 40, ptr(disp), ptr(disp), 0, 1, 0, out, None) == invalid
        assert lib.rn_interp_mode_increments_device(handle, pos, 40, ptr(disp), ptr(disp), 2, 2, 0, out, None) == invalid
        assert lib.rn_interp_partial_raman_tensors(handle, ptr(ref), ptr(disp), 2, ptr(labels), 0, ptr(disp)) == invalid
        assert lib.rn_interp_partial_raman_tensors(handle, None, ptr(disp), 2, ptr(labels), 1, ptr(disp)) == invalid
        # and the handle still works
        alpha = np.empty((40, 3, 3))
        assert lib.rn_interp_calc_polarizabilities(handle, ptr(g["positions"]), 40, ptr(alpha)) == _lib.RN_OK
        np.testing.assert_array_equal(alpha, model.calc_polarizabilities(g["positions"]))
    finally:
        lib.rn_interp_destroy(handle)
