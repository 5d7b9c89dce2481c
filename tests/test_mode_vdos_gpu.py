"""The on-device mode-projected VDOS (``rn_md_mode_vdos`` / ``rn_md_mode_vdos_device``) against the host path: shapes at
which the projection kernel's tiles can go wrong, Parseval against ``rn_md_vdos``, blocking, determinism, the entry
checks and the device-resident classes.  Every comparison is per row: ``max|got - want| / max|want|`` of that row, so
that a weak mode's row is not hidden behind a strong one."""
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

from ramannoodle_amd import _lib
from ramannoodle_amd.dynamics import Phonons, Trajectory, TrajectoryEnsemble
from ramannoodle_amd.spectrum import (DeviceModeVibrationalDensityOfStates,
                                      DeviceModeVibrationalDensityOfStatesEnsemble, ModeVibrationalDensityOfStates,
                                      VibrationalDensityOfStates, _mode_vdos_on_device, _segment_starts, mode_vectors,
                                      segment_plan)
from tests.conftest import load_golden
from tests.helpers import product_model_from_golden
from tests.test_polarized_spectra_gpu import _sleep_cycles
from tests.test_vdos_gpu import DT, LATTICE, _run

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _vectors(atoms, modes, orthonormal=False):
    """``modes`` seeded vectors ``(modes, atoms, 3)`` of very different sizes (a factor 1e3 between rows), or the first
    ``modes`` of a random orthonormal basis."""
    rng = np.random.default_rng(7 * atoms + modes)
    if orthonormal:
        q, _ = np.linalg.qr(rng.normal(size=(3 * atoms, 3 * atoms)))
        return np.ascontiguousarray(q.T[:modes].reshape(modes, atoms, 3))
    return rng.normal(size=(modes, atoms, 3)) * np.logspace(-1.5, 1.5, modes)[:, None, None]


def _row_errors(got, want):
    scale = np.abs(want).max(axis=-1)
    assert np.all(scale > 0)
    return np.abs(got - want).max(axis=-1) / scale


def _close(got, want, tol):
    assert got.shape == want.shape
    if want.size:
        err = _row_errors(got, want).max()
        print(f"largest relative error of a row {err:.3e} (bound {tol:g})")
        assert err <= tol


CASES = [  # (S, N, M, W, hop, taper, a lattice per frame)
    (3, 1, 1, 3, None, "boxcar", False),           # 3N = 3 < one k-step; one step
    (50, 5, 15, 50, None, "boxcar", False),        # M = 3N < one 16-mode tile
    (64, 67, 17, 17, 8, "hann", False),            # two atom tiles and 3 atoms; 3N = 201 = 1 mod 4; M crosses 16
    (257, 130, 65, 65, 16, "blackman", True),      # n = 64: one time tile; M crosses a 64-mode tile; midpoint lattices
    (4097, 3, 9, 4097, None, "boxcar", False),     # 64 time tiles, L = 8192
]


@pytest.mark.parametrize("steps,atoms,modes,width,hop,taper,per_frame", CASES)
def test_device_matches_the_host_path(steps, atoms, modes, width, hop, taper, per_frame):
    f, lattice, masses, _ = _run(steps, atoms, 1, per_frame)
    vdos = ModeVibrationalDensityOfStates(f, DT, lattice, _vectors(atoms, modes), masses)
    assert vdos.num_modes == modes
    if width == steps:
        w_host, want = vdos.measure()
        w_dev, got = vdos.measure(device=0)
        np.testing.assert_array_equal(w_dev, w_host)
        assert got.shape == (modes, (width - 1 + 1) // 2 - 1)
        _close(got, want, 1e-10)
        hop = width
    for average in (True, False):
        w_host, want = vdos.measure_segments(width, hop, taper, average)
        w_dev, got = vdos.measure_segments(width, hop, taper, average, device=0)
        np.testing.assert_array_equal(w_dev, w_host)
        _close(got, want, 1e-10)


def test_an_orthonormal_basis_sums_to_the_device_vdos():
    f, lattice, masses, _ = _run(130, 33, 1)
    modes = ModeVibrationalDensityOfStates(f, DT, lattice, _vectors(33, 99, True), masses)
    whole = VibrationalDensityOfStates(f, DT, lattice, masses)
    _close(modes.measure(device=0)[1].sum(axis=0, keepdims=True), whole.measure(device=0)[1], 1e-10)
    for average in (True, False):
        got = modes.measure_segments(33, 16, "hann", average, device=0)[1].sum(axis=-2, keepdims=True)
        _close(got, whole.measure_segments(33, 16, "hann", average, device=0)[1], 1e-10)


def _blocking_case():
    f, lattice, masses, _ = _run(257, 130, 1, True)
    width, hop, tau = segment_plan(257, 65, 16, "blackman")
    return f, lattice, masses, _vectors(130, 65), width, tau, _segment_starts(257, width, hop)


def _reduce(case, average, limit=0, starts=None):
    f, lattice, masses, vectors, width, tau, table = case
    return _mode_vdos_on_device(f, lattice, masses, vectors, DT, width, table if starts is None else starts, tau,
                                average, 0, workspace_limit=limit)[1]


def test_workspace_limit_blocks_modes_and_segments():
    case = _blocking_case()
    atoms, modes, n, segments = 130, 65, 64, len(case[-1])
    length, bins = 128, 31
    per_series = length * 16               # one mode's series of one segment
    per_row = length * 16 + bins * 8       # one row's power spectrum and bins
    base = n * 8 + segments * 8 + modes * 3 * atoms * 8  # the taper, the start table, the weighted vectors
    limits = {
        "several mode blocks of one segment": base + 20 * (per_series + per_row),
        "blocks of a few segments": base + 4 * modes * (per_series + per_row),
        "one series and one row": base + per_series + per_row + 100,
    }
    assert limits["several mode blocks of one segment"] < base + modes * (per_series + per_row)
    assert limits["blocks of a few segments"] < base + segments * modes * per_series
    for average in (True, False):
        full = _reduce(case, average)
        for name, limit in limits.items():
            print(name, limit)
            _close(_reduce(case, average, limit), full, 1e-13)
        with pytest.raises(MemoryError):
            _reduce(case, average, 1000)


def test_repeated_calls_are_bit_identical_and_rows_follow_the_table():
    case = _blocking_case()
    for average in (True, False):
        first = _reduce(case, average)
        np.testing.assert_array_equal(_reduce(case, average), first)
    rows = _reduce(case, False)
    np.testing.assert_array_equal(_reduce(case, False, starts=case[-1][::-1].copy()), rows[::-1])


def _phase_times(lib):
    millis = (C.c_double * 4)(-1.0, -1.0, -1.0, -1.0)
    assert lib.rn_md_mode_vdos_phase_times(millis) == _lib.RN_OK
    return np.array(millis)


@pytest.mark.parametrize("average", (True, False))
def test_phase_times_are_kept_only_while_profiling(average):
    """Several mode blocks of one segment, so that every phase runs more than once per call."""
    lib = _lib.load()
    case = _blocking_case()
    limit = 64 * 8 + len(case[-1]) * 8 + 65 * 3 * 130 * 8 + 20 * (128 * 16 + 128 * 16 + 31 * 8)
    plain = _reduce(case, average, limit)
    np.testing.assert_array_equal(_phase_times(lib), np.zeros(4))
    assert lib.rn_md_mode_vdos_set_profiling(1) == _lib.RN_OK
    try:
        t0 = time.perf_counter()
        profiled = _reduce(case, average, limit)
        wall_ms = 1e3 * (time.perf_counter() - t0)
        millis = _phase_times(lib)
    finally:
        assert lib.rn_md_mode_vdos_set_profiling(0) == _lib.RN_OK
    np.testing.assert_array_equal(profiled, plain)
    print(f"projection, forward FFTs, power, back half: {millis} ms; the call took {wall_ms:.3f} ms")
    assert np.isfinite(millis).all() and np.all(millis > 0)
    assert millis.sum() <= wall_ms
    np.testing.assert_array_equal(_phase_times(lib), np.zeros(4))
    assert lib.rn_md_mode_vdos_phase_times(None) == _lib.RN_ERR_INVALID_ARGUMENT


def test_raw_entry_checks():
    lib = _lib.load()
    steps, atoms, modes, width = 20, 4, 5, 9
    f, lattice, masses, _ = _run(steps, atoms, 1)
    f = np.ascontiguousarray(f)
    lattices = np.ascontiguousarray(lattice[None])
    vectors = _vectors(atoms, modes)
    tau = np.ones(width - 1)
    starts = np.array([0, 5, steps - width], dtype=np.int64)
    bins = (width - 1 + 1) // 2 - 1
    out = np.full((3, modes, bins), -7.0)
    names = ("positions", "lattices", "num_lattices", "S", "N", "masses", "vectors", "M", "segment_steps", "starts", "Q",
             "taper", "average", "device", "workspace_limit", "densities", "num_bins")
    good = {"positions": f, "lattices": lattices, "num_lattices": 1, "S": steps, "N": atoms, "masses": masses,
            "vectors": vectors, "M": modes, "segment_steps": width, "starts": starts, "Q": 3, "taper": tau, "average": 0,
            "device": 0, "workspace_limit": 0, "densities": out, "num_bins": bins}

    assert tuple(good) == names  # the order of the C arguments

    def call(**changes):
        args = dict(good, **changes)
        keep = [np.ascontiguousarray(v) if isinstance(v, np.ndarray) and v is not out else v for v in args.values()]
        raw = [C.c_void_p(v.ctypes.data) if isinstance(v, np.ndarray) else (C.c_void_p(None) if v is None else v)
               for v in keep]
        return lib.rn_md_mode_vdos(*raw)

    def spoiled(value):
        bad = vectors.copy()
        bad[modes - 1, atoms - 1, 2] = value
        return bad

    invalid = [
        *({name: None} for name in ("positions", "lattices", "masses", "vectors", "starts", "taper", "densities")),
        {"N": 0}, {"M": 0}, {"M": -1}, {"M": 3 * atoms + 1}, {"num_lattices": 2}, {"num_lattices": 0},
        {"segment_steps": 2}, {"segment_steps": steps + 1}, {"Q": 0}, {"num_bins": bins + 1}, {"average": 2},
        {"average": -1}, {"starts": np.array([0, -1, 3], dtype=np.int64)},
        {"starts": np.array([0, 5, steps - width + 1], dtype=np.int64)},
        {"masses": np.array([1.0, 0.0, 1.0, 1.0])}, {"masses": np.array([1.0, -2.0, 1.0, 1.0])},
        {"masses": np.array([1.0, np.nan, 1.0, 1.0])}, {"masses": np.array([1.0, np.inf, 1.0, 1.0])},
        {"vectors": spoiled(np.nan)}, {"vectors": spoiled(np.inf)}, {"vectors": spoiled(-np.inf)},
    ]
    for changes in invalid:
        assert call(**changes) == _lib.RN_ERR_INVALID_ARGUMENT, changes
        assert np.all(out == -7.0), changes
    assert call(device=4096) == _lib.RN_ERR_NO_DEVICE
    assert call(workspace_limit=1000) == _lib.RN_ERR_OUT_OF_MEMORY
    assert np.all(out == -7.0)
    assert call() == _lib.RN_OK
    want = ModeVibrationalDensityOfStates(f, DT, lattice, vectors, masses).measure_segments(
        width, 5, "boxcar", average=False)[1]
    _close(out[:2], want[:2], 1e-10)
    # the _device entry makes the same checks and returns the same bits
    device_entry = lib.rn_md_mode_vdos_device
    tensors = torch.tensor(f, device="cuda"), torch.tensor(lattices, device="cuda")
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    again = np.full_like(out, -7.0)
    rc = device_entry(C.c_void_p(tensors[0].data_ptr()), C.c_void_p(tensors[1].data_ptr()), 1, steps, atoms, p(masses),
                      p(vectors), 3 * atoms + 1, width, p(starts), 3, p(tau), 0, 0, 0, p(again), bins, C.c_void_p(None))
    assert rc == _lib.RN_ERR_INVALID_ARGUMENT
    rc = device_entry(C.c_void_p(tensors[0].data_ptr()), C.c_void_p(tensors[1].data_ptr()), 1, steps, atoms, p(masses),
                      p(spoiled(np.nan)), modes, width, p(starts), 3, p(tau), 0, 0, 0, p(again), bins, C.c_void_p(None))
    assert rc == _lib.RN_ERR_INVALID_ARGUMENT
    assert np.all(again == -7.0)
    rc = device_entry(C.c_void_p(tensors[0].data_ptr()), C.c_void_p(tensors[1].data_ptr()), 1, steps, atoms, p(masses),
                      p(vectors), modes, width, p(starts), 3, p(tau), 0, 0, 0, p(again), bins, C.c_void_p(None))
    assert rc == _lib.RN_OK
    np.testing.assert_array_equal(again, out)


def _phonons(atoms, modes):
    rng = np.random.default_rng(atoms + modes)
    return Phonons(rng.random((atoms, 3)), np.linspace(50.0, 900.0, modes), 0.1 * rng.normal(size=(modes, atoms, 3)))


def test_device_resident_path_equals_the_host_input_call():
    for per_frame in (False, True):
        f, lattice, masses, _ = _run(257, 130, 1, per_frame)
        trajectory = Trajectory(f, DT, lattice if per_frame else None)
        arguments = dict(phonons=_phonons(130, 65), lattice=LATTICE, masses=masses)
        resident = trajectory.get_mode_vdos(on_device=True, **arguments)
        assert isinstance(resident, DeviceModeVibrationalDensityOfStates) and resident.num_modes == 65
        plain = trajectory.get_mode_vdos(**arguments)
        for average in (True, False):
            w_res, got = resident.measure_segments(65, 16, "blackman", average)
            w_host, want = plain.measure_segments(65, 16, "blackman", average, device=0)
            np.testing.assert_array_equal(w_res, w_host)
            np.testing.assert_array_equal(got, want)
        _close(resident.measure(host=True)[1], resident.measure()[1], 1e-10)


def test_device_resident_ensemble_equals_the_host_input_call():
    masses = _run(130, 33, 1)[2]
    runs = [Trajectory(_run(steps, 33, 1)[0], DT) for steps in (130, 97)]
    ensemble = TrajectoryEnsemble(runs)
    arguments = dict(phonons=_phonons(33, 20), lattice=LATTICE, masses=masses, modes=np.arange(0, 20, 2))
    resident = ensemble.get_mode_vdos(on_device=True, **arguments)
    assert isinstance(resident, DeviceModeVibrationalDensityOfStatesEnsemble) and resident.num_modes == 10
    plain = ensemble.get_mode_vdos(**arguments)
    for average in (True, False):
        w_res, got = resident.measure_segments(33, 16, "hann", average)
        w_host, want = plain.measure_segments(33, 16, "hann", average, device=0)
        np.testing.assert_array_equal(w_res, w_host)
        np.testing.assert_array_equal(got, want)
        _close(resident.measure_segments(33, 16, "hann", average, host=True)[1], got, 1e-10)
    assert got.shape[0] == len(resident.segment_starts(33, 16)[0])


def test_waits_for_the_producer_stream():
    """The positions are written on a side stream behind a bounded sleep; the reduction, called with that stream
    current, must see the finished positions."""
    f, lattice, masses, _ = _run(4097, 3, 1)
    vectors = _vectors(3, 9)
    _, want = ModeVibrationalDensityOfStates(f, DT, lattice, vectors, masses).measure()
    source = torch.tensor(f, device="cuda")
    target = torch.zeros_like(source)
    vdos = DeviceModeVibrationalDensityOfStates(target, DT, lattice, vectors, masses)
    vdos.measure()  # plans and buffers made outside the window
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vdos.measure()
    call_ms = 1e3 * (time.perf_counter() - t0)
    cycles = _sleep_cycles()
    side = torch.cuda.Stream()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        start.record()
        torch.cuda._sleep(cycles)
        end.record()
        target.copy_(source)
        _, got = vdos.measure()
    torch.cuda.synchronize()
    slept = start.elapsed_time(end)
    assert slept <= 2000.0, f"the sleep held the stream {slept:.0f} ms"
    assert slept >= 10.0 * call_ms, f"the sleep held the stream {slept:.1f} ms, a call takes {call_ms:.2f} ms"
    _close(got, want, 1e-10)


def test_raman_spectrum_vdos_and_mode_vdos_of_one_trajectory_share_their_axis():
    g = load_golden("triclinic20")
    model = product_model_from_golden(g)
    positions = np.asarray(g["md/positions"], dtype=np.float64)
    trajectory = Trajectory(positions, float(g["md/timestep"]))
    w_raman, _ = trajectory.get_raman_spectrum(model, on_device=True).measure()
    lattice = np.asarray(g["lattice"], dtype=np.float64).reshape(3, 3)
    w_vdos, _ = trajectory.get_vdos(lattice, on_device=True, device=model.device_index).measure()
    atoms = positions.shape[1]
    w_modes, densities = trajectory.get_mode_vdos(_phonons(atoms, 3 * atoms), lattice, on_device=True,
                                                  device=model.device_index).measure()
    np.testing.assert_array_equal(w_modes, w_raman)
    np.testing.assert_array_equal(w_modes, w_vdos)
    assert densities.shape == (3 * atoms, len(w_raman))
    peaks = densities.max(axis=1)
    assert np.isfinite(densities).all() and np.all(peaks > 0)
