"""The on-device VDOS reducer (``rn_md_vdos`` / ``rn_md_vdos_device``) against the host path: shapes at which the
builder's tiles, the atom and segment blocks and the group ranges can go wrong; blocking, determinism, the entry checks
and the device-resident path."""
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

from ramannoodle_amd import _lib
from ramannoodle_amd.dynamics import Trajectory
from ramannoodle_amd.spectrum import (DeviceVibrationalDensityOfStates, VibrationalDensityOfStates, _segment_starts,
                                      _vdos_on_device, segment_plan)
from ramannoodle_amd.structure import apply_pbc
from tests.conftest import load_golden
from tests.helpers import product_model_from_golden
from tests.test_polarized_spectra_gpu import _sleep_cycles

pytestmark = pytest.mark.gpu

LATTICE = np.array([[4.0, 0.3, 0.0], [0.1, 5.0, 0.2], [0.0, -0.4, 6.0]])
DT = 1.5


@functools.lru_cache(maxsize=None)
def _run(steps, atoms, groups, per_frame=False):
    """``(wrapped positions, lattice(s), masses, labels)``: atoms that drift through cell faces, steps below 0.4 of a
    cell; group ``groups - 1`` has one atom (atoms permitting), the others are dealt round robin."""
    rng = np.random.default_rng(steps * 1000 + atoms)
    t = np.arange(steps)[:, None, None]
    phase = 0.3 * t * (1 + np.arange(atoms) % 7)[None, :, None] + rng.random((atoms, 3))
    drift = np.clip(0.1 * rng.normal(size=(atoms, 3)), -0.25, 0.25)
    f = rng.random((atoms, 3)) + 0.03 * np.sin(phase) + t * drift * min(1.0, 30.0 / steps)
    assert np.abs(np.diff(f, axis=0)).max() < 0.4
    labels = np.arange(atoms) % max(groups - 1, 1)
    labels[atoms // 2] = groups - 1
    if len(np.unique(labels)) != groups:  # (fewer atoms than groups cannot happen in the cases below)
        raise AssertionError("a group is empty")
    lattice = LATTICE
    if per_frame:
        strain = 1.0 + 0.02 * np.sin(0.05 * np.arange(steps))[:, None, None] * rng.random((1, 3, 3))
        lattice = LATTICE[None] * strain
    return apply_pbc(f), lattice, rng.uniform(1.0, 100.0, atoms), labels.astype(np.int32)


def _close(got, want, tol):
    assert got.shape == want.shape
    if want.size:
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"relative error {err:.3e} (bound {tol:g})")
        assert err <= tol


CASES = [  # (S, N, G, W, hop, taper, a lattice per frame)
    (3, 1, 1, 3, None, "boxcar", False),
    (50, 5, 3, 50, None, "boxcar", False),
    (64, 67, 16, 17, 8, "hann", False),
    (257, 130, 2, 65, 16, "blackman", True),
    (4097, 3, 1, 4097, None, "boxcar", False),
]


@pytest.mark.parametrize("steps,atoms,groups,width,hop,taper,per_frame", CASES)
def test_device_matches_the_host_path(steps, atoms, groups, width, hop, taper, per_frame):
    f, lattice, masses, labels = _run(steps, atoms, groups, per_frame)
    vdos = VibrationalDensityOfStates(f, DT, lattice, masses, labels, groups)
    if width == steps:
        w_host, want = vdos.measure()
        w_dev, got = vdos.measure(device=0)
        np.testing.assert_array_equal(w_dev, w_host)
        assert got.shape == (groups, (width - 1 + 1) // 2 - 1)
        _close(got, want, 1e-10)
        hop = width
    for average in (True, False):
        w_host, want = vdos.measure_segments(width, hop, taper, average)
        w_dev, got = vdos.measure_segments(width, hop, taper, average, device=0)
        np.testing.assert_array_equal(w_dev, w_host)
        _close(got, want, 1e-10)


def _blocking_case():
    f, lattice, masses, labels = _run(257, 130, 2, True)
    width, hop, tau = segment_plan(257, 65, 16, "blackman")
    return f, lattice, masses, labels, width, tau, _segment_starts(257, width, hop)


def _reduce(case, average, limit=0):
    f, lattice, masses, labels, width, tau, starts = case
    return _vdos_on_device(f, lattice, masses, labels, 2, DT, width, starts, tau, average, 0, workspace_limit=limit)[1]


def test_workspace_limit_blocks_atoms_segments_and_groups():
    case = _blocking_case()
    atoms, groups, n, segments = 130, 2, 64, len(case[-1])
    length, bins = 128, 31
    per_atom = 3 * length * 16             # one atom's three series of one segment
    per_row = length * 16 + bins * 8       # one row's power spectrum and bins
    base = n * 8 + segments * 8 + atoms * 12  # the taper, the start table, sqrt(m) and the atom list
    limits = {
        "several atom blocks of one segment": base + groups * per_row + 40 * per_atom,
        "blocks of segments": base + 4 * (atoms * per_atom + groups * per_row),
        "one atom, one row: atom, segment and group blocks": base + per_atom + per_row + 100,
    }
    assert limits["blocks of segments"] < base + segments * atoms * per_atom
    for average in (True, False):
        full = _reduce(case, average)
        for name, limit in limits.items():
            print(name, limit)
            _close(_reduce(case, average, limit), full, 1e-13)
        with pytest.raises(MemoryError):
            _reduce(case, average, 1000)


def test_repeated_calls_are_bit_identical():
    case = _blocking_case()
    for average in (True, False):
        first = _reduce(case, average)
        np.testing.assert_array_equal(_reduce(case, average), first)


def _phase_times(lib):
    millis = (C.c_double * 4)(-1.0, -1.0, -1.0, -1.0)
    assert lib.rn_md_vdos_phase_times(millis) == _lib.RN_OK
    return np.array(millis)


@pytest.mark.parametrize("average", (True, False))
def test_phase_times_are_kept_only_while_profiling(average):
    """Several atom blocks of one segment, so that every phase runs more than once per call."""
    lib = _lib.load()
    case = _blocking_case()
    limit = 64 * 8 + len(case[-1]) * 8 + 130 * 12 + 2 * (128 * 16 + 31 * 8) + 40 * (3 * 128 * 16)
    plain = _reduce(case, average, limit)
    np.testing.assert_array_equal(_phase_times(lib), np.zeros(4))
    assert lib.rn_md_vdos_set_profiling(1) == _lib.RN_OK
    try:
        t0 = time.perf_counter()
        profiled = _reduce(case, average, limit)
        wall_ms = 1e3 * (time.perf_counter() - t0)
        millis = _phase_times(lib)
    finally:
        assert lib.rn_md_vdos_set_profiling(0) == _lib.RN_OK
    np.testing.assert_array_equal(profiled, plain)
    print(f"builder, forward FFTs, power, back half: {millis} ms; the call took {wall_ms:.3f} ms")
    assert np.isfinite(millis).all() and np.all(millis > 0)
    assert millis.sum() <= wall_ms
    np.testing.assert_array_equal(_phase_times(lib), np.zeros(4))
    assert lib.rn_md_vdos_phase_times(None) == _lib.RN_ERR_INVALID_ARGUMENT


def test_single_segment_and_start_table():
    f, lattice, masses, labels = _run(50, 5, 3)
    vdos = VibrationalDensityOfStates(f, DT, lattice, masses, labels, 3)
    _, whole = vdos.measure(device=0)
    _, one = vdos.measure_segments(50, taper="boxcar", device=0)
    np.testing.assert_array_equal(one, whole)
    width, hop, tau = segment_plan(50, 17, 8, "hann")
    table = np.arange((50 - 17) // 8 + 1, dtype=np.int64) * 8
    _, rows = vdos.measure_segments(17, 8, "hann", average=False, device=0)
    _, at = _vdos_on_device(f, vdos._lattices, masses, labels, 3, DT, width, table, tau, False, 0)
    np.testing.assert_array_equal(at, rows)
    _, reversed_rows = _vdos_on_device(f, vdos._lattices, masses, labels, 3, DT, width, table[::-1].copy(), tau, False, 0)
    np.testing.assert_array_equal(reversed_rows, rows[::-1])


def test_raw_entry_checks():
    lib = _lib.load()
    steps, atoms, groups, width = 20, 4, 2, 9
    f, lattice, masses, labels = _run(steps, atoms, groups)
    f = np.ascontiguousarray(f)
    lattices = np.ascontiguousarray(lattice[None])
    tau = np.ones(width - 1)
    starts = np.array([0, 5, steps - width], dtype=np.int64)
    bins = (width - 1 + 1) // 2 - 1
    out = np.full((3, groups, bins), -7.0)
    names = ("positions", "lattices", "num_lattices", "S", "N", "masses", "labels", "G", "segment_steps", "starts", "Q",
             "taper", "average", "device", "workspace_limit", "densities", "num_bins")
    good = {"positions": f, "lattices": lattices, "num_lattices": 1, "S": steps, "N": atoms, "masses": masses,
            "labels": labels, "G": groups, "segment_steps": width, "starts": starts, "Q": 3, "taper": tau, "average": 0,
            "device": 0, "workspace_limit": 0, "densities": out, "num_bins": bins}

    assert tuple(good) == names  # the order of the C arguments

    def call(**changes):
        args = dict(good, **changes)
        keep = [np.ascontiguousarray(v) if isinstance(v, np.ndarray) and v is not out else v for v in args.values()]
        raw = [C.c_void_p(v.ctypes.data) if isinstance(v, np.ndarray) else (C.c_void_p(None) if v is None else v)
               for v in keep]
        return lib.rn_md_vdos(*raw)

    invalid = [
        *({name: None} for name in ("positions", "lattices", "masses", "labels", "starts", "taper", "densities")),
        {"N": 0}, {"G": 0}, {"G": 17}, {"num_lattices": 2}, {"num_lattices": 0}, {"segment_steps": 2},
        {"segment_steps": steps + 1}, {"Q": 0}, {"num_bins": bins + 1}, {"average": 2}, {"average": -1},
        {"starts": np.array([0, -1, 3], dtype=np.int64)}, {"starts": np.array([0, 5, steps - width + 1], dtype=np.int64)},
        {"labels": np.array([0, 1, 2, 0], dtype=np.int32)}, {"labels": np.array([0, -1, 1, 0], dtype=np.int32)},
        {"masses": np.array([1.0, 0.0, 1.0, 1.0])}, {"masses": np.array([1.0, -2.0, 1.0, 1.0])},
        {"masses": np.array([1.0, np.nan, 1.0, 1.0])}, {"masses": np.array([1.0, np.inf, 1.0, 1.0])},
    ]
    for changes in invalid:
        assert call(**changes) == _lib.RN_ERR_INVALID_ARGUMENT, changes
        assert np.all(out == -7.0), changes
    assert call(device=4096) == _lib.RN_ERR_NO_DEVICE
    assert call(workspace_limit=1000) == _lib.RN_ERR_OUT_OF_MEMORY
    assert np.all(out == -7.0)
    assert call() == _lib.RN_OK
    want = VibrationalDensityOfStates(f, DT, lattice, masses, labels, groups).measure_segments(
        width, 5, "boxcar", average=False)[1]
    _close(out[:2], want[:2], 1e-10)
    # the _device entry makes the same checks
    device_entry = lib.rn_md_vdos_device
    tensors = torch.tensor(f, device="cuda"), torch.tensor(lattices, device="cuda")
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    rc = device_entry(C.c_void_p(tensors[0].data_ptr()), C.c_void_p(tensors[1].data_ptr()), 1, steps, atoms, p(masses),
                      p(labels), 17, width, p(starts), 3, p(tau), 0, 0, 0, p(out), bins, C.c_void_p(None))
    assert rc == _lib.RN_ERR_INVALID_ARGUMENT
    again = np.empty_like(out)
    rc = device_entry(C.c_void_p(tensors[0].data_ptr()), C.c_void_p(tensors[1].data_ptr()), 1, steps, atoms, p(masses),
                      p(labels), groups, width, p(starts), 3, p(tau), 0, 0, 0, p(again), bins, C.c_void_p(None))
    assert rc == _lib.RN_OK
    np.testing.assert_array_equal(again, out)


def test_device_resident_path_equals_the_host_input_call():
    for per_frame in (False, True):
        f, lattice, masses, labels = _run(257, 130, 2, per_frame)
        trajectory = Trajectory(f, DT, lattice if per_frame else None)
        arguments = dict(lattice=None if per_frame else lattice, masses=masses, groups=labels)
        resident = trajectory.get_vdos(on_device=True, **arguments)
        assert isinstance(resident, DeviceVibrationalDensityOfStates)
        plain = trajectory.get_vdos(**arguments)
        for average in (True, False):
            w_res, got = resident.measure_segments(65, 16, "blackman", average)
            w_host, want = plain.measure_segments(65, 16, "blackman", average, device=0)
            np.testing.assert_array_equal(w_res, w_host)
            np.testing.assert_array_equal(got, want)
        _close(resident.measure(host=True)[1], resident.measure()[1], 1e-10)


def test_waits_for_the_producer_stream():
    """The positions are written on a side stream behind a bounded sleep; the reduction, called with that stream
    current, must see the finished positions."""
    f, lattice, masses, labels = _run(4097, 3, 1)
    _, want = VibrationalDensityOfStates(f, DT, lattice, masses, labels, 1).measure()
    source = torch.tensor(f, device="cuda")
    target = torch.zeros_like(source)
    vdos = DeviceVibrationalDensityOfStates(target, DT, lattice, masses, labels, 1)
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


def test_raman_spectrum_and_vdos_of_one_trajectory_share_their_axis():
    g = load_golden("triclinic20")
    model = product_model_from_golden(g)
    trajectory = Trajectory(g["md/positions"], float(g["md/timestep"]))
    w_raman, intensities = trajectory.get_raman_spectrum(model, on_device=True).measure()
    lattice = np.asarray(g["lattice"], dtype=np.float64).reshape(3, 3)
    w_vdos, densities = trajectory.get_vdos(lattice, on_device=True, device=model.device_index).measure()
    np.testing.assert_array_equal(w_vdos, w_raman)
    assert densities.shape == (1, len(w_raman))
    assert np.isfinite(intensities).all() and np.isfinite(densities).all() and densities.max() > 0
