"""MD Raman spectra over several runs and segment spectra by atom group, reduced on the GPU (``rn_md_raman_segments_at``,
``rn_md_raman_partial_segments`` and their ``_device`` forms) against the host paths: run lengths, segment lengths, hops,
tapers, group and configuration counts, the start table on a hop grid against ``rn_md_raman_segments`` bit for bit, one
boxcar segment against ``rn_md_raman_partial``, segment blocks and row sub-blocks under a small workspace, the argument
checks, determinism, separate plan caches, the device-resident path through ``TrajectoryEnsemble`` and ordering behind
work still queued on the caller's stream.  Every GPU step is small and bounded."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from ramannoodle_amd import _lib
from ramannoodle_amd.spectrum import (DeviceMDRamanEnsemble, DevicePartialMDRamanEnsemble,
                                      DevicePartialMDRamanSpectrum, MDRamanEnsemble, PartialMDRamanEnsemble,
                                      PartialMDRamanSpectrum, _md_intensities_on_device,
                                      _md_partial_segments_on_device, _md_segments_at_on_device,
                                      ensemble_segment_starts, polarized_weights, segment_plan)
from tests.conftest import load_golden
from tests.helpers import product_model_from_golden
from tests.test_polarized_spectra_gpu import (CORRECTIONS, _close, _configurations, _polarized, _series,
                                              _sleep_cycles)
from tests.test_segment_spectra_gpu import _segments

pytestmark = pytest.mark.gpu

# (run lengths, W, H, K, taper): one segment; three unequal runs, odd n; W = 3 (no bins); no overlap and many
# configurations
SHAPES = [([64], 64, 1, 7, "hann"), ([50, 81, 64], 17, 5, 1, "blackman"), ([50, 40], 3, 1, 7, "hamming"),
          ([1001, 700], 100, 100, 720, "hann")]


@pytest.fixture(autouse=True)
def _no_default_device_mode():
    torch.set_default_device(None)
    yield


def _p(array):
    return None if array is None else C.c_void_p(array.ctypes.data)


def _runs(lengths, seed):
    return [_series(steps, seed + 7 * r) for r, steps in enumerate(lengths)]


def _increment_runs(lengths, groups, seed):
    """Per-group increments ``(S_r - 1, G, 3, 3)`` of each run, symmetric."""
    rng = np.random.default_rng(seed)
    runs = []
    for steps in lengths:
        t = np.arange(steps - 1)[:, None, None, None]
        freq = 1 + np.arange(groups * 9).reshape(1, groups, 3, 3) % 23
        incr = 0.05 * rng.normal(size=(steps - 1, groups, 3, 3)) + np.cos(0.01 * t * freq + rng.uniform(0, 6))
        runs.append(incr + np.swapaxes(incr, 2, 3))
    return runs


def _bins(width):
    return width // 2 - 1  # ceil((W - 1) / 2) - 1


def _segments_at(alpha, width, starts, tau, weights, average, limit=0):
    """Raw ``rn_md_raman_segments_at``: (status, intensities)."""
    alpha = np.ascontiguousarray(alpha, dtype=np.float64)
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    starts = np.ascontiguousarray(starts, dtype=np.int64)
    count = weights.shape[0]
    out = np.full((count, _bins(width)) if average else (len(starts), count, _bins(width)), np.nan)
    rc = _lib.load().rn_md_raman_segments_at(_p(alpha), alpha.shape[0], width, _p(starts), len(starts), _p(tau),
                                             _p(weights), count, int(average), 0, limit, _p(out), _bins(width))
    return rc, out


def _partial_segments(incr, width, starts, tau, weights, average, limit=0):
    """Raw ``rn_md_raman_partial_segments``: (status, packed intensities)."""
    incr = np.ascontiguousarray(incr, dtype=np.float64)
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    starts = np.ascontiguousarray(starts, dtype=np.int64)
    count, groups = weights.shape[0], incr.shape[1]
    pairs = groups * (groups + 1) // 2
    out = np.full((count, pairs, _bins(width)) if average else (len(starts), count, pairs, _bins(width)), np.nan)
    rc = _lib.load().rn_md_raman_partial_segments(_p(incr), incr.shape[0], groups, width, _p(starts), len(starts),
                                                  _p(tau), _p(weights), count, int(average), 0, limit, _p(out),
                                                  _bins(width))
    return rc, out


@pytest.mark.parametrize("lengths,width,hop,k,taper", SHAPES)
def test_device_matches_host(lengths, width, hop, k, taper):
    e_i, e_s, rotations = _configurations(k, k)
    ensemble = MDRamanEnsemble(_runs(lengths, sum(lengths)), 1.5)
    segments = {"segment_steps": width, "hop": hop, "taper": taper}
    for average in (True, False):
        for kwargs in ({}, CORRECTIONS):
            w_host, i_host = ensemble.measure_segments_polarized(e_i, e_s, rotations, average=average, **segments,
                                                                 **kwargs)
            w_dev, i_dev = ensemble.measure_segments_polarized(e_i, e_s, rotations, average=average, device=0,
                                                               **segments, **kwargs)
            np.testing.assert_array_equal(w_dev, w_host)
            _close(i_dev, i_host, 1e-10)
        _, i_host = ensemble.measure_segments(average=average, **segments)
        _, i_dev = ensemble.measure_segments(average=average, device=0, **segments)
        _close(i_dev, i_host, 1e-10)
    if len(set(lengths)) == 1:
        _close(ensemble.measure(device=0)[1], ensemble.measure()[1], 1e-10)


@pytest.mark.parametrize("k", [1, 7])
@pytest.mark.parametrize("groups", [1, 3, 16])
@pytest.mark.parametrize("lengths,width,hop,taper", [shape[:3] + shape[4:] for shape in SHAPES])
def test_device_partial_matches_host(lengths, width, hop, taper, groups, k):
    e_i, e_s, rotations = _configurations(k, k + groups)
    ensemble = PartialMDRamanEnsemble(_increment_runs(lengths, groups, sum(lengths) + groups), 1.5)
    segments = {"segment_steps": width, "hop": hop, "taper": taper}
    rows = len(ensemble_segment_starts(lengths, width, hop)[0])
    for average in (True, False):
        for kwargs in ({}, CORRECTIONS):
            w_host, i_host = ensemble.measure_segments_polarized(e_i, e_s, rotations, average=average, **segments,
                                                                 **kwargs)
            w_dev, i_dev = ensemble.measure_segments_polarized(e_i, e_s, rotations, average=average, device=0,
                                                               **segments, **kwargs)
            np.testing.assert_array_equal(w_dev, w_host)
            assert i_dev.shape == (() if average else (rows,)) + (k, groups, groups, len(w_host))
            _close(i_dev, i_host, 1e-10)
            np.testing.assert_array_equal(i_dev, np.swapaxes(i_dev, -2, -3))
        _, i_host = ensemble.measure_segments(average=average, **segments)
        _, i_dev = ensemble.measure_segments(average=average, device=0, **segments)
        _close(i_dev, i_host, 1e-10)
    # one series: PartialMDRamanSpectrum's own segments
    single = PartialMDRamanSpectrum(ensemble.increments[:lengths[0] - 1], 1.5)
    _, i_host = single.measure_segments(**segments)
    _, i_dev = single.measure_segments(device=0, **segments)
    _close(i_dev, i_host, 1e-10)


@pytest.mark.parametrize("steps,width,hop,k", [(257, 65, 16, 7), (2000, 256, 64, 720)])
def test_a_hop_grid_is_the_segment_entry_bit_for_bit(steps, width, hop, k):
    alpha = _series(steps, steps)
    e_i, e_s, rotations = _configurations(k, k)
    weights, _ = polarized_weights(e_i, e_s, rotations)
    _, _, tau = segment_plan(steps, width, hop, "hann")
    starts = np.arange((steps - width) // hop + 1) * hop
    for average in (True, False):
        rc, want = _segments(alpha, width, hop, tau, weights, average)
        assert rc == _lib.RN_OK
        rc, got = _segments_at(alpha, width, starts, tau, weights, average)
        assert rc == _lib.RN_OK
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("steps,groups", [(64, 3), (1000, 16), (4096, 1)])
def test_one_boxcar_segment_is_the_partial_entry(steps, groups):
    incr = _increment_runs([steps + 1], groups, steps)[0]
    e_i, e_s, rotations = _configurations(7, 11)
    weights, _ = polarized_weights(e_i, e_s, rotations)
    _, want = PartialMDRamanSpectrum(incr, 1.0).measure_polarized(e_i, e_s, rotations, device=0)
    for average in (True, False):
        _, got = _md_partial_segments_on_device(incr, 1.0, weights, steps + 1, [0], np.ones(steps), average, 0)
        _close(got.reshape(want.shape), want, 1e-10)


def test_workspace_limit_blocks_and_out_of_memory():
    lengths = [500, 501]
    width, hop, tau = segment_plan(500, 129, 32, "hann")
    starts, _ = ensemble_segment_starts(lengths, width, hop)
    e_i, e_s, rotations = _configurations(7, 4)
    weights, _ = polarized_weights(e_i, e_s, rotations)
    alpha = MDRamanEnsemble(_runs(lengths, 9), 1.0).polarizability_ts
    incr = PartialMDRamanEnsemble(_increment_runs(lengths, 3, 9), 1.0).increments
    # whole: a segment's components take 6 * 256 complex doubles (24 576 B) and a row 256 complex doubles and 63 bins
    # (4 600 B): 150 000 B hold three of the 24 segments and some of their 21 rows, 45 000 B one segment and three of
    # the 7 configurations.  By group (G = 3): a segment takes 73 728 B and there are 42 rows per segment: 300 000 B
    # hold two or three segments and some of their rows, 100 000 B one segment and five rows.
    for average in (True, False):
        rc, full = _segments_at(alpha, width, starts, tau, weights, average)
        assert rc == _lib.RN_OK
        for limit in (150_000, 45_000):
            rc, small = _segments_at(alpha, width, starts, tau, weights, average, limit=limit)
            assert rc == _lib.RN_OK, limit
            _close(small, full, 1e-10)
        rc, _ = _segments_at(alpha, width, starts, tau, weights, average, limit=1000)
        assert rc == _lib.RN_ERR_OUT_OF_MEMORY
        rc, full = _partial_segments(incr, width, starts, tau, weights, average)
        assert rc == _lib.RN_OK
        for limit in (300_000, 100_000):
            rc, small = _partial_segments(incr, width, starts, tau, weights, average, limit=limit)
            assert rc == _lib.RN_OK, limit
            _close(small, full, 1e-10)
        rc, _ = _partial_segments(incr, width, starts, tau, weights, average, limit=1000)
        assert rc == _lib.RN_ERR_OUT_OF_MEMORY
        with pytest.raises(MemoryError):
            _md_segments_at_on_device(alpha, 1.0, weights, width, starts, tau, average, 0, workspace_limit=1000)
        with pytest.raises(MemoryError):
            _md_partial_segments_on_device(incr, 1.0, weights, width, starts, tau, average, 0, workspace_limit=1000)


def test_argument_checks():
    lib = _lib.load()
    width, bins = 64, 31
    tau = np.ones(width - 1)
    weights = np.ones((2, 21))
    out = np.empty((3, 2, 3, bins + 1))  # room for a wrong num_bins that slips through
    alpha = _series(200, 1)
    incr = _increment_runs([200], 2, 1)[0]  # N = 199

    def starts_of(*values):
        return np.array(values, dtype=np.int64)

    table = starts_of(0, 50, 136)  # 136 = S - W = N + 1 - W: the last segment that fits
    names = ("source", "steps", "G", "segment_steps", "starts", "Q", "taper", "weights", "K", "average", "device",
             "workspace_limit", "intensities", "num_bins")
    good = {"source": None, "steps": None, "G": 2, "segment_steps": width, "starts": table, "Q": 3, "taper": tau,
            "weights": weights, "K": 2, "average": 0, "device": 0, "workspace_limit": 0, "intensities": out,
            "num_bins": bins}

    def call(entry, **changes):
        values = dict(good, **changes)
        args = [_p(values[name]) if name in ("source", "starts", "taper", "weights", "intensities") else values[name]
                for name in names if not (name == "G" and entry is lib.rn_md_raman_segments_at)]
        return entry(*args)

    for entry, source, steps in ((lib.rn_md_raman_segments_at, alpha, 200), (lib.rn_md_raman_partial_segments, incr, 199)):
        def check(entry=entry, source=source, steps=steps, **changes):
            return call(entry, **dict({"source": source, "steps": steps}, **changes))

        invalid = _lib.RN_ERR_INVALID_ARGUMENT
        for name in ("source", "starts", "taper", "weights", "intensities"):
            assert check(**{name: None}) == invalid, name
        assert check(K=0) == invalid
        assert check(Q=0) == invalid
        assert check(Q=-1) == invalid
        assert check(starts=starts_of(-1, 50, 136)) == invalid
        assert check(starts=starts_of(0, 50, 137)) == invalid  # start > S - W; start + W - 1 > N
        assert check(starts=starts_of(0, 1 << 40, 136)) == invalid
        assert check(segment_steps=2, num_bins=0) == invalid
        assert check(segment_steps=201, num_bins=99, starts=starts_of(0, 0, 0)) == invalid
        assert check(num_bins=bins + 1) == invalid
        assert check(num_bins=bins - 1) == invalid
        assert check(average=2) == invalid
        assert check(average=-1) == invalid
        assert check(device=99) == _lib.RN_ERR_NO_DEVICE
        assert check(device=99, starts=starts_of(0, 50, 137)) == invalid  # (the argument checks come first)
        assert check() == _lib.RN_OK
        assert check(average=1) == _lib.RN_OK
        assert check(Q=1, starts=starts_of(136)) == _lib.RN_OK
    for groups in (0, 17, -1):
        assert call(lib.rn_md_raman_partial_segments, source=incr, steps=199, G=groups) == _lib.RN_ERR_INVALID_ARGUMENT
    assert call(lib.rn_md_raman_partial_segments, source=incr, steps=0) == _lib.RN_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        _md_segments_at_on_device(alpha, 1.0, weights, width, [0, 137], tau, True, 0)


def test_repeatable_and_caches_separate():
    lengths = [2049, 1500]
    e_i, e_s, rotations = _configurations(7, 6)
    weights, _ = polarized_weights(e_i, e_s, rotations)
    width, hop, tau = segment_plan(1500, 513, None, "hann")
    starts, _ = ensemble_segment_starts(lengths, width, hop)
    alpha = MDRamanEnsemble(_runs(lengths, 5), 1.0).polarizability_ts
    incr = PartialMDRamanEnsemble(_increment_runs(lengths, 3, 5), 1.0).increments

    def older_reducers():
        """One call to each of the four older reducers (cache entries of other sizes in between)."""
        _, unpolarized = _md_intensities_on_device(alpha[:1001], 1.0, 0)
        rc, polarized = _polarized(alpha[:1001], weights)
        assert rc == _lib.RN_OK
        _, partial = PartialMDRamanSpectrum(incr[:1000], 1.0).measure_polarized(e_i, e_s, rotations, device=0)
        rc, grid = _segments(alpha[:1001], width, hop, tau, weights, True)
        assert rc == _lib.RN_OK
        return unpolarized, polarized, partial, grid

    before = older_reducers()
    dev_whole = DeviceMDRamanEnsemble(torch.tensor(alpha, device="cuda"), 1.0, lengths)
    dev_partial = DevicePartialMDRamanEnsemble(torch.tensor(incr, device="cuda"), 1.0, lengths)
    for average in (True, False):
        rc, first = _segments_at(alpha, width, starts, tau, weights, average)
        assert rc == _lib.RN_OK
        rc, first_partial = _partial_segments(incr, width, starts, tau, weights, average)
        assert rc == _lib.RN_OK
        for got, want in zip(older_reducers(), before):
            np.testing.assert_array_equal(got, want)
        rc, second = _segments_at(alpha, width, starts, tau, weights, average)
        assert rc == _lib.RN_OK
        np.testing.assert_array_equal(second, first)
        rc, second_partial = _partial_segments(incr, width, starts, tau, weights, average)
        assert rc == _lib.RN_OK
        np.testing.assert_array_equal(second_partial, first_partial)
        # the device-resident entries on the same series give the same bits
        _, third = dev_whole.measure_segments_polarized(e_i, e_s, rotations, segment_steps=513, average=average)
        np.testing.assert_array_equal(third, first)
        _, third = dev_partial.measure_segments_polarized(e_i, e_s, rotations, segment_steps=513, average=average)
        rows, cols = np.triu_indices(3)
        np.testing.assert_array_equal(third[..., rows, cols, :], first_partial)


def test_device_resident_through_trajectory_ensemble():
    from ramannoodle_amd.dynamics import Trajectory, TrajectoryEnsemble
    g = load_golden("triclinic20")
    model = product_model_from_golden(g).eval()
    positions, timestep = g["md/positions"], float(g["md/timestep"])
    cut = len(positions) // 2 + 3
    ensemble = TrajectoryEnsemble([Trajectory(positions[:cut], timestep), Trajectory(positions[cut:], timestep)])
    lengths = [cut, len(positions) - cut]
    assert lengths[0] != lengths[1]
    width = min(lengths) - 2
    e_i, e_s, rotations = _configurations(7, 2)
    on_dev = ensemble.get_raman_spectrum(model, on_device=True)
    on_host = ensemble.get_raman_spectrum(model)
    assert isinstance(on_dev, DeviceMDRamanEnsemble) and type(on_host) is MDRamanEnsemble
    assert on_dev.run_lengths == on_host.run_lengths == lengths
    for left, right in zip(on_dev.segment_starts(width, 1), on_host.segment_starts(width, 1)):
        np.testing.assert_array_equal(left, right)
    partial_dev = ensemble.get_partial_raman_spectrum(model, "species", on_device=True)
    partial_host = ensemble.get_partial_raman_spectrum(model, "species")
    assert isinstance(partial_dev, DevicePartialMDRamanEnsemble) and type(partial_host) is PartialMDRamanEnsemble
    assert partial_dev.run_lengths == partial_host.run_lengths == lengths
    for average in (True, False):
        for kwargs in ({}, CORRECTIONS):
            w_h, i_h = on_host.measure_segments(width, 1, "hamming", average, **kwargs)
            w_d, i_d = on_dev.measure_segments(width, 1, "hamming", average, **kwargs)
            np.testing.assert_array_equal(w_d, w_h)
            _close(i_d, i_h, 1e-10)
            w_h, i_h = partial_host.measure_segments(width, 1, "hamming", average, **kwargs)
            w_d, i_d = partial_dev.measure_segments(width, 1, "hamming", average, **kwargs)
            np.testing.assert_array_equal(w_d, w_h)
            _close(i_d, i_h, 1e-10)
            segments = {"segment_steps": width, "hop": 1, "average": average}
            _, i_h = on_host.measure_segments_polarized(e_i, e_s, rotations, **segments, **kwargs)
            _, i_d = on_dev.measure_segments_polarized(e_i, e_s, rotations, **segments, **kwargs)
            _close(i_d, i_h, 1e-10)
            _, i_h = partial_host.measure_segments_polarized(e_i, e_s, rotations, **segments, **kwargs)
            _, i_d = partial_dev.measure_segments_polarized(e_i, e_s, rotations, **segments, **kwargs)
            _close(i_d, i_h, 1e-10)
    # a single trajectory's device-resident increments have the segment measurements too
    single = Trajectory(positions, timestep).get_partial_raman_spectrum(model, "species", on_device=True)
    assert isinstance(single, DevicePartialMDRamanSpectrum)
    _, i_d = single.measure_segments(width, 4)
    _, i_h = single.measure_segments(width, 4, host=True)
    _close(i_d, i_h, 1e-10)


def test_waits_for_the_producer_stream():
    """The joined series and increments are written on a side stream behind a bounded sleep; the reductions, called
    with that stream current, must see the finished data."""
    lengths = [12_001, 8_000]
    e_i, e_s, rotations = _configurations(7, 8)
    segments = {"segment_steps": 1025, "hop": 256}
    host_whole = MDRamanEnsemble(_runs(lengths, 8), 1.0)
    host_partial = PartialMDRamanEnsemble(_increment_runs(lengths, 2, 8), 1.0)
    _, want_whole = host_whole.measure_segments_polarized(e_i, e_s, rotations, **segments)
    _, want_partial = host_partial.measure_segments_polarized(e_i, e_s, rotations, **segments)
    source_whole = torch.tensor(host_whole.polarizability_ts, device="cuda")
    source_partial = torch.tensor(host_partial.increments, device="cuda")
    target_whole, target_partial = torch.zeros_like(source_whole), torch.zeros_like(source_partial)
    whole = DeviceMDRamanEnsemble(target_whole, 1.0, lengths)
    partial = DevicePartialMDRamanEnsemble(target_partial, 1.0, lengths)

    def measure(spectrum):
        return spectrum.measure_segments_polarized(e_i, e_s, rotations, **segments)[1]

    call_ms = 0.0
    for spectrum in (whole, partial):
        measure(spectrum)  # plans and buffers made outside the window
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        measure(spectrum)
        call_ms = max(call_ms, 1e3 * (time.perf_counter() - t0))
    cycles = _sleep_cycles()
    side = torch.cuda.Stream()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        start.record()
        torch.cuda._sleep(cycles)
        end.record()
        target_whole.copy_(source_whole)
        got_whole = measure(whole)
        torch.cuda._sleep(cycles)
        target_partial.copy_(source_partial)
        got_partial = measure(partial)
    torch.cuda.synchronize()
    slept = start.elapsed_time(end)
    assert slept <= 2000.0, f"the sleep held the stream {slept:.0f} ms"
    assert slept >= 10.0 * call_ms, f"the sleep held the stream {slept:.1f} ms, a call takes {call_ms:.2f} ms"
    _close(got_whole, want_whole, 1e-10)
    _close(got_partial, want_partial, 1e-10)
