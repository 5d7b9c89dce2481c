"""Segment-averaged and time-resolved MD Raman spectra reduced on the GPU (``rn_md_raman_segments`` and its ``_device``
form) against the host path of ``measure_segments_polarized``: segment lengths, hops, tapers and configuration counts, a
single segment against ``rn_md_raman_polarized``, segment blocks and row sub-blocks under a small workspace, the argument
checks, determinism, separate plan caches, the device-resident path and ordering behind work still queued on the caller's
stream.  Every GPU step is small and bounded."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from ramannoodle_amd import _lib
from ramannoodle_amd.spectrum import (DeviceMDRamanSpectrum, MDRamanSpectrum, _md_intensities_on_device,
                                      _md_segments_on_device, polarized_weights, segment_plan)
from tests.conftest import load_golden
from tests.helpers import product_model_from_golden
from tests.test_polarized_spectra_gpu import (CORRECTIONS, _close, _configurations, _polarized, _series,
                                              _sleep_cycles)

pytestmark = pytest.mark.gpu


def _segments(alpha, width, hop, tau, weights, average, limit=0, device=0, bins=None):
    """Raw ``rn_md_raman_segments``: (status, intensities)."""
    alpha = np.ascontiguousarray(alpha, dtype=np.float64)
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    steps, count = alpha.shape[0], weights.shape[0]
    if bins is None:
        bins = width // 2 - 1  # ceil((W - 1) / 2) - 1
    shape = (count, bins) if average else ((steps - width) // hop + 1, count, bins)
    out = np.full(shape, np.nan)
    rc = _lib.load().rn_md_raman_segments(C.c_void_p(alpha.ctypes.data), steps, width, hop, C.c_void_p(tau.ctypes.data),
                                          C.c_void_p(weights.ctypes.data), count, int(average), device, limit,
                                          C.c_void_p(out.ctypes.data), bins)
    return rc, out


# (S, W, H, K, taper): one segment; even n at 75 % overlap; W = 3; no overlap, odd n; 75 % overlap and many
# configurations; one configuration; a long series
@pytest.mark.parametrize("steps,width,hop,k,taper", [
    (64, 64, 1, 7, "hann"), (257, 65, 16, 1, "blackman"), (50, 3, 1, 7, "hamming"), (1001, 100, 100, 720, "hann"),
    (2000, 256, 64, 720, "boxcar"), (4096, 1025, 512, 1, "hann"), (200_001, 4097, 2048, 7, "hann")])
def test_device_matches_host(steps, width, hop, k, taper):
    alpha = _series(steps, steps)
    e_i, e_s, rotations = _configurations(k, k)
    spectrum = MDRamanSpectrum(alpha, 1.5)
    segments = {"segment_steps": width, "hop": hop, "taper": taper}
    for average in (True, False):
        for kwargs in ({}, CORRECTIONS):
            w_host, i_host = spectrum.measure_segments_polarized(e_i, e_s, rotations, average=average, **segments,
                                                                 **kwargs)
            w_dev, i_dev = spectrum.measure_segments_polarized(e_i, e_s, rotations, average=average, device=0,
                                                               **segments, **kwargs)
            np.testing.assert_array_equal(w_dev, w_host)
            _close(i_dev, i_host, 1e-10)
        _, i_host = spectrum.measure_segments(average=average, **segments)
        _, i_dev = spectrum.measure_segments(average=average, device=0, **segments)
        _close(i_dev, i_host, 1e-10)


@pytest.mark.parametrize("steps,width,hop", [(1500, 1001, 1000), (64, 64, 1), (4097, 4097, 2048)])
def test_single_boxcar_segment_is_the_polarized_entry(steps, width, hop):
    alpha = _series(steps, 11)
    e_i, e_s, rotations = _configurations(7, 11)
    weights, _ = polarized_weights(e_i, e_s, rotations)
    rc, want = _polarized(alpha[:width], weights)
    assert rc == _lib.RN_OK
    for average in (True, False):
        rc, got = _segments(alpha, width, hop, np.ones(width - 1), weights, average)
        assert rc == _lib.RN_OK
        _close(got.reshape(want.shape), want, 1e-10)


def test_workspace_limit_blocks_and_out_of_memory():
    alpha = _series(1001, 9)
    e_i, e_s, rotations = _configurations(7, 4)
    weights, _ = polarized_weights(e_i, e_s, rotations)
    width, hop, tau = segment_plan(1001, 129, 32, "hann")
    # a segment's components take 6 * 256 complex doubles (24 576 B) and a row 256 complex doubles and 63 bins (4 600 B):
    # 150 000 B hold three of the 28 segments and some of their 21 rows, 45 000 B one segment and three of the 7
    # configurations (the averaged call then transforms the segments once per block of configurations)
    for average in (True, False):
        rc, full = _segments(alpha, width, hop, tau, weights, average)
        assert rc == _lib.RN_OK
        for limit in (150_000, 45_000):
            rc, small = _segments(alpha, width, hop, tau, weights, average, limit=limit)
            assert rc == _lib.RN_OK, limit
            _close(small, full, 1e-13)
        rc, _ = _segments(alpha, width, hop, tau, weights, average, limit=1000)
        assert rc == _lib.RN_ERR_OUT_OF_MEMORY
        with pytest.raises(MemoryError):
            _md_segments_on_device(alpha, 1.0, weights, width, hop, tau, average, 0, workspace_limit=1000)


def test_argument_checks():
    alpha = _series(200, 1)
    width, hop, bins = 64, 32, 31  # ceil(63 / 2) - 1
    tau = np.ones(width - 1)
    weights = np.ones((2, 21))
    out = np.empty((5, 2, bins + 1))  # room for a wrong num_bins that slips through
    lib = _lib.load()
    p = C.c_void_p
    good = [p(alpha.ctypes.data), 200, width, hop, p(tau.ctypes.data), p(weights.ctypes.data), 2, 0, 0, 0,
            p(out.ctypes.data), bins]

    def call(**changes):
        names = ("alpha", "S", "segment_steps", "hop", "taper", "weights", "K", "average", "device",
                 "workspace_limit", "intensities", "num_bins")
        args = list(good)
        for name, value in changes.items():
            args[names.index(name)] = value
        return lib.rn_md_raman_segments(*args)

    assert call(alpha=None) == _lib.RN_ERR_INVALID_ARGUMENT
    assert call(taper=None) == _lib.RN_ERR_INVALID_ARGUMENT
    assert call(weights=None) == _lib.RN_ERR_INVALID_ARGUMENT
    assert call(intensities=None) == _lib.RN_ERR_INVALID_ARGUMENT
    assert call(K=0) == _lib.RN_ERR_INVALID_ARGUMENT
    assert call(segment_steps=2, num_bins=0) == _lib.RN_ERR_INVALID_ARGUMENT
    assert call(segment_steps=201, num_bins=99) == _lib.RN_ERR_INVALID_ARGUMENT
    assert call(hop=0) == _lib.RN_ERR_INVALID_ARGUMENT
    assert call(num_bins=bins + 1) == _lib.RN_ERR_INVALID_ARGUMENT
    assert call(num_bins=bins - 1) == _lib.RN_ERR_INVALID_ARGUMENT
    assert call(average=2) == _lib.RN_ERR_INVALID_ARGUMENT
    assert call(average=-1) == _lib.RN_ERR_INVALID_ARGUMENT
    assert call(device=99) == _lib.RN_ERR_NO_DEVICE
    assert call(device=99, average=2) == _lib.RN_ERR_INVALID_ARGUMENT  # (the argument checks come first)
    assert call() == _lib.RN_OK
    assert call(average=1) == _lib.RN_OK


def test_repeatable_and_caches_separate():
    steps = 4097
    alpha = _series(steps, 5)
    e_i, e_s, rotations = _configurations(720, 6)
    weights, _ = polarized_weights(e_i, e_s, rotations)
    width, hop, tau = segment_plan(steps, 513, None, "hann")
    _, unpolarized_before = _md_intensities_on_device(alpha, 1.0, 0)
    rc, polarized_before = _polarized(alpha, weights)
    assert rc == _lib.RN_OK
    dev = DeviceMDRamanSpectrum(torch.tensor(alpha, device="cuda"), 1.0)
    for average in (True, False):
        rc, first = _segments(alpha, width, hop, tau, weights, average)
        assert rc == _lib.RN_OK
        rc, second = _segments(alpha, width, hop, tau, weights, average)
        assert rc == _lib.RN_OK
        np.testing.assert_array_equal(first, second)
        # the device-resident entry on the same series gives the same bits
        _, third = dev.measure_segments_polarized(e_i, e_s, rotations, segment_steps=513, average=average)
        np.testing.assert_array_equal(third, first)
    _, unpolarized_after = _md_intensities_on_device(alpha, 1.0, 0)
    np.testing.assert_array_equal(unpolarized_before, unpolarized_after)
    rc, polarized_after = _polarized(alpha, weights)
    assert rc == _lib.RN_OK
    np.testing.assert_array_equal(polarized_before, polarized_after)


def test_device_resident_through_trajectory():
    from ramannoodle_amd.dynamics import Trajectory
    g = load_golden("triclinic20")
    model = product_model_from_golden(g)
    traj = Trajectory(g["md/positions"], float(g["md/timestep"]))
    on_dev = traj.get_raman_spectrum(model, on_device=True)
    assert isinstance(on_dev, DeviceMDRamanSpectrum)
    on_host = MDRamanSpectrum(on_dev.polarizability_ts, float(g["md/timestep"]))
    np.testing.assert_array_equal(on_dev.segment_starts(24, 8), on_host.segment_starts(24, 8))
    e_i, e_s, rotations = _configurations(7, 2)
    for average in (True, False):
        for kwargs in ({}, CORRECTIONS):
            w_h, i_h = on_host.measure_segments(24, 8, "hamming", average, **kwargs)
            w_d, i_d = on_dev.measure_segments(24, 8, "hamming", average, **kwargs)
            np.testing.assert_array_equal(w_d, w_h)
            _close(i_d, i_h, 1e-10)
            _, i_x = on_dev.measure_segments(24, 8, "hamming", average, host=True, **kwargs)
            _close(i_x, i_h, 1e-14)
            for orientation in (rotations, "polycrystalline"):
                segments = {"segment_steps": 24, "hop": 8, "average": average}
                w_h, i_h = on_host.measure_segments_polarized(e_i, e_s, orientation, **segments, **kwargs)
                w_d, i_d = on_dev.measure_segments_polarized(e_i, e_s, orientation, **segments, **kwargs)
                np.testing.assert_array_equal(w_d, w_h)
                _close(i_d, i_h, 1e-10)
                _, i_x = on_dev.measure_segments_polarized(e_i, e_s, orientation, host=True, **segments, **kwargs)
                _close(i_x, i_h, 1e-14)
    # the reference's spectrum from the device-reduced single boxcar segment
    spectrum = DeviceMDRamanSpectrum(torch.tensor(g["md/alpha_ts"], device="cuda"), float(g["md/timestep"]))
    _, raw = spectrum.measure_segments(48, taper="boxcar")
    _close(raw, g["md/int_raw"], 1e-9)


def test_waits_for_the_producer_stream():
    """alpha(t) is written on a side stream behind a bounded sleep; the reduction, called with that stream
    current, must see the finished series."""
    steps = 20_001
    alpha = _series(steps, 8)
    e_i, e_s, rotations = _configurations(7, 8)
    segments = {"segment_steps": 1025, "hop": 256}
    _, want = MDRamanSpectrum(alpha, 1.0).measure_segments_polarized(e_i, e_s, rotations, **segments)
    source = torch.tensor(alpha, device="cuda")
    target = torch.zeros_like(source)
    spectrum = DeviceMDRamanSpectrum(target, 1.0)
    spectrum.measure_segments_polarized(e_i, e_s, rotations, **segments)  # plans and buffers made outside the window
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    spectrum.measure_segments_polarized(e_i, e_s, rotations, **segments)
    call_ms = 1e3 * (time.perf_counter() - t0)
    cycles = _sleep_cycles()
    side = torch.cuda.Stream()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        start.record()
        torch.cuda._sleep(cycles)
        end.record()
        target.copy_(source)
        _, got = spectrum.measure_segments_polarized(e_i, e_s, rotations, **segments)
    torch.cuda.synchronize()
    slept = start.elapsed_time(end)
    assert slept <= 2000.0, f"the sleep held the stream {slept:.0f} ms"
    assert slept >= 10.0 * call_ms, f"the sleep held the stream {slept:.1f} ms, a call takes {call_ms:.2f} ms"
    _close(got, want, 1e-10)
