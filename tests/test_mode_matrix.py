"""Mode-by-mode interference matrices of MD Raman bands: what needs no GPU.

The numpy path of ``ModeMDRamanSpectrum.measure_interference`` against the band sums of the host pair reducer
(``_md_partial_segments_host``) and of the host mode reducer (``_md_modes_host``), the host code that turns bin weights
into frequency-side weights (``rn_md_raman_mode_matrix_response``) against the brute-force sum, ``band_weights`` and its
errors, the new symbols, and the ensemble classes with ``TrajectoryEnsemble.get_mode_raman_spectrum``."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ramannoodle_amd import _lib
from ramannoodle_amd.dynamics import Phonons, Trajectory, TrajectoryEnsemble
from ramannoodle_amd.spectrum import (DeviceModeMDRamanEnsemble, ModeMDRamanEnsemble, ModeMDRamanSpectrum,
                                      PartialMDRamanEnsemble, _md_modes_host, _md_partial_segments_host,
                                      _measure_weights, band_weights, ensemble_segment_starts, polarized_weights,
                                      segment_plan)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMESTEP = 1.5
ENTRIES = ("rn_md_raman_mode_matrix", "rn_md_raman_mode_matrix_device", "rn_md_raman_mode_matrix_set_profiling",
           "rn_md_raman_mode_matrix_phase_times", "rn_md_raman_mode_matrix_response")


def _increments(steps, channels, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(steps)[:, None, None, None]
    freq = 1 + np.arange(channels * 9).reshape(1, channels, 3, 3) % 23
    incr = 0.05 * rng.normal(size=(steps, channels, 3, 3)) + np.cos(0.07 * t * freq)
    return incr * np.logspace(-1, 1, channels)[None, :, None, None]


def _bands(wavenumbers):
    """Three bands over bins of ``wavenumbers``: a few bins, one bin, all bins."""
    step = wavenumbers[0]
    return np.array([[2.5 * step, 6.5 * step], [wavenumbers[-2] - 0.1 * step, wavenumbers[-2] + 0.1 * step],
                     [0.0, wavenumbers[-1] + step]])


@pytest.mark.parametrize("taper", ["hann", "boxcar"])
@pytest.mark.parametrize("segments", [1, 4])
@pytest.mark.parametrize("channels", [1, 2, 6])
def test_numpy_path_is_the_band_sum_of_the_pair_reducer(channels, segments, taper):
    width, hop = 24, 9  # n = 23, L = 64
    incr = _increments(width - 1 + hop * (segments - 1), channels, seed=channels)
    spectrum = ModeMDRamanSpectrum(incr, TIMESTEP)
    _, _, tau = segment_plan(len(incr) + 1, width, hop, taper)
    starts = spectrum.segment_starts(width, hop)
    assert len(starts) == segments
    rng = np.random.default_rng(2)
    e_i, e_s = rng.normal(size=(3, 3)), rng.normal(size=(3, 3))
    for count in (1, 3):
        weights = _measure_weights() if count == 1 else polarized_weights(e_i, e_s)[0]
        wavenumbers, pairs = _md_partial_segments_host(incr, TIMESTEP, weights, width, starts, tau, True)
        bands = _bands(wavenumbers)
        want = np.einsum("bi,kmni->kbmn", band_weights(wavenumbers, bands), pairs)
        if count == 1:
            edges, got = spectrum.measure_interference(bands, width, hop, taper)
            want = want[0]
        else:
            edges, got = spectrum.measure_interference_polarized(e_i, e_s, bands=bands, segment_steps=width, hop=hop,
                                                                 taper=taper)
        np.testing.assert_array_equal(edges, bands)
        assert got.shape == want.shape == (3, 3, channels, channels)[-want.ndim:]
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        np.testing.assert_array_equal(got, np.swapaxes(got, -1, -2))
    # one configuration squeezes the K axis
    _, one = spectrum.measure_interference_polarized(e_i[0], e_s[0], bands=bands, segment_steps=width, hop=hop)
    assert one.shape == (3, channels, channels)


def _response(n, bin_weights, scale=1.0):
    """``rn_md_raman_mode_matrix_response``: [B][L/2+1] (the zero tail checked and cut)."""
    length = 1 << int(np.ceil(np.log2(2 * n - 1)))
    padded = (length // 2 + 1 + 3) // 4 * 4
    bin_weights = np.ascontiguousarray(bin_weights, dtype=np.float64)
    out = np.full((bin_weights.shape[0], padded), np.nan)
    rc = _lib.load().rn_md_raman_mode_matrix_response(n, C.c_void_p(bin_weights.ctypes.data), bin_weights.shape[0],
                                                      bin_weights.shape[1], scale, C.c_void_p(out.ctypes.data))
    assert rc == 0
    assert np.all(out[:, length // 2 + 1:] == 0.0)
    return length, out[:, :length // 2 + 1]


@pytest.mark.parametrize("n", [23, 32, 1000])
def test_frequency_weights_against_the_brute_force_sum(n):
    """n = 23 and the even n = 32 (L = 64) with every bin weighted, and n = 1000 (L = 2048) with a few, among them the
    first and the last and bins next to a frequency of the padded grid."""
    bins = (n + 1) // 2 - 1
    rng = np.random.default_rng(n)
    if n < 100:
        bin_weights = np.stack([np.where((np.arange(bins) >= 2) & (np.arange(bins) < 5), 1.0, 0.0),
                                rng.normal(size=bins), np.eye(bins)[bins - 1]])
    else:
        bin_weights = np.zeros((3, bins))
        bin_weights[0, [0, 1, 2]] = 1.0
        bin_weights[1, [124, 249, 250, bins - 1]] = rng.normal(size=4)  # bin 124: (bin + 1) / n = 256 / 2048
        bin_weights[2, bins - 1] = 1.0
    length, got = _response(n, bin_weights)
    assert length == (64 if n < 100 else 2048)
    used = np.flatnonzero(np.any(bin_weights != 0.0, axis=0))
    tau = np.arange(n)[None, None, :]
    f = np.arange(length)[None, :, None]
    brute = np.zeros((bins, length))
    brute[used] = np.cos(2 * np.pi * tau * (f / length - (used[:, None, None] + 1) / n)).sum(axis=-1) / length
    u = bin_weights @ brute  # [B][L]
    folded = u[:, :length // 2 + 1].copy()
    folded[:, 1:length // 2] += u[:, :length // 2:-1]
    # both sides carry round-off of a few eps times the n terms of a sum whose largest value is n / L
    assert np.abs(got - folded).max() <= 1e-13 * n * np.abs(bin_weights).sum(axis=1).max()
    _, scaled = _response(n, bin_weights, scale=0.25)
    np.testing.assert_array_equal(scaled, 0.25 * got)
    # the response reproduces the back half: the band sums of a random even power spectrum
    power = rng.uniform(size=length // 2 + 1)
    lags = np.fft.irfft(power, n=length)[:n]
    rows = np.real(np.fft.fft(lags))[1:bins + 1]
    assert np.abs(got @ power - bin_weights @ rows).max() <= 1e-12 * np.abs(rows).max() * np.abs(bin_weights).sum(1).max()
    lib = _lib.load()
    out = np.zeros((3, length // 2 + 4))
    for bad in ((1, bins), (n, bins + 1)):
        assert lib.rn_md_raman_mode_matrix_response(bad[0], C.c_void_p(bin_weights.ctypes.data), 3, bad[1], 1.0,
                                                    C.c_void_p(out.ctypes.data)) == _lib.RN_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("corrected", [False, True])
def test_entries_sum_to_the_band_and_the_diagonal_is_the_self_spectra(corrected):
    channels, width, hop = 6, 24, 9
    incr = _increments(60, channels, seed=3)
    spectrum = ModeMDRamanSpectrum(incr, TIMESTEP)
    keywords = dict(laser_correction=corrected, bose_einstein_correction=corrected, temperature=250)
    wavenumbers, rows = spectrum.measure_segments(width, hop, **keywords)  # the rows of _md_modes_host, corrected
    _, _, tau = segment_plan(len(incr) + 1, width, hop, "hann")
    _, raw = _md_modes_host(incr, TIMESTEP, _measure_weights(), width, spectrum.segment_starts(width, hop), tau, True)
    bands = _bands(wavenumbers)
    indicator = band_weights(wavenumbers, bands)
    assert set(np.unique(indicator)) == {0.0, 1.0}
    np.testing.assert_array_equal(indicator.sum(axis=1), [4, 1, len(wavenumbers)])
    if not corrected:
        np.testing.assert_array_equal(rows, raw[0])
    _, got = spectrum.measure_interference(bands, width, hop, **keywords)
    band_sums = rows @ indicator.T  # [C+1][B]
    scale = np.abs(got).max(axis=(1, 2))
    assert np.all(np.abs(got.sum(axis=(1, 2)) - band_sums[-1]) <= 1e-12 * channels ** 2 * scale)
    assert np.all(np.abs(np.diagonal(got, axis1=1, axis2=2) - band_sums[:-1].T) <= 1e-12 * scale[:, None])
    # the whole run as one boxcar segment: measure()
    _, whole = spectrum.measure(**keywords)
    wavenumbers, _ = spectrum.measure()
    bands = _bands(wavenumbers)
    _, got = spectrum.measure_interference(bands, **keywords)
    want = whole[-1] @ band_weights(wavenumbers, bands).T
    assert np.all(np.abs(got.sum(axis=(1, 2)) - want) <= 1e-12 * channels ** 2 * np.abs(got).max(axis=(1, 2)))


def test_band_weights_and_their_errors():
    wavenumbers = 10.0 * np.arange(1, 9)
    weights = band_weights(wavenumbers, [[10.0, 30.0], [75.0, 1e4]])
    np.testing.assert_array_equal(weights, [[1, 1, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 1]])  # [lo, hi)
    assert weights.dtype == np.float64 and weights.flags.c_contiguous
    corrected = band_weights(wavenumbers, [[10.0, 30.0]], laser_correction=True, bose_einstein_correction=True)
    assert np.all(corrected[0, :2] > 0) and np.all(corrected[0, 2:] == 0) and corrected[0, 0] != corrected[0, 1]
    with pytest.raises(ValueError, match=r"bands\[1\].*holds no bin.*10 cm"):
        band_weights(wavenumbers, [[10.0, 30.0], [31.0, 39.0]])
    with pytest.raises(ValueError, match="holds no bin"):
        band_weights(wavenumbers, [[0.0, 10.0]])  # half-open: the bin at 10 is outside
    for bad in ([[30.0, 30.0]], [[40.0, 20.0]], [[np.nan, 20.0]], [[10.0, np.inf]], [10.0, 30.0], [[10.0, 20.0, 30.0]],
                np.zeros((0, 2)), [[[10.0, 30.0]]], "band"):
        with pytest.raises(ValueError):
            band_weights(wavenumbers, bad)
    spectrum = ModeMDRamanSpectrum(_increments(40, 2, seed=1), TIMESTEP)
    for bad in ([[1e6, 2e6]], [[500.0, 100.0]], [[np.nan, 1.0]], [100.0, 500.0]):
        with pytest.raises(ValueError):
            spectrum.measure_interference(bad)
        with pytest.raises(ValueError):
            spectrum.measure_interference_polarized([1.0, 0, 0], [1.0, 0, 0], bands=bad, segment_steps=24)
    with pytest.raises(NotImplementedError):
        spectrum.measure_interference([[0.0, 1e5]], orientation=np.eye(3))


def test_new_symbols_are_declared_listed_and_exported():
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True,
                        text=True).stdout
    exported = set(re.findall(r" T (\w+)", nm))
    with open(os.path.join(ROOT, "include", "rn_potgnn.h"), encoding="utf-8") as file:
        text = file.read()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), f"{name} is not declared in rn_potgnn.h"
        assert name in _lib.SIGNATURES, name
        assert name in exported, name
    table = _lib.SIGNATURES
    host, device = table["rn_md_raman_mode_matrix"], table["rn_md_raman_mode_matrix_device"]
    assert device[0] == host[0] and device[1] == host[1] + [C.c_void_p]
    # rn_md_raman_modes with (bin_weights, B) where it has `average`
    modes = table["rn_md_raman_modes"][1]
    assert host[1] == modes[:9] + [C.c_void_p, C.c_int64] + modes[10:]


def _runs(lengths, channels, seed):
    return [_increments(length - 1, channels, seed + run) for run, length in enumerate(lengths)]


def test_ensemble_segments_stay_inside_their_runs():
    lengths = [40, 31, 55]
    ensemble = ModeMDRamanEnsemble(_runs(lengths, 3, seed=20), TIMESTEP)
    assert ensemble.run_lengths == lengths and ensemble.num_channels == 3
    assert ensemble.increments.shape == (sum(lengths) - 1, 3, 3, 3)
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    for offset in offsets[1:]:
        assert np.all(ensemble.increments[offset - 1] == 0.0)  # the row between two runs
    run_index, within = ensemble.segment_starts(24, 9)
    starts, index = ensemble_segment_starts(lengths, 24, 9)
    np.testing.assert_array_equal(run_index, index)
    np.testing.assert_array_equal(within + offsets[run_index], starts)
    assert np.all(within >= 0) and np.all(within + 24 <= np.asarray(lengths)[run_index])
    assert np.all(np.bincount(run_index) == [(length - 24) // 9 + 1 for length in lengths])
    _, rows = ensemble.measure_segments(24, 9, average=False)
    assert rows.shape[0] == len(starts)
    # row q is the segment of its own run
    for q in (0, len(starts) - 1):
        run = ModeMDRamanSpectrum(_runs(lengths, 3, seed=20)[run_index[q]], TIMESTEP)
        _, own = run.measure_segments(24, 9, average=False)
        np.testing.assert_allclose(rows[q], own[within[q] // 9], rtol=0, atol=1e-12 * np.abs(own).max())
    with pytest.raises(ValueError):
        ensemble.measure()  # runs of several lengths have no common whole spectrum
    with pytest.raises(ValueError):
        ensemble.measure_segments(32)  # longer than the shortest run
    with pytest.raises(ValueError):
        ModeMDRamanEnsemble([], TIMESTEP)
    with pytest.raises(ValueError):
        ModeMDRamanEnsemble([_increments(20, 3, 0), _increments(20, 4, 0)], TIMESTEP)
    with pytest.raises(ValueError, match="CUDA tensors"):
        DeviceModeMDRamanEnsemble(_runs(lengths, 3, seed=20), TIMESTEP)  # not CUDA tensors
    chosen = ensemble.select([2, 0])
    assert isinstance(chosen, PartialMDRamanEnsemble) and chosen.run_lengths == lengths
    np.testing.assert_array_equal(chosen.increments[:, 0], ensemble.increments[:, 2])


def test_two_equal_runs_give_the_mean_of_their_power_means():
    lengths = [46, 46]
    runs = _runs(lengths, 4, seed=30)
    ensemble = ModeMDRamanEnsemble(runs, TIMESTEP)
    single = [ModeMDRamanSpectrum(run, TIMESTEP) for run in runs]
    rng = np.random.default_rng(3)
    e_i, e_s = rng.normal(size=(2, 3)), rng.normal(size=(2, 3))

    def same(got, want):
        assert got[1].shape == want[0][1].shape
        mean = 0.5 * (want[0][1] + want[1][1])
        assert np.abs(got[1] - mean).max() <= 1e-12 * np.abs(mean).max()

    same(ensemble.measure(), [s.measure() for s in single])
    same(ensemble.measure_polarized(e_i, e_s), [s.measure_polarized(e_i, e_s) for s in single])
    same(ensemble.measure_segments(24, 11), [s.measure_segments(24, 11) for s in single])
    same(ensemble.measure_segments_polarized(e_i, e_s, segment_steps=24, hop=11),
         [s.measure_segments_polarized(e_i, e_s, segment_steps=24, hop=11) for s in single])
    wavenumbers, _ = ensemble.measure_segments(24, 11)
    bands = _bands(wavenumbers)
    same(ensemble.measure_interference(bands, 24, 11), [s.measure_interference(bands, 24, 11) for s in single])
    same(ensemble.measure_interference_polarized(e_i, e_s, bands=bands, segment_steps=24, hop=11),
         [s.measure_interference_polarized(e_i, e_s, bands=bands, segment_steps=24, hop=11) for s in single])
    bands = _bands(ensemble.measure()[0])
    same(ensemble.measure_interference(bands), [s.measure_interference(bands) for s in single])


class _NoJacobian:
    num_atoms = 4
    device_index = 0


def test_trajectory_ensemble_front_end_without_a_gpu():
    lattice = np.array([[4.1, 0.3, -0.2], [0.5, 5.2, 0.4], [-0.3, 0.6, 6.3]])
    rng = np.random.default_rng(0)
    fractional = np.linalg.qr(rng.normal(size=(12, 12)))[0].T.reshape(12, 4, 3) @ np.linalg.inv(lattice)
    phonons = Phonons(np.zeros((4, 3)), np.arange(12.0), fractional)
    ensemble = TrajectoryEnsemble([Trajectory(rng.uniform(size=(6, 4, 3)), 1.0) for _ in range(2)])
    with pytest.raises(TypeError):
        ensemble.get_mode_raman_spectrum(_NoJacobian(), phonons, lattice)
    with pytest.raises(TypeError):
        ensemble.get_mode_raman_spectrum(_NoJacobian(), phonons, lattice, on_device=True)
