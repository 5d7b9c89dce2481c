"""Replicate spectra and error bars of segment-averaged MD Raman spectra: what needs no GPU.

``replicate_weights`` and ``segment_blocks``, the host path of ``measure_segment_replicates`` against the combination of
the rows of ``measure_segments_polarized(average=False)``, the closed forms of the three standard errors,
``lineshape.replicate_errors`` on hand-made fits, the classes that have no replicates, and the new symbols."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ramannoodle_amd import _lib, replicates
from ramannoodle_amd.lineshape import LorentzianFits, replicate_errors
from ramannoodle_amd.replicates import (SpectrumEstimate, measure_segment_replicates,
                                        measure_segment_replicates_polarized, measure_segments_error,
                                        replicate_standard_error, replicate_weights, segment_blocks)
from ramannoodle_amd.spectrum import (MDRamanEnsemble, MDRamanSpectrum, ModeMDRamanSpectrum,
                                      ModeVibrationalDensityOfStates, PartialMDRamanEnsemble, PartialMDRamanSpectrum,
                                      VibrationalDensityOfStates, ensemble_segment_starts)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMESTEP = 1.5
CORRECTIONS = {"laser_correction": True, "laser_wavelength": 532, "bose_einstein_correction": True, "temperature": 250}
ENTRIES = ("rn_md_raman_segment_replicates", "rn_md_raman_segment_replicates_device",
           "rn_md_raman_segment_replicates_set_profiling", "rn_md_raman_segment_replicates_phase_times")
UNEQUAL = np.array([0, 0, 0, 1, 2, 2, 2, 2, 1, 0])  # block sizes 4, 2, 4, not contiguous


def _series(steps, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(steps)[:, None, None]
    alpha = rng.normal(size=(steps, 3, 3)) * 0.1 + np.sin(0.05 * t * (1 + np.arange(9).reshape(3, 3)))
    return alpha + np.swapaxes(alpha, 1, 2)


def _ensemble(lengths=(50, 81, 64)):
    return MDRamanEnsemble([_series(steps, 11 + steps) for steps in lengths], TIMESTEP)


# ----------------------------------------------------------------------------- replicate_weights
@pytest.mark.parametrize("method", ["bootstrap", "jackknife", "blocks"])
def test_rows_sum_to_one_with_unequal_blocks(method):
    weights = replicate_weights(UNEQUAL, method, replicates=50, seed=3)
    assert weights.shape == (50 if method == "bootstrap" else 3, len(UNEQUAL))
    assert weights.flags.c_contiguous and weights.dtype == np.float64
    assert np.abs(weights.sum(axis=1) - 1.0).max() <= 1e-15


def test_bootstrap_draws_whole_blocks_from_a_seed():
    first = replicate_weights(UNEQUAL, "bootstrap", replicates=40, seed=5)
    np.testing.assert_array_equal(first, replicate_weights(UNEQUAL, "bootstrap", replicates=40, seed=5))
    assert not np.array_equal(first, replicate_weights(UNEQUAL, "bootstrap", replicates=40, seed=6))
    counts = np.random.default_rng(5).multinomial(3, np.full(3, 1.0 / 3.0), size=40)
    assert np.all(counts.sum(axis=1) == 3)
    sizes = np.bincount(UNEQUAL)
    np.testing.assert_array_equal(first, counts[:, UNEQUAL] / (counts @ sizes)[:, None])
    # the counts of a row, recovered from its weights, sum to G
    recovered = np.stack([first[:, np.flatnonzero(UNEQUAL == block)[0]] for block in range(3)], axis=1)
    recovered *= (counts @ sizes)[:, None]
    assert np.abs(recovered.sum(axis=1) - 3).max() <= 1e-12


def test_jackknife_and_block_rows():
    jackknife = replicate_weights(UNEQUAL, "jackknife")
    blocks = replicate_weights(UNEQUAL, "blocks")
    sizes = np.bincount(UNEQUAL)
    for r in range(3):
        inside = UNEQUAL == r
        assert np.all(jackknife[r, inside] == 0.0) and np.all(jackknife[r, ~inside] == 1.0 / (10 - sizes[r]))
        assert np.all(blocks[r, ~inside] == 0.0) and np.all(blocks[r, inside] == 1.0 / sizes[r])
    # one block: its mean is defined, a delete-one mean is not
    np.testing.assert_array_equal(replicate_weights(np.zeros(4, dtype=int), "blocks"), np.full((1, 4), 0.25))
    np.testing.assert_array_equal(replicate_weights(np.zeros(4, dtype=int), "bootstrap", 2), np.full((2, 4), 0.25))


def test_replicate_weights_errors():
    with pytest.raises(ValueError, match="at least two blocks"):
        replicate_weights(np.zeros(4, dtype=int), "jackknife")
    with pytest.raises(ValueError, match="unused"):
        replicate_weights([0, 2, 2])
    with pytest.raises(ValueError, match="negative"):
        replicate_weights([0, -1, 1])
    with pytest.raises(ValueError, match="wrong shape"):
        replicate_weights(np.zeros((2, 2), dtype=int))
    with pytest.raises(ValueError, match="wrong shape"):
        replicate_weights(np.zeros(0, dtype=int))
    with pytest.raises(TypeError):
        replicate_weights([0.0, 1.0])
    with pytest.raises(ValueError, match="unknown method"):
        replicate_weights([0, 1], "subsample")
    for bad in (0, -3):
        with pytest.raises(ValueError, match="invalid replicates"):
            replicate_weights([0, 1], "bootstrap", replicates=bad)
    with pytest.raises(TypeError):
        replicate_weights([0, 1], "bootstrap", replicates=2.5)


# ----------------------------------------------------------------------------- segment_blocks
def test_segment_blocks():
    lengths = [50, 81, 64]
    ensemble = _ensemble(lengths)
    want = ensemble_segment_starts(lengths, 17, 5)[1]
    np.testing.assert_array_equal(segment_blocks(ensemble, 17, 5), want)
    count = len(want)
    single = MDRamanSpectrum(_series(81, 2), TIMESTEP)
    np.testing.assert_array_equal(segment_blocks(single, 17, 5), np.arange(13))  # one block per segment
    one_run = MDRamanEnsemble([_series(81, 2)], TIMESTEP)
    np.testing.assert_array_equal(segment_blocks(one_run, 17, 5), np.arange(13))
    for groups in (1, 4, 7, count):
        labels = segment_blocks(ensemble, 17, 5, blocks=groups)
        assert labels.shape == (count,) and np.all(np.diff(labels) >= 0)
        sizes = np.bincount(labels)
        assert len(sizes) == groups and sizes.max() - sizes.min() <= 1
    given = np.arange(count) % 3
    np.testing.assert_array_equal(segment_blocks(ensemble, 17, 5, blocks=given), given)
    for bad in (0, count + 1):
        with pytest.raises(ValueError, match="invalid blocks"):
            segment_blocks(ensemble, 17, 5, blocks=bad)
    with pytest.raises(ValueError, match="wrong shape"):
        segment_blocks(ensemble, 17, 5, blocks=given[:-1])
    with pytest.raises(ValueError, match="unused"):
        segment_blocks(ensemble, 17, 5, blocks=2 * given)


# ----------------------------------------------------------------------------- the host path
@pytest.mark.parametrize("corrections", [{}, CORRECTIONS])
@pytest.mark.parametrize("k", [1, 7])
def test_host_replicates_are_combinations_of_the_segment_rows(k, corrections):
    ensemble = _ensemble()
    rng = np.random.default_rng(k)
    e_i, e_s = rng.normal(size=(k, 3)), rng.normal(size=(k, 3))
    segments = {"segment_steps": 17, "hop": 5, "taper": "hann"}
    w_rows, rows = ensemble.measure_segments_polarized(e_i, e_s, average=False, **segments, **corrections)
    count = rows.shape[0]
    assert rows.shape[1] == k and count == 30
    labels = segment_blocks(ensemble, 17, 5)
    tables = [replicate_weights(labels, "bootstrap", 9, 4), replicate_weights(labels, "jackknife"),
              replicate_weights(labels, "blocks"), rng.normal(size=(5, count)), np.full((1, count), 1.0 / count)]
    keywords = [{"replicates": 9, "seed": 4}, {"method": "jackknife"}, {"method": "blocks"},
                {"replicate_weights": tables[3], "method": "jackknife", "blocks": 2},  # (the table overrides the rest)
                {"replicate_weights": tables[4]}]
    for table, extra in zip(tables, keywords):
        w, got = measure_segment_replicates_polarized(ensemble, e_i, e_s, **segments, **extra, **corrections)
        np.testing.assert_array_equal(w, w_rows)
        want = np.einsum("rq,qkb->rkb", table, rows)
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # the uniform row is the mean
    _, mean = ensemble.measure_segments_polarized(e_i, e_s, average=True, **segments, **corrections)
    assert np.abs(got[0] - mean).max() <= 1e-12 * np.abs(mean).max()
    # the powder average: rows (R, bins)
    _, rows = ensemble.measure_segments(17, 5, average=False, **corrections)
    _, got = measure_segment_replicates(ensemble, 17, 5, replicate_weights=tables[3], **corrections)
    want = tables[3] @ rows
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # a single run goes through the same table
    single = MDRamanSpectrum(_series(81, 2), TIMESTEP)
    _, rows = single.measure_segments(17, 5, average=False)
    _, got = measure_segment_replicates(single, 17, 5, method="jackknife")
    want = replicate_weights(np.arange(13), "jackknife") @ rows
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_replicate_weights_argument_is_checked():
    ensemble = _ensemble()
    for bad in (np.ones((3, 29)), np.ones(30), np.ones((0, 30))):
        with pytest.raises(ValueError, match="wrong shape"):
            measure_segment_replicates(ensemble, 17, 5, replicate_weights=bad)
    with pytest.raises(ValueError, match="not finite"):
        measure_segment_replicates(ensemble, 17, 5, replicate_weights=np.full((2, 30), np.nan))
    with pytest.raises(TypeError):
        measure_segment_replicates(ensemble, 17, 5, replicate_weights=np.full((2, 30), "a"))
    with pytest.raises(NotImplementedError):
        measure_segment_replicates(ensemble, 17, 5, orientation=np.eye(3))


# ----------------------------------------------------------------------------- closed forms
class _Stub(MDRamanSpectrum):
    """A spectrum whose Q segment rows are given: the replicates are their combinations (``given_rows`` puts them in
    the place of the reduction), the mean their mean."""

    def __init__(self, rows):
        super().__init__(_series(4 * len(rows) + 4, 1), TIMESTEP)  # Q segments of 8 frames, hop 4
        self.rows = rows
        self.axis = np.arange(1.0, rows.shape[1] + 1.0)

    def _segments(self, weights, segment_steps, hop, taper, average, device):
        assert average
        return self.axis, self.rows.mean(axis=0)[None, :]


@pytest.fixture
def given_rows(monkeypatch):
    def rows_of_the_stub(spectrum, weights, table, replicate_weights, device):
        assert replicate_weights.shape[1] == len(table[2]) == len(spectrum.rows)
        return spectrum.axis, (replicate_weights @ spectrum.rows)[:, None, :]

    monkeypatch.setattr(replicates, "_replicate_rows", rows_of_the_stub)


def test_jackknife_and_blocks_are_the_standard_error_of_the_block_means(given_rows):
    rng = np.random.default_rng(8)
    rows = rng.normal(size=(24, 11)) ** 2 + np.arange(24)[:, None]
    stub = _Stub(rows)
    for groups in (2, 6, 24):
        means = rows.reshape(groups, 24 // groups, 11).mean(axis=1)
        want = means.std(axis=0, ddof=1) / np.sqrt(groups)
        for method in ("jackknife", "blocks"):
            estimate = measure_segments_error(stub, 8, 4, blocks=groups, method=method, level=0.9)
            assert isinstance(estimate, SpectrumEstimate) and estimate.method == method
            assert estimate.replicates.shape == (groups, 11)
            np.testing.assert_array_equal(estimate.wavenumbers, stub.axis)
            np.testing.assert_array_equal(estimate.mean, rows.mean(axis=0))
            assert np.abs(estimate.standard_error - want).max() <= 1e-13 * np.abs(want).max(), (groups, method)
            reach = 1.6448536269514722 * estimate.standard_error  # the 0.95 quantile of the standard normal
            np.testing.assert_allclose(estimate.upper - estimate.mean, reach, rtol=1e-12)
            np.testing.assert_allclose(estimate.mean - estimate.lower, reach, rtol=1e-12)
    with pytest.raises(ValueError, match="equal numbers"):
        measure_segments_error(stub, 8, 4, blocks=5, method="blocks")  # 24 segments in five blocks
    measure_segments_error(stub, 8, 4, blocks=5, method="jackknife")   # (the jackknife takes them)
    with pytest.raises(ValueError, match="at least two"):
        measure_segments_error(stub, 8, 4, blocks=1, method="blocks")
    with pytest.raises(ValueError, match="invalid level"):
        measure_segments_error(stub, 8, 4, level=1.0)
    with pytest.raises(ValueError, match="unknown method"):
        measure_segments_error(stub, 8, 4, method="subsample")


def test_bootstrap_error_and_band(given_rows):
    rng = np.random.default_rng(9)
    rows = rng.normal(size=(24, 5)) + 10.0
    stub = _Stub(rows)
    estimate = measure_segments_error(stub, 8, 4, blocks=6, replicates=300, seed=2, level=0.8)
    table = replicate_weights(np.repeat(np.arange(6), 4), "bootstrap", 300, 2)
    np.testing.assert_array_equal(estimate.replicates, table @ rows)
    np.testing.assert_allclose(estimate.standard_error, (table @ rows).std(axis=0, ddof=1), rtol=1e-13)
    np.testing.assert_allclose(estimate.lower, np.percentile(table @ rows, 10.0, axis=0), rtol=1e-13)
    np.testing.assert_allclose(estimate.upper, np.percentile(table @ rows, 90.0, axis=0), rtol=1e-13)
    assert np.all(estimate.lower < estimate.mean) and np.all(estimate.mean < estimate.upper)
    # about the standard error of the mean of six independent block means
    naive = rows.reshape(6, 4, 5).mean(axis=1).std(axis=0, ddof=1) / np.sqrt(6)
    assert np.all(estimate.standard_error > 0.5 * naive) and np.all(estimate.standard_error < 1.5 * naive)


def test_error_bars_of_a_real_series_on_the_host():
    ensemble = _ensemble()
    estimate = measure_segments_error(ensemble, 17, 5, method="jackknife", **CORRECTIONS)
    w, mean = ensemble.measure_segments(17, 5, **CORRECTIONS)
    np.testing.assert_array_equal(estimate.wavenumbers, w)
    np.testing.assert_array_equal(estimate.mean, mean)
    assert estimate.replicates.shape == (3, len(w)) and np.all(estimate.standard_error > 0)
    with pytest.raises(AttributeError):
        estimate.mean = None  # frozen


# ----------------------------------------------------------------------------- replicate_errors
def _fits(position, hwhm, height, status):
    position, hwhm, height = (np.asarray(a, dtype=np.float64) for a in (position, hwhm, height))
    status = np.asarray(status, dtype=np.int32)
    return LorentzianFits(height=height, position=position, hwhm=hwhm, baseline=0 * height,
                          area=np.pi * height * hwhm, integral=height, centroid=position, rss=0 * height, status=status,
                          iterations=np.ones_like(status))


def test_replicate_errors_formulas_and_exclusions():
    rng = np.random.default_rng(3)
    position = 500.0 + rng.normal(size=(6, 2))
    hwhm = 4.0 + 0.3 * rng.normal(size=(6, 2))
    height = 2.0 + 0.1 * rng.normal(size=(6, 2))
    status = np.zeros((6, 2), dtype=np.int32)
    status[[1, 4], 1] = (3, 1)  # window 1 loses two replicates
    position[1, 1] = np.nan
    fits = _fits(position, hwhm, height, status)
    keep = [np.arange(6), np.array([0, 2, 3, 5])]
    for method in ("bootstrap", "jackknife", "blocks"):
        errors = replicate_errors(fits, method)
        np.testing.assert_array_equal(errors.used, [6, 4])
        for name, values in (("position_error", position), ("hwhm_error", hwhm), ("lifetime_ps_error", fits.lifetime_ps),
                             ("area_error", fits.area)):
            for window in range(2):
                x = values[keep[window], window]
                m = len(x)
                want = {"bootstrap": x.std(ddof=1), "jackknife": np.sqrt((m - 1) / m * np.sum((x - x.mean()) ** 2)),
                        "blocks": x.std(ddof=1) / np.sqrt(m)}[method]
                np.testing.assert_allclose(getattr(errors, name)[window], want, rtol=1e-12)
    # G named by the caller: the jackknife's factor and the blocks' root use it
    errors = replicate_errors(fits, "jackknife", blocks_count=6)
    x = position[keep[1], 1]
    np.testing.assert_allclose(errors.position_error[1], np.sqrt(5 / 6 * np.sum((x - x.mean()) ** 2)), rtol=1e-12)
    # fewer than two usable replicates: NaN, and nothing else is touched
    status[1:, 0] = 2
    errors = replicate_errors(_fits(position, hwhm, height, status), "bootstrap")
    np.testing.assert_array_equal(errors.used, [1, 4])
    assert np.isnan(errors.position_error[0]) and np.isnan(errors.lifetime_ps_error[0]) and np.isnan(errors.area_error[0])
    assert np.isfinite(errors.position_error[1])
    status[:, 0] = 1
    assert replicate_errors(_fits(position, hwhm, height, status), "blocks").used[0] == 0
    with pytest.raises(ValueError, match="unknown method"):
        replicate_errors(fits, "subsample")
    with pytest.raises(ValueError, match="replicate axis"):
        replicate_errors(_fits(500.0, 4.0, 2.0, 0), "bootstrap")


def test_replicate_standard_error_without_a_mask():
    rng = np.random.default_rng(4)
    x = rng.normal(size=(7, 3, 2))
    error, used = replicate_standard_error(x, "bootstrap")
    np.testing.assert_allclose(error, x.std(axis=0, ddof=1), rtol=1e-13)
    np.testing.assert_array_equal(used, np.full((3, 2), 7))
    assert np.all(np.isnan(replicate_standard_error(x[:1], "jackknife")[0]))


# ----------------------------------------------------------------------------- classes without replicates
def test_other_reducers_have_no_replicates():
    rng = np.random.default_rng(5)
    incr = rng.normal(size=(40, 2, 3, 3))
    positions = rng.uniform(size=(41, 3, 3))
    vectors = np.eye(9).reshape(9, 3, 3)[:2]
    spectra = [PartialMDRamanSpectrum(incr, TIMESTEP), PartialMDRamanEnsemble([incr, incr], TIMESTEP),
               ModeMDRamanSpectrum(incr, TIMESTEP), VibrationalDensityOfStates(positions, TIMESTEP, np.eye(3) * 5.0),
               ModeVibrationalDensityOfStates(positions, TIMESTEP, np.eye(3) * 5.0, vectors)]
    for spectrum in spectra:
        for call in (lambda s: measure_segment_replicates(s, 9),
                     lambda s: measure_segment_replicates_polarized(s, [1, 0, 0], [1, 0, 0], segment_steps=9),
                     lambda s: measure_segments_error(s, 9)):
            with pytest.raises(NotImplementedError, match="replicates are implemented for whole spectra"):
                call(spectrum)


# ----------------------------------------------------------------------------- the C interface
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
    host, device = table["rn_md_raman_segment_replicates"], table["rn_md_raman_segment_replicates_device"]
    assert device[0] == host[0] and device[1] == host[1] + [C.c_void_p]
    # rn_md_raman_segments_at with (replicate_weights, R) where it has `average`
    at = table["rn_md_raman_segments_at"][1]
    assert host[1] == at[:8] + [C.c_void_p, C.c_int64] + at[9:]


def test_argument_checks_come_before_the_device():
    """What the entry refuses without touching a GPU: the output keeps its prefill."""
    lib = _lib.load()
    alpha = np.ascontiguousarray(_series(60, 1))
    starts = np.array([0, 20, 43], dtype=np.int64)
    tau, weights, table = np.ones(16), np.ones((2, 21)), np.full((4, 3), 0.25)
    out = np.full((4, 2, 7), np.nan)

    def p(array):
        return None if array is None else C.c_void_p(array.ctypes.data)

    def call(alpha=alpha, starts=starts, count=3, tau=tau, weights=weights, k=2, table=table, r=4, out=out, bins=7):
        return lib.rn_md_raman_segment_replicates(p(alpha), 60, 17, p(starts), count, p(tau), p(weights), k, p(table), r,
                                                  0, 0, p(out), bins)

    invalid = _lib.RN_ERR_INVALID_ARGUMENT
    for name in ("alpha", "starts", "tau", "weights", "table", "out"):
        assert call(**{name: None}) == invalid, name
    assert call(r=0) == invalid and call(r=-2) == invalid and call(k=0) == invalid and call(count=0) == invalid
    for bad in (np.nan, np.inf):
        broken = table.copy()
        broken[3, 2] = bad
        assert call(table=broken) == invalid
    assert call(starts=np.array([0, 20, 44], dtype=np.int64)) == invalid
    assert call(starts=np.array([-1, 20, 43], dtype=np.int64)) == invalid
    assert call(bins=8) == invalid and call(bins=6) == invalid
    assert np.all(np.isnan(out))
