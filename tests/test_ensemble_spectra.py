"""MD Raman spectra averaged over several runs, whole and by atom group, on the host (``MDRamanEnsemble``,
``PartialMDRamanEnsemble``, ``PartialMDRamanSpectrum.measure_segments``, ``dynamics.TrajectoryEnsemble``), anchored to
classes that know neither runs nor segments: every boxcar row against the spectrum of its own slice of its own run, the
mean against the rows, one run against ``MDRamanSpectrum``, a constant offset between runs (which a segment across the
boundary would see), permuted runs, the sum rule and the diagonal of the partial spectra, the start table and the
errors.  No GPU needed."""
import numpy as np
import pytest

from ramannoodle_amd import _lib
from ramannoodle_amd.dynamics import Trajectory, TrajectoryEnsemble
from ramannoodle_amd.spectrum import (MDRamanEnsemble, MDRamanSpectrum, PartialMDRamanEnsemble, PartialMDRamanSpectrum,
                                      ensemble_segment_starts)
from tests.test_polarized_spectra_gpu import CORRECTIONS, _close, _configurations, _series

RUNS = [50, 81, 64]
WIDTH, HOP = 17, 5
TIMESTEP = 1.5
TOL = 1e-10


def _runs(lengths=RUNS, seed=3):
    return [_series(steps, seed + 7 * r) for r, steps in enumerate(lengths)]


def _increment_runs(lengths=RUNS, groups=3, seed=5):
    """Per-group increments ``(S_r - 1, G, 3, 3)`` of each run, symmetric."""
    rng = np.random.default_rng(seed)
    runs = []
    for steps in lengths:
        t = np.arange(steps - 1)[:, None, None, None]
        freq = 1 + np.arange(groups * 9).reshape(1, groups, 3, 3) % 23
        incr = 0.05 * rng.normal(size=(steps - 1, groups, 3, 3)) + np.cos(0.01 * t * freq + rng.uniform(0, 6))
        runs.append(incr + np.swapaxes(incr, 2, 3))
    return runs


def test_segment_table_of_three_runs():
    starts, run_index = ensemble_segment_starts(RUNS, WIDTH, HOP)
    # (50 - 17) // 5 + 1 = 7, (81 - 17) // 5 + 1 = 13 and (64 - 17) // 5 + 1 = 10 segments; offsets 0, 50 and 131
    want = [0, 5, 10, 15, 20, 25, 30,
            50, 55, 60, 65, 70, 75, 80, 85, 90, 95, 100, 105, 110,
            131, 136, 141, 146, 151, 156, 161, 166, 171, 176]
    np.testing.assert_array_equal(starts, want)
    np.testing.assert_array_equal(run_index, [0] * 7 + [1] * 13 + [2] * 10)
    assert starts.dtype == np.int64 and run_index.dtype == np.int64
    # no segment crosses a boundary: its last step lies in its own run
    ends = np.cumsum(RUNS)
    assert np.all(starts + WIDTH <= ends[run_index])
    # the default hop is half a segment
    starts, run_index = ensemble_segment_starts([40, 20], 16)
    np.testing.assert_array_equal(starts, [0, 8, 16, 24, 40])
    np.testing.assert_array_equal(run_index, [0, 0, 0, 0, 1])
    run, within = MDRamanEnsemble(_runs(), TIMESTEP).segment_starts(WIDTH, HOP)
    np.testing.assert_array_equal(run, [0] * 7 + [1] * 13 + [2] * 10)
    np.testing.assert_array_equal(within, list(range(0, 31, 5)) + list(range(0, 61, 5)) + list(range(0, 46, 5)))


def test_boxcar_rows_are_the_spectra_of_the_slices():
    runs = _runs()
    e_i, e_s, rotations = _configurations(7, 7)
    ensemble = MDRamanEnsemble(runs, TIMESTEP)
    run_index, within = ensemble.segment_starts(WIDTH, HOP)
    for kwargs in ({}, CORRECTIONS):
        wavenumbers, rows = ensemble.measure_segments_polarized(e_i, e_s, rotations, segment_steps=WIDTH, hop=HOP,
                                                                taper="boxcar", average=False, **kwargs)
        assert rows.shape == (30, 7, len(wavenumbers))
        for q, (r, a) in enumerate(zip(run_index, within)):
            w_want, want = MDRamanSpectrum(runs[r][a:a + WIDTH], TIMESTEP).measure_polarized(e_i, e_s, rotations,
                                                                                             **kwargs)
            np.testing.assert_array_equal(wavenumbers, w_want)
            _close(rows[q], want, TOL)
    _, rows = ensemble.measure_segments(WIDTH, HOP, "boxcar", False)
    for q, (r, a) in enumerate(zip(run_index, within)):
        _close(rows[q], MDRamanSpectrum(runs[r][a:a + WIDTH], TIMESTEP).measure()[1], TOL)


def test_average_is_the_mean_of_the_rows():
    e_i, e_s, rotations = _configurations(7, 1)
    ensemble = MDRamanEnsemble(_runs(), TIMESTEP)
    segments = {"segment_steps": WIDTH, "hop": HOP, "taper": "hann"}
    for kwargs in ({}, CORRECTIONS):
        _, rows = ensemble.measure_segments_polarized(e_i, e_s, rotations, average=False, **segments, **kwargs)
        _, mean = ensemble.measure_segments_polarized(e_i, e_s, rotations, average=True, **segments, **kwargs)
        _close(mean, rows.mean(axis=0), TOL)
    _, rows = ensemble.measure_segments(average=False, **segments)
    _, mean = ensemble.measure_segments(average=True, **segments)
    _close(mean, rows.mean(axis=0), TOL)


def test_one_run_is_the_single_series():
    alpha = _series(200, 2)
    e_i, e_s, rotations = _configurations(7, 2)
    ensemble, single = MDRamanEnsemble([alpha], TIMESTEP), MDRamanSpectrum(alpha, TIMESTEP)
    for average in (True, False):
        for taper in ("hann", "blackman"):
            w_got, got = ensemble.measure_segments(33, 8, taper, average)
            w_want, want = single.measure_segments(33, 8, taper, average)
            np.testing.assert_array_equal(w_got, w_want)
            _close(got, want, TOL)
            _, got = ensemble.measure_segments_polarized(e_i, e_s, rotations, segment_steps=33, taper=taper,
                                                         average=average)
            _, want = single.measure_segments_polarized(e_i, e_s, rotations, segment_steps=33, taper=taper,
                                                        average=average)
            _close(got, want, TOL)
    _close(ensemble.measure()[1], single.measure()[1], TOL)
    _close(ensemble.measure_polarized(e_i, e_s, rotations)[1], single.measure_polarized(e_i, e_s, rotations)[1], TOL)


def test_no_segment_straddles_a_run_boundary():
    """Run 2 is run 1 plus a large constant tensor: a constant drops out of the differences within a run, and only a
    difference across the boundary would see it."""
    first = _series(60, 4)
    offset = 100.0 * (1.0 + np.arange(9.0).reshape(3, 3) + np.arange(9.0).reshape(3, 3).T)
    ensemble = MDRamanEnsemble([first, first + offset], TIMESTEP)
    e_i, e_s, rotations = _configurations(7, 4)
    segments = {"segment_steps": WIDTH, "hop": HOP, "taper": "hamming"}
    _, rows = ensemble.measure_segments_polarized(e_i, e_s, rotations, average=False, **segments)
    count = (60 - WIDTH) // HOP + 1
    assert rows.shape[0] == 2 * count
    _close(rows[count:], rows[:count], TOL)  # (offsets up to 1.7e3 cost the differences three of their sixteen digits)
    _, mean = ensemble.measure_segments_polarized(e_i, e_s, rotations, average=True, **segments)
    _, alone = MDRamanSpectrum(first, TIMESTEP).measure_segments_polarized(e_i, e_s, rotations, average=True,
                                                                           **segments)
    _close(mean, alone, TOL)


def test_permuting_the_runs_permutes_the_rows():
    runs = _runs()
    order = [2, 0, 1]
    e_i, e_s, rotations = _configurations(7, 9)
    segments = {"segment_steps": WIDTH, "hop": HOP}
    straight = MDRamanEnsemble(runs, TIMESTEP)
    permuted = MDRamanEnsemble([runs[r] for r in order], TIMESTEP)
    _, rows = straight.measure_segments_polarized(e_i, e_s, rotations, average=False, **segments)
    _, rows_p = permuted.measure_segments_polarized(e_i, e_s, rotations, average=False, **segments)
    run_index, _ = straight.segment_starts(WIDTH, HOP)
    _close(rows_p, np.concatenate([rows[run_index == r] for r in order]), TOL)
    _, mean = straight.measure_segments_polarized(e_i, e_s, rotations, **segments)
    _, mean_p = permuted.measure_segments_polarized(e_i, e_s, rotations, **segments)
    _close(mean_p, mean, TOL)


def test_whole_spectra_need_runs_of_one_length():
    runs = _runs([64, 64, 64])
    e_i, e_s, rotations = _configurations(7, 3)
    ensemble = MDRamanEnsemble(runs, TIMESTEP)
    wavenumbers, got = ensemble.measure(**CORRECTIONS)
    want = np.mean([MDRamanSpectrum(run, TIMESTEP).measure(**CORRECTIONS)[1] for run in runs], axis=0)
    np.testing.assert_array_equal(wavenumbers, MDRamanSpectrum(runs[0], TIMESTEP).measure()[0])
    _close(got, want, TOL)
    _, got = ensemble.measure_polarized(e_i, e_s, rotations)
    want = np.mean([MDRamanSpectrum(run, TIMESTEP).measure_polarized(e_i, e_s, rotations)[1] for run in runs], axis=0)
    _close(got, want, TOL)
    with pytest.raises(ValueError, match="one length"):
        MDRamanEnsemble(_runs(), TIMESTEP).measure()
    with pytest.raises(ValueError, match="one length"):
        MDRamanEnsemble(_runs(), TIMESTEP).measure_polarized(e_i, e_s, rotations)
    with pytest.raises(ValueError, match="one length"):
        PartialMDRamanEnsemble(_increment_runs(), TIMESTEP).measure()


def test_partial_sum_rule_against_the_whole_ensemble():
    incr = _increment_runs()
    e_i, e_s, rotations = _configurations(7, 5)
    partial = PartialMDRamanEnsemble(incr, TIMESTEP)
    whole = MDRamanEnsemble([np.concatenate([np.zeros((1, 3, 3)), np.cumsum(run.sum(axis=1), axis=0)]) for run in incr],
                            TIMESTEP)
    assert partial.run_lengths == RUNS
    for average in (True, False):
        for kwargs in ({}, CORRECTIONS):
            segments = {"segment_steps": WIDTH, "hop": HOP, "taper": "hann", "average": average}
            w_got, got = partial.measure_segments_polarized(e_i, e_s, rotations, **segments, **kwargs)
            w_want, want = whole.measure_segments_polarized(e_i, e_s, rotations, **segments, **kwargs)
            np.testing.assert_array_equal(w_got, w_want)
            assert got.shape == ((7, 3, 3, 7) if average else (30, 7, 3, 3, 7))
            np.testing.assert_array_equal(got, np.swapaxes(got, -2, -3))
            _close(got.sum(axis=(-2, -3)), want, TOL)
        _, got = partial.measure_segments(WIDTH, HOP, "hann", average)
        _, want = whole.measure_segments(WIDTH, HOP, "hann", average)
        _close(got.sum(axis=(-2, -3)), want, TOL)
    # the rows of the mean are the mean of the rows
    _, rows = partial.measure_segments(WIDTH, HOP, "blackman", False)
    _, mean = partial.measure_segments(WIDTH, HOP, "blackman", True)
    _close(mean, rows.mean(axis=0), TOL)


def test_partial_boxcar_rows_are_the_partial_spectra_of_the_slices():
    incr = _increment_runs()
    partial = PartialMDRamanEnsemble(incr, TIMESTEP)
    run_index, within = partial.segment_starts(WIDTH, HOP)
    np.testing.assert_array_equal(run_index, [0] * 7 + [1] * 13 + [2] * 10)
    wavenumbers, rows = partial.measure_segments(WIDTH, HOP, "boxcar", False)
    for q, (r, a) in enumerate(zip(run_index, within)):
        w_want, want = PartialMDRamanSpectrum(incr[r][a:a + WIDTH - 1], TIMESTEP).measure()
        np.testing.assert_array_equal(wavenumbers, w_want)
        for g in range(3):
            _close(rows[q, g, g], want[g, g], TOL)
        _close(rows[q], want, TOL)
    # a single series: the segments of PartialMDRamanSpectrum itself, and an ensemble of that one run
    single = PartialMDRamanSpectrum(incr[1], TIMESTEP)
    starts = single.segment_starts(WIDTH, HOP)
    np.testing.assert_array_equal(starts, np.arange(13) * HOP)
    _, rows = single.measure_segments(WIDTH, HOP, "boxcar", False)
    for q, a in enumerate(starts):
        _close(rows[q], PartialMDRamanSpectrum(incr[1][a:a + WIDTH - 1], TIMESTEP).measure()[1], TOL)
    _, alone = PartialMDRamanEnsemble([incr[1]], TIMESTEP).measure_segments(WIDTH, HOP, "boxcar", False)
    _close(alone, rows, TOL)
    # runs of one length: the mean of the runs' whole partial spectra
    equal = _increment_runs([40, 40])
    _, got = PartialMDRamanEnsemble(equal, TIMESTEP).measure()
    want = np.mean([PartialMDRamanSpectrum(run, TIMESTEP).measure()[1] for run in equal], axis=0)
    _close(got, want, TOL)


def test_a_run_shorter_than_a_segment_is_an_error():
    with pytest.raises(ValueError, match="segment_steps"):
        ensemble_segment_starts([50, 16, 64], WIDTH, HOP)
    with pytest.raises(ValueError, match="segment_steps"):
        MDRamanEnsemble(_runs([50, 16]), TIMESTEP).measure_segments(WIDTH, HOP)
    with pytest.raises(ValueError, match="segment_steps"):
        PartialMDRamanEnsemble(_increment_runs([50, 16]), TIMESTEP).measure_segments(WIDTH, HOP)
    with pytest.raises(ValueError):
        MDRamanEnsemble([], TIMESTEP)
    with pytest.raises(ValueError):
        ensemble_segment_starts([], WIDTH)


def test_trajectory_ensemble_refuses_mixed_runs():
    rng = np.random.default_rng(0)
    a = Trajectory(rng.uniform(size=(5, 4, 3)), 2.0)
    with pytest.raises(ValueError, match="timestep"):
        TrajectoryEnsemble([a, Trajectory(rng.uniform(size=(6, 4, 3)), 1.0)])
    with pytest.raises(ValueError, match="atoms"):
        TrajectoryEnsemble([a, Trajectory(rng.uniform(size=(6, 5, 3)), 2.0)])
    with pytest.raises(ValueError):
        TrajectoryEnsemble([])
    with pytest.raises(TypeError):
        TrajectoryEnsemble([a, rng.uniform(size=(6, 4, 3))])
    ensemble = TrajectoryEnsemble([a, Trajectory(rng.uniform(size=(6, 4, 3)), 2.0)])
    assert ensemble.run_lengths == [5, 6] and ensemble.timestep == 2.0

    class Constant:  # a model without the device entries
        def calc_polarizabilities(self, positions_batch):
            if positions_batch.shape[1] != 4:
                raise ValueError("wrong number of atoms")
            return np.cumsum(np.tile(np.eye(3), (len(positions_batch), 1, 1)), axis=0)

    spectrum = ensemble.get_raman_spectrum(Constant())
    assert isinstance(spectrum, MDRamanEnsemble) and spectrum.run_lengths == [5, 6]
    with pytest.raises(TypeError, match="calc_polarizabilities_device"):
        ensemble.get_raman_spectrum(Constant(), on_device=True)
    with pytest.raises(TypeError, match="calc_group_increments_device"):
        ensemble.get_partial_raman_spectrum(Constant(), "species")


def test_c_abi_table_lists_the_entries():
    for name in ("rn_md_raman_segments_at", "rn_md_raman_partial_segments"):
        host, device = _lib.SIGNATURES[name], _lib.SIGNATURES[name + "_device"]
        assert device[1][:-1] == host[1] and len(device[1]) == len(host[1]) + 1


def test_the_start_table_is_checked_before_any_device_work():
    """A bad table is refused on a machine without a GPU too; a good one gets as far as the device check."""
    import ctypes as C
    lib = _lib.load()

    def p(array):
        return C.c_void_p(array.ctypes.data)

    alpha, incr = np.zeros((200, 3, 3)), np.zeros((199, 2, 9))
    tau, weights = np.ones(63), np.ones((2, 21))
    out = np.zeros((3, 2, 3, 31))

    def both(starts, count=3):
        starts = np.array(starts, dtype=np.int64)
        return (lib.rn_md_raman_segments_at(p(alpha), 200, 64, p(starts), count, p(tau), p(weights), 2, 0, 0, 0, p(out), 31),
                lib.rn_md_raman_partial_segments(p(incr), 199, 2, 64, p(starts), count, p(tau), p(weights), 2, 0, 0, 0,
                                                 p(out), 31))

    invalid = (_lib.RN_ERR_INVALID_ARGUMENT,) * 2
    assert both([-1, 50, 136]) == invalid
    assert both([0, 50, 137]) == invalid  # 137 > S - W = N + 1 - W = 136
    assert both([0, 50, 136], count=0) == invalid
    assert all(rc != _lib.RN_ERR_INVALID_ARGUMENT for rc in both([0, 50, 136]))
