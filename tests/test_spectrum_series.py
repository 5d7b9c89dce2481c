"""The holder of an MD spectrum class's time series (``spectrum._Series``): its segment tables against
``segment_plan`` / ``_segment_starts`` / ``ensemble_segment_starts`` called directly, the gap rows between joined runs of
increments, and the refusals that need no GPU.  Host only."""
import numpy as np
import pytest
import torch

from ramannoodle_amd.spectrum import _Series, _segment_starts, ensemble_segment_starts, segment_plan

W, HOP = 9, 4
RUN_SETS = [(17, 17), (33, 21)]


def _increments(frames: int, seed: int):
    return np.random.default_rng(seed).normal(size=(frames - 1, 3, 3, 3))


def _same_table(table, want):
    assert table[0] == want[0]
    np.testing.assert_array_equal(table[1], want[1])
    np.testing.assert_array_equal(table[2], want[2])
    assert table[2].dtype == np.int64


@pytest.mark.parametrize("taper", ["hann", "boxcar"])
@pytest.mark.parametrize("increments", [False, True])
def test_single_run_tables_are_the_hop_grid(taper, increments):
    frames = 33
    series = _Series(np.zeros((frames - int(increments), 3, 3)), increments=increments)
    assert series.frames == frames and series.gpu is None and series.host() is series.data
    source, stream = series.source(0)
    assert source is series.data and stream is None
    width, hop, tau = segment_plan(frames, W, HOP, taper)
    _same_table(series.segment_table(W, HOP, taper), (width, tau, _segment_starts(frames, width, hop)))
    np.testing.assert_array_equal(series.segment_starts(W, HOP), _segment_starts(frames, W, HOP))
    np.testing.assert_array_equal(series.segment_starts(W), _segment_starts(frames, W, W // 2))  # the default hop
    _same_table(series.whole_table(), (frames, np.ones(frames - 1), np.zeros(1, dtype=np.int64)))


@pytest.mark.parametrize("taper", ["hann", "boxcar"])
@pytest.mark.parametrize("lengths", RUN_SETS)
def test_ensemble_tables_are_the_segments_of_every_run(lengths, taper):
    runs = [np.random.default_rng(index).normal(size=(length, 3, 3)) for index, length in enumerate(lengths)]
    series = _Series.of_runs(runs, (3, 3), False)
    assert series.run_lengths == list(lengths) and series.frames == sum(lengths)
    np.testing.assert_array_equal(series.data, np.concatenate(runs))
    width, hop, tau = segment_plan(min(lengths), W, HOP, taper)
    starts, run_index = ensemble_segment_starts(lengths, width, hop)
    _same_table(series.segment_table(W, HOP, taper), (width, tau, starts))
    got_run, got_start = series.segment_starts(W, HOP)
    np.testing.assert_array_equal(got_run, run_index)
    np.testing.assert_array_equal(got_start, starts - np.array([0, lengths[0]])[run_index])
    np.testing.assert_array_equal(got_start, np.concatenate([_segment_starts(length, W, HOP) for length in lengths]))


@pytest.mark.parametrize("lengths", RUN_SETS)
def test_runs_of_increments_are_joined_with_one_zero_row_that_no_segment_reads(lengths):
    runs = [_increments(length, index) for index, length in enumerate(lengths)]
    series = _Series.of_runs(runs, (3, 3), True, increments=True)
    assert series.run_lengths == list(lengths)  # frames: one more than each run's increments
    assert series.shape == (sum(lengths) - 1, 3, 3, 3) and series.frames == sum(lengths)
    first = lengths[0]
    np.testing.assert_array_equal(series.data[:first - 1], runs[0])
    np.testing.assert_array_equal(series.data[first - 1], np.zeros((3, 3, 3)))  # exactly one gap row
    np.testing.assert_array_equal(series.data[first:], runs[1])
    assert np.all(series.data[first] != 0.0)
    for taper in ("hann", "boxcar"):
        width, _, starts = series.segment_table(W, HOP, taper)
        run_index, within = series.segment_starts(W, HOP)
        offsets = np.array([0, first])[run_index]
        np.testing.assert_array_equal(starts, offsets + within)
        last_frame = starts + width - 1  # the last frame of segment q; it reads increments starts .. last_frame - 1
        assert np.all(within >= 0) and np.all(last_frame <= offsets + np.array(lengths)[run_index] - 1)
        read = starts[:, None] + np.arange(width - 1)[None, :]
        assert first - 1 not in read
        assert (run_index == 0).any() and (run_index == 1).any()


def test_whole_table_is_one_boxcar_segment_per_run_of_runs_of_one_length():
    runs = [_increments(17, 0), _increments(17, 1)]
    series = _Series.of_runs(runs, (3, 3), True, increments=True)
    _same_table(series.whole_table(), (17, np.ones(16), np.array([0, 17], dtype=np.int64)))
    unequal = _Series.of_runs([_increments(33, 0), _increments(21, 1)], (3, 3), True, increments=True)
    message = r"the mean of the runs' whole spectra needs runs of one length, not \[21, 33\]: use measure_segments"
    with pytest.raises(ValueError, match=message):
        unequal.whole_table()
    with pytest.raises(ValueError, match=message):
        _Series.of_runs([np.zeros((33, 3, 3)), np.zeros((21, 3, 3))], (3, 3), False).whole_table("too few")
    # fewer than three frames: segment_plan's message, or the caller's
    short = _Series(np.zeros((1, 2, 3, 3)), increments=True)
    with pytest.raises(ValueError, match="invalid segment_steps: 2 < 3"):
        short.whole_table()
    with pytest.raises(ValueError, match="^too few$"):
        short.whole_table("too few")
    with pytest.raises(ValueError, match="invalid segment_steps: 22 > 21 time steps"):
        unequal.segment_table(22, None, "hann")


def test_host_runs_are_checked_as_the_ensembles_always_did():
    with pytest.raises(ValueError, match="^an ensemble needs at least one run$"):
        _Series.of_runs([], (3, 3), False)
    with pytest.raises(ValueError, match=r"runs\[1\] has wrong shape: \(5,2,3,3\) != \(_,3,3,3\)"):
        _Series.of_runs([np.zeros((5, 3, 3, 3)), np.zeros((5, 2, 3, 3))], (3, 3), True, increments=True)
    with pytest.raises(TypeError, match=r"runs\[0\] should have type ndarray, not list"):
        _Series.of_runs([[1.0]], (3, 3), False)


def test_run_lengths_of_a_joined_tensor_are_checked_before_the_tensor_is():
    """Every ``run_lengths`` refusal that can be reached without a CUDA tensor; a host tensor that passes them is then
    refused for not being one."""
    joined = torch.zeros((33, 3, 3), dtype=torch.float64)
    pattern = (None, 3, 3)
    with pytest.raises(ValueError, match="^runs: one joined tensor needs run_lengths$"):
        _Series.of_tensor_runs("runs", joined, None, pattern)
    for lengths in ([20, 14], [33, 0], [], [17, 17]):
        text = rf"^runs: run_lengths \[{', '.join(map(str, lengths))}\] do not add up to the 33 rows of the tensor$"
        with pytest.raises(ValueError, match=text):
            _Series.of_tensor_runs("runs", joined, lengths, pattern)
    # increments: sum(run_lengths) - 1 rows
    with pytest.raises(ValueError, match=r"^runs: run_lengths \[17, 16\] do not add up to the 33 rows of the tensor$"):
        _Series.of_tensor_runs("runs", torch.zeros((33, 2, 3, 3), dtype=torch.float64), [17, 16], (None, None, 3, 3),
                               increments=True)
    with pytest.raises(ValueError, match="^runs must be a contiguous float64 CUDA tensor$"):
        _Series.of_tensor_runs("runs", joined, [17, 16], pattern)
    with pytest.raises(ValueError, match="^positions_ts must be a contiguous float64 CUDA tensor$"):
        _Series.of_tensor_runs("positions_ts", joined, [33], pattern)
    with pytest.raises(ValueError, match=r"^runs has wrong shape: \(33, 3, 3\) != \(_,_,3,3\)$"):
        _Series.of_tensor_runs("runs", joined, [17, 17], (None, None, 3, 3), increments=True)
    with pytest.raises(ValueError, match="^runs: run_lengths goes with one joined tensor, not with a sequence of runs$"):
        _Series.of_tensor_runs("runs", [joined], [33], pattern)
    with pytest.raises(ValueError, match="^an ensemble needs at least one run$"):
        _Series.of_tensor_runs("runs", [], None, pattern)
    with pytest.raises(ValueError, match="^runs must be contiguous float64 CUDA tensors$"):
        _Series.of_tensor_runs("runs", [np.zeros((5, 2, 3, 3))], None, (None, None, 3, 3), increments=True,
                               tensors_only=True)


def test_device_or_host_resolves_the_public_pair():
    series = _Series(np.zeros((5, 3, 3)))
    assert series.device_or_host(None, False) is None and series.device_or_host(2, False) == 2
    assert series.device_or_host(2, True) is None
