"""The nearest-reference search and the farthest-point selection on the GPU (``include/rn_select.h``) against the host
statements ``nearest_host`` and ``select_farthest_host``.

Tolerances.  Indices must be equal.  The test first asserts on the CPU (tests/selection_cases.py) that every decision is
clear of rounding: best and runner-up differ by more than ``1e-9 (|x'|^2 + |r'|^2)``, about 1e6 roundings of the product
form.  Distances: ``rtol = 1e-12``.  This is derived, not measured: the reported distances come from at most ``D <= 128``
squared differences in float64, summed in another order than numpy's, which bounds the difference by about ``D u =
1.4e-14``.

Shapes.  The search works on tiles of ``rn_select_tile_rows()`` = 64 rows of X, 64 rows of R and 16 columns; a reference
is split into ascending ranges of whole tiles so that about 256 workgroups run.  The cases straddle every edge: 63, 64 and
65 rows on either side, 15, 16 and 17 columns, the widths 1, 5, 14, 64 and 70, one row against one row, a reference of 5
ranges of one tile and one of 46 ranges of two tiles.  The selection owns slices of 128 rows: 1, 17 and 130 rows."""
import ctypes as C

import numpy as np
import pytest
import torch

from ramannoodle_amd import _lib, selection
from tests import guard_bands
from tests.selection_cases import GAP, farthest_case, farthest_gap, nearest_case, nearest_gap

pytestmark = pytest.mark.gpu

RTOL = 1e-12

# rows of X, rows of R, columns
NEAREST_SHAPES = [(1, 1, 1), (63, 65, 5), (64, 64, 14), (65, 63, 64), (17, 130, 70), (5, 40, 15), (5, 40, 16), (5, 40, 17),
                  (17, 300, 5), (130, 5763, 14)]


@pytest.fixture(autouse=True)
def _no_default_device_mode():
    torch.set_default_device(None)
    yield


def on_gpu(array):
    return torch.tensor(np.asarray(array), dtype=torch.float64, device="cuda:0")


@pytest.mark.parametrize("with_params", [False, True], ids=["plain", "center and scale"])
@pytest.mark.parametrize("shape", NEAREST_SHAPES, ids=lambda s: "S%d M%d D%d" % s)
def test_nearest_matches_the_host_statement(shape, with_params):
    x, r, center, scale = nearest_case(*shape, with_params)
    zeros, ones = np.zeros(shape[2]), np.ones(shape[2])
    margin = nearest_gap(x, r, zeros if center is None else center, ones if scale is None else scale)
    assert margin > GAP, margin
    if shape == (17, 300, 5):
        assert selection.reference_splits(17, 300) == 5
    if shape == (130, 5763, 14):
        assert selection.reference_splits(130, 5763) == 46  # 91 tiles in ranges of two: the last range holds one
    want_distance, want_index = selection.nearest_host(x, r, center, scale)
    distance, index = selection.nearest(x, r, center, scale, device=0)
    print(f"{shape}: margin {margin:.3e}, worst relative distance error "
          f"{np.max(np.abs(distance - want_distance) / want_distance):.3e}")
    np.testing.assert_array_equal(index, want_index)
    np.testing.assert_allclose(distance, want_distance, rtol=RTOL, atol=0)
    assert distance.shape == index.shape == (shape[0],) and index.dtype == np.int64


@pytest.mark.parametrize("with_params", [False, True], ids=["plain", "center and scale"])
def test_exact_duplicates_tie_to_the_lower_index_across_tiles_and_ranges(with_params):
    """150 rows and, behind them, exact copies of rows 3, 70 and 149: three tiles, one range each, so that a copy lies in
    another tile and another workgroup than its original (3, 70) or in the same tile (149)."""
    base, _, center, scale = nearest_case(150, 150, 14, with_params)
    originals = np.array([3, 70, 149])
    rows = np.concatenate([base, base[originals]])
    copies = np.arange(150, 153)
    assert selection.reference_splits(len(rows), len(rows)) == 3
    distance, index = selection.nearest(rows, rows, center, scale, device=0)
    want = np.arange(len(rows))
    want[copies] = originals
    np.testing.assert_array_equal(index, want)  # every row finds itself, a copy finds its original
    np.testing.assert_array_equal(distance, 0.0)
    # leave one out: never the row itself; an original finds its copy and a copy its original, at distance exactly 0
    # (among the distinct rows every choice is clear; an original and its copy tie exactly, which is the point)
    zeros, ones = np.zeros(14), np.ones(14)
    assert nearest_gap(base, base, zeros if center is None else center, ones if scale is None else scale, True) > GAP
    distance, index = selection.nearest(rows, rows, center, scale, exclude_self=True, device=0)
    assert not np.any(index == np.arange(len(rows)))
    np.testing.assert_array_equal(index[originals], copies)
    np.testing.assert_array_equal(index[copies], originals)
    np.testing.assert_array_equal(distance[np.concatenate([originals, copies])], 0.0)
    want_distance, want_index = selection.nearest_host(rows, rows, center, scale, exclude_self=True)
    np.testing.assert_array_equal(index, want_index)
    np.testing.assert_allclose(distance, want_distance, rtol=RTOL, atol=0)
    # a reference that holds a row three times, the copies first in other ranges: the lowest index wins
    reference = np.concatenate([base[:140], base[[7]], base[140:], base[[7]]])
    distance, index = selection.nearest(base[[7, 8]], reference, center, scale, device=0)
    np.testing.assert_array_equal(index, [7, 8])
    # one row, itself excluded: no candidate
    distance, index = selection.nearest(base[:1], base[:1], exclude_self=True, device=0)
    assert index[0] == -1 and np.isinf(distance[0])


@pytest.mark.parametrize("with_params", [False, True], ids=["plain", "scale"])
@pytest.mark.parametrize("mode", ["mean", "first", "reference"])
@pytest.mark.parametrize("rows,count", [(1, 1), (17, 1), (17, 17), (130, 1), (130, 130)])
def test_select_farthest_matches_the_host_statement(rows, count, mode, with_params):
    x, r, first, scale = farthest_case(rows, count, mode, with_params)
    margin = farthest_gap(x, count, r, first, np.ones(x.shape[1]) if scale is None else scale)
    assert margin > GAP, margin
    want_picks, want_distance = selection.select_farthest_host(x, count, r, first, scale=scale)
    picks, distance = selection.select_farthest(x, count, r, first, scale=scale, device=0)
    np.testing.assert_array_equal(picks, want_picks)
    np.testing.assert_allclose(distance, want_distance, rtol=RTOL, atol=0)  # (inf equals inf)
    assert picks.shape == distance.shape == (count,) and picks.dtype == np.int64
    if count == rows:
        assert sorted(picks) == list(range(rows))
    if mode != "reference":
        assert np.isinf(distance[0]) and np.all(np.isfinite(distance[1:]))


def test_copies_of_reference_rows_are_picked_last():
    x, r, _, _ = farthest_case(130, 130, "reference", False)
    rows = np.concatenate([r[:3], x[:20], r[5:7]])
    picks, distance = selection.select_farthest(rows, len(rows), reference=r, device=0)
    assert sorted(picks) == list(range(len(rows)))
    assert set(picks[-5:]) == {0, 1, 2, 23, 24} and np.all(distance[-5:] == 0) and np.all(distance[:-5] > 0)
    np.testing.assert_array_equal(picks[-5:], [0, 1, 2, 23, 24])  # equal values: the lowest index first


@pytest.mark.parametrize("lead", guard_bands.LEADS, ids=["aligned", "odd"])
def test_device_views_inside_guarded_buffers(lead):
    """X and R as views inside NaN-banded device buffers, the results in banded host arrays: the bands are intact, every
    result element is written, and the results equal those of the host-array calls bit for bit."""
    x, r, center, scale = nearest_case(65, 63, 64, True)
    plain = selection.nearest(x, r, center, scale, device=0)
    plain_picks = selection.select_farthest(x, 9, r, center=center, scale=scale, device=0)
    plain_unseeded = selection.select_farthest(x, 9, scale=scale, device=0)
    x_buffer, x_view = guard_bands.banded(x, torch.float64, lead, guard_bands.NAN, device="cuda:0", row=64)
    r_buffer, r_view = guard_bands.banded(r, torch.float64, lead, guard_bands.NAN, device="cuda:0", row=64)
    with guard_bands.banded_host_results(selection, lead) as results:
        got = selection.nearest(x_view, r_view, center, scale)
        got_picks = selection.select_farthest(x_view, 9, r_view, center=center, scale=scale)
        got_unseeded = selection.select_farthest(x_view, 9, scale=scale)
    torch.cuda.synchronize()
    assert len(results) == 6
    for buffer, view in results:
        guard_bands.assert_bands_intact(buffer, view, "a host result")
        guard_bands.assert_overwritten(buffer, view, "a host result")
    guard_bands.assert_bands_intact(x_buffer, x_view, "X")
    guard_bands.assert_bands_intact(r_buffer, r_view, "R")
    guard_bands.assert_same_bits(x_view, x, "X")
    guard_bands.assert_same_bits(r_view, r, "R")
    for ours, theirs in ((got, plain), (got_picks, plain_picks), (got_unseeded, plain_unseeded)):
        np.testing.assert_array_equal(ours[0], theirs[0])
        np.testing.assert_array_equal(ours[1], theirs[1])
    with pytest.raises(ValueError, match="both"):
        selection.nearest(x_view, r)
    with pytest.raises(ValueError, match="contiguous float64 CUDA"):
        selection.nearest(x_view.float(), r_view)


def test_a_small_call_after_a_larger_one_repeats_its_bits_and_phase_times():
    lib = _lib.load()
    small = nearest_case(5, 40, 15, True)
    larger = nearest_case(130, 5763, 14, False)
    first = selection.nearest(*small, device=0) + selection.select_farthest(small[0], 5, small[1], device=0)
    selection.nearest(*larger, device=0)
    selection.select_farthest(larger[0], 130, larger[1], device=0)
    times = np.full(4, -1.0)
    assert lib.rn_select_phase_times(C.c_void_p(times.ctypes.data)) == _lib.RN_OK and not times.any()
    assert lib.rn_select_set_profiling(1) == _lib.RN_OK
    try:
        again = selection.nearest(*small, device=0)
        assert lib.rn_select_phase_times(C.c_void_p(times.ctypes.data)) == _lib.RN_OK
        assert times[0] > 0 and times[1] > 0 and times[2] == 0 and times[3] > 0, times
        again += selection.select_farthest(small[0], 5, small[1], device=0)
        assert lib.rn_select_phase_times(C.c_void_p(times.ctypes.data)) == _lib.RN_OK
        assert np.all(times > 0), times
    finally:
        assert lib.rn_select_set_profiling(0) == _lib.RN_OK
    for before, after in zip(first, again):
        np.testing.assert_array_equal(after, before)
