"""``ramannoodle_amd.selection`` on the host: ``nearest_host`` and ``select_farthest_host`` against brute-force loops
over their definitions (tests/selection_cases.py) on tiny arrays, every refusal of the front end and of the C entries
(which check their arguments before they touch a device), and the agreement of include/rn_select.h with the ctypes
table.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ramannoodle_amd import _lib, selection
from tests.selection_cases import brute_farthest, brute_nearest, farthest_case, nearest_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rn_select_nearest", "rn_select_nearest_device", "rn_select_farthest", "rn_select_farthest_device",
           "rn_select_tile_rows", "rn_select_reference_splits", "rn_select_set_profiling", "rn_select_phase_times",
           "rn_select_last_error")


@pytest.mark.parametrize("with_params", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 1), (7, 5, 3), (4, 9, 14)])
def test_nearest_host_is_the_definition(shape, with_params):
    x, r, center, scale = nearest_case(*shape, with_params)
    distance, index = selection.nearest(x, r, center, scale)  # device=None and host arrays: the host function
    squared, want = brute_nearest(x, r, scale)
    np.testing.assert_array_equal(index, want)
    np.testing.assert_allclose(distance, np.sqrt(squared), rtol=1e-13)
    assert distance.dtype == np.float64 and index.dtype == np.int64 and distance.shape == index.shape == (shape[0],)


def test_nearest_host_ties_go_to_the_lowest_index():
    r = np.array([[0.0, 1.0], [2.0, 0.0], [0.0, 1.0], [-2.0, 0.0], [2.0, 0.0]])
    x = np.array([[0.0, 1.0], [0.0, 0.0], [2.0, 0.0], [0.0, -7.0]])
    distance, index = selection.nearest_host(x, r)
    np.testing.assert_array_equal(index, [0, 0, 1, 1])  # (row 3: rows 1, 3 and 4 are equally far; row 1: 0 and 2)
    np.testing.assert_array_equal(index, brute_nearest(x, r)[1])
    np.testing.assert_array_equal(distance[[0, 2]], 0.0)


def test_nearest_host_exclude_self():
    x = nearest_case(9, 9, 4, False)[0]
    rows = np.concatenate([x, x[[2, 5]]])  # rows 9 and 10 repeat rows 2 and 5
    distance, index = selection.nearest_host(rows, rows, exclude_self=True)
    assert not np.any(index == np.arange(len(rows)))
    np.testing.assert_array_equal(index, brute_nearest(rows, rows, exclude_self=True)[1])
    np.testing.assert_array_equal(index[[2, 5, 9, 10]], [9, 10, 2, 5])
    np.testing.assert_array_equal(distance[[2, 5, 9, 10]], 0.0)
    plain = selection.nearest_host(rows, rows)
    np.testing.assert_array_equal(plain[1][:9], np.arange(9))  # (without it every row finds itself, or its first copy)
    np.testing.assert_array_equal(plain[1][9:], [2, 5])
    # a single row has no neighbour but itself
    alone = selection.nearest_host(x[:1], x[:1], exclude_self=True)
    assert alone[1][0] == -1 and np.isinf(alone[0][0])


@pytest.mark.parametrize("with_params", [False, True])
@pytest.mark.parametrize("mode", ["mean", "first", "reference"])
@pytest.mark.parametrize("rows,count", [(1, 1), (6, 1), (6, 6), (11, 4)])
def test_select_farthest_host_is_the_definition(rows, count, mode, with_params):
    x, r, first, scale = farthest_case(rows, count, mode, with_params, columns=3, references=4)
    picks, distance = selection.select_farthest(x, count, r, first, scale=scale)
    want, squared = brute_farthest(x, count, r, first, scale)
    np.testing.assert_array_equal(picks, want)
    np.testing.assert_allclose(distance, np.sqrt(squared), rtol=1e-13)
    assert picks.dtype == np.int64 and picks.shape == distance.shape == (count,)
    if mode == "first":
        assert picks[0] == first
    if mode != "reference":
        assert np.isinf(distance[0])


@pytest.mark.parametrize("mode", ["mean", "reference"])
def test_count_equal_to_the_rows_is_a_permutation_with_falling_distances(mode):
    x, r, first, scale = farthest_case(11, 11, mode, False, columns=3, references=4)
    rows = np.concatenate([x, x[[0, 3]]])  # with exact copies: they come last, at distance 0, the lower index first
    picks, distance = selection.select_farthest_host(rows, len(rows), r, first, scale=scale)
    assert sorted(picks) == list(range(len(rows)))
    assert np.all(np.diff(distance) <= 0)
    np.testing.assert_array_equal(distance[-2:], 0.0)
    assert set(picks[-2:]) == {11, 12} and np.all(distance[:-2] > 0)


def test_a_reference_set_seeds_the_selection():
    x, r, _, _ = farthest_case(11, 4, "reference", False, columns=3, references=4)
    picks, distance = selection.select_farthest_host(x, 4, reference=r)
    seed_distance = selection.nearest_host(x, r)[0]
    assert picks[0] == np.argmax(seed_distance) and distance[0] == seed_distance.max()
    # rows that are in the reference set are the last to be picked: their distance is 0 from the start
    both = np.concatenate([r[:2], x])
    picks, distance = selection.select_farthest_host(both, len(both), reference=r)
    assert set(picks[-2:]) == {0, 1} and np.all(distance[-2:] == 0) and np.all(distance[:-2] > 0)
    # an empty reference is no reference
    np.testing.assert_array_equal(selection.select_farthest_host(x, 4, reference=np.zeros((0, 3)))[0],
                                  selection.select_farthest_host(x, 4)[0])


BAD = np.array([[0.0, 1.0], [np.nan, 2.0]])
GOOD = np.array([[0.0, 1.0], [3.0, 2.0], [1.0, 1.0]])


@pytest.mark.parametrize("device", [None, 0])
def test_every_refusal_of_the_front_end(device):
    """With a device the same checks run before the library is asked for anything: no GPU is needed to be refused."""
    with pytest.raises(ValueError, match="descriptors"):
        selection.nearest(np.zeros(3), GOOD, device=device)
    with pytest.raises(ValueError, match="reference"):
        selection.nearest(GOOD, np.zeros((2, 2, 2)), device=device)
    with pytest.raises(ValueError, match="D = 3"):
        selection.nearest(GOOD, np.zeros((4, 3)), device=device)
    with pytest.raises(ValueError, match="at least 1"):
        selection.nearest(GOOD, np.zeros((0, 2)), device=device)
    with pytest.raises(ValueError, match=r"descriptors\[1\]\[0\] is not finite"):
        selection.nearest(BAD, GOOD, device=device)
    with pytest.raises(ValueError, match=r"reference\[1\]\[0\] is not finite"):
        selection.nearest(GOOD, BAD, device=device)
    with pytest.raises(ValueError, match="scale"):
        selection.nearest(GOOD, GOOD, scale=np.ones(3), device=device)
    with pytest.raises(ValueError, match=r"center\[1\] is not finite"):
        selection.nearest(GOOD, GOOD, center=np.array([0.0, np.inf]), device=device)
    with pytest.raises(ValueError, match="count = 4"):
        selection.select_farthest(GOOD, 4, device=device)
    with pytest.raises(ValueError, match="count"):
        selection.select_farthest(GOOD, -1, device=device)
    with pytest.raises(ValueError, match="count"):
        selection.select_farthest(GOOD, 1.5, device=device)
    with pytest.raises(ValueError, match="first = 3"):
        selection.select_farthest(GOOD, 2, first=3, device=device)
    with pytest.raises(ValueError, match="reference decides"):
        selection.select_farthest(GOOD, 2, reference=GOOD, first=0, device=device)
    with pytest.raises(ValueError, match="D = 3"):
        selection.select_farthest(GOOD, 2, reference=np.zeros((4, 3)), device=device)
    with pytest.raises(ValueError, match=r"descriptors\[1\]\[0\] is not finite"):
        selection.select_farthest(BAD, 1, device=device)


def _pointer(array):
    return C.c_void_p(None if array is None else array.ctypes.data)


def test_the_c_entries_refuse_before_they_touch_a_device():
    lib = _lib.load()
    x, r = np.ascontiguousarray(GOOD), np.ascontiguousarray(GOOD[:2])
    squared, index = np.zeros(3), np.zeros(3, dtype=np.int64)

    def nearest_rc(x=x, rows=3, r=r, refs=2, columns=2, center=None, scale=None, out=squared):
        return lib.rn_select_nearest(0, _pointer(x), rows, _pointer(r), refs, columns, _pointer(center), _pointer(scale), 0,
                                     _pointer(out), _pointer(index))

    def farthest_rc(x=x, rows=3, r=None, refs=0, first=-1, count=2):
        return lib.rn_select_farthest(0, _pointer(x), rows, 2, _pointer(r), refs, None, None, first, count, _pointer(index),
                                      _pointer(squared))

    def text():
        return lib.rn_select_last_error().decode()

    assert nearest_rc(columns=0) == _lib.RN_ERR_INVALID_ARGUMENT and "D = 0" in text()
    assert nearest_rc(refs=0) == _lib.RN_ERR_INVALID_ARGUMENT and "M = 0" in text()
    assert nearest_rc(rows=-1) == _lib.RN_ERR_INVALID_ARGUMENT
    assert nearest_rc(x=None) == _lib.RN_ERR_INVALID_ARGUMENT and "null" in text()
    assert nearest_rc(out=None) == _lib.RN_ERR_INVALID_ARGUMENT and "null" in text()
    assert nearest_rc(x=np.ascontiguousarray(BAD), rows=2) == _lib.RN_ERR_INVALID_ARGUMENT and "X[1][0]" in text()
    assert nearest_rc(r=np.ascontiguousarray(BAD)) == _lib.RN_ERR_INVALID_ARGUMENT and "R[1][0]" in text()
    assert nearest_rc(scale=np.array([1.0, np.nan])) == _lib.RN_ERR_INVALID_ARGUMENT and "scale[1]" in text()
    assert nearest_rc(center=np.array([np.inf, 0.0])) == _lib.RN_ERR_INVALID_ARGUMENT and "center[0]" in text()
    assert nearest_rc(rows=0) == _lib.RN_OK  # S = 0 is a no-op, with or without a GPU
    assert farthest_rc(count=4) == _lib.RN_ERR_INVALID_ARGUMENT and "count = 4" in text()
    assert farthest_rc(count=-1) == _lib.RN_ERR_INVALID_ARGUMENT
    assert farthest_rc(first=3) == _lib.RN_ERR_INVALID_ARGUMENT and "first = 3" in text()
    assert farthest_rc(r=r, refs=2, first=0) == _lib.RN_ERR_INVALID_ARGUMENT and "reference decides" in text()
    assert farthest_rc(r=None, refs=2) == _lib.RN_ERR_INVALID_ARGUMENT and "null" in text()
    assert farthest_rc(count=0) == _lib.RN_OK and farthest_rc(rows=0, count=0) == _lib.RN_OK
    assert lib.rn_select_phase_times(None) == _lib.RN_ERR_INVALID_ARGUMENT
    # a refusal leaves the results alone
    assert not squared.any() and not index.any()


def test_header_and_ctypes_table_agree():
    with open(os.path.join(ROOT, "include", "rn_select.h"), encoding="utf-8") as file:
        header = re.sub(r"/\*.*?\*/", "", file.read(), flags=re.S)
    assert set(re.findall(r"\b(rn_\w+)\s*\(", header)) == set(ENTRIES)
    assert set(_lib.SELECT_SIGNATURES) == set(ENTRIES)
    for other in (_lib.SIGNATURES, _lib.INTERP_SIGNATURES, _lib.LINESHAPE_SIGNATURES, _lib.PEAKFIT_SIGNATURES,
                  _lib.QH_SIGNATURES, _lib.HT_SIGNATURES, _lib.BM_SIGNATURES):
        assert not set(ENTRIES) & set(other)
    lib = _lib.load()
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == _lib.SELECT_SIGNATURES[name][1]
    for name in ("rn_select_nearest", "rn_select_farthest"):  # the device entry: the same arguments and a stream
        host, device = _lib.SELECT_SIGNATURES[name], _lib.SELECT_SIGNATURES[name + "_device"]
        assert device[0] == host[0] and device[1] == host[1] + [C.c_void_p]
    assert lib.rn_select_tile_rows() == 64
    assert lib.rn_select_reference_splits(1, 1) == 1 and lib.rn_select_reference_splits(17, 300) == 5
    assert lib.rn_select_reference_splits(130, 5763) == 46  # 91 tiles, two a range


def test_descriptors_need_a_model_with_a_latent_space():
    from ramannoodle_amd.dynamics import Trajectory, TrajectoryEnsemble

    class NoLatentSpace:  # what the interpolation models look like from here
        num_atoms = 2

    run = Trajectory(np.zeros((3, 2, 3)), 1.0)
    for frames in (run, TrajectoryEnsemble([run, run])):
        with pytest.raises(TypeError, match="latent space"):
            frames.get_descriptors(NoLatentSpace())
