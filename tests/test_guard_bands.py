"""The guard-band helper on host buffers (tests/guard_bands.py) and the completeness of the table of
tests/guard_band_cases.py: every ``*_device`` / ``*_to_device`` entry of ``ramannoodle_amd/_lib.py`` has a guard-band
case, or is exempt because none of its pointers is device memory.  No GPU needed."""
import re

import numpy as np
import pytest

from ramannoodle_amd import spectrum
from tests.guard_band_cases import ENTRIES, EXEMPT, device_entry_names
from tests.guard_bands import (ALIGNED, LEADS, NAN, ODD, SENTINEL, assert_bands_intact, assert_overwritten, assert_same_bits,
                               banded, banded_host_results, fill_bits, interior_bits, prefill_bits)


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int32, np.int64])
@pytest.mark.parametrize("lead", LEADS)
def test_a_banded_input_is_a_contiguous_view_between_its_bands(dtype, lead):
    values = np.arange(3 * 5 * 7).reshape(3, 5, 7).astype(dtype)
    buffer, view = banded(values, dtype, lead, NAN)
    assert buffer.ndim == 1 and view.shape == values.shape and view.dtype == np.dtype(dtype)
    assert view.flags["C_CONTIGUOUS"] and np.shares_memory(view, buffer)
    offset = (view.ctypes.data - buffer.ctypes.data) // view.itemsize
    assert offset == lead and buffer.size - offset - view.size >= lead
    assert (view.ctypes.data % view.itemsize) == 0
    if lead == ODD:  # aligned to the element, and to nothing wider
        assert (view.ctypes.data - buffer.ctypes.data) % (2 * view.itemsize) == view.itemsize
    np.testing.assert_array_equal(view, values)
    if np.dtype(dtype).kind == "f":
        assert np.isnan(np.asarray(buffer)[:lead]).all() and np.isnan(np.asarray(buffer)[lead + view.size:]).all()
    assert_bands_intact(buffer, view)


def test_a_band_is_at_least_one_tile_row():
    buffer, view = banded((2, 5000), np.float64, ODD, SENTINEL, row=5000)
    offset = (view.ctypes.data - buffer.ctypes.data) // 8
    assert offset >= 5000 and buffer.size - offset - view.size >= 5000
    assert offset % 2 == 1  # (the alignment class of the lead is kept)
    assert_bands_intact(buffer, view)


def test_a_changed_band_element_is_reported_by_its_offset_from_the_view():
    buffer, view = banded((4, 9), np.float64, ALIGNED, SENTINEL)
    assert_bands_intact(buffer, view)
    np.asarray(buffer)[ALIGNED + view.size + 2] = 1.0
    with pytest.raises(AssertionError, match=re.escape("+3 elements past the end")):
        assert_bands_intact(buffer, view, "out")
    np.asarray(buffer)[ALIGNED + view.size + 2] = np.asarray(buffer)[0]
    assert_bands_intact(buffer, view)
    np.asarray(buffer)[ALIGNED - 5] = 0.0
    with pytest.raises(AssertionError, match=re.escape("-5 elements before the start")):
        assert_bands_intact(buffer, view, "out")


@pytest.mark.parametrize("dtype,as_int", [(np.float64, np.int64), (np.float32, np.int32)])
def test_a_changed_nan_payload_bit_is_reported(dtype, as_int):
    """The bands of an input are NaN: a comparison of values would pass whatever was written there; the bits do not."""
    buffer, view = banded(np.ones(6), dtype, ODD, NAN)
    band = np.asarray(buffer)[ODD + view.size:]
    assert np.isnan(band).all()
    band.view(as_int)[0] ^= 1  # still a NaN, another payload
    assert np.isnan(band).all()
    with pytest.raises(AssertionError, match=re.escape("+1 elements past the end")):
        assert_bands_intact(buffer, view, "positions")
    band.view(as_int)[0] ^= 1
    assert_bands_intact(buffer, view)
    # and a sentinel band against a canonical NaN written over it
    buffer, view = banded((6,), dtype, ALIGNED, SENTINEL)
    np.asarray(buffer)[ALIGNED - 1] = np.nan
    with pytest.raises(AssertionError, match=re.escape("-1 elements before the start")):
        assert_bands_intact(buffer, view)


def test_an_output_that_is_not_fully_written_is_reported():
    buffer, view = banded((3, 4), np.float64, ALIGNED, SENTINEL)
    assert fill_bits(np.float64, SENTINEL) != prefill_bits(np.float64) != fill_bits(np.float64, NAN)
    assert np.all(interior_bits(buffer, view) == prefill_bits(np.float64))
    with pytest.raises(AssertionError, match="12 elements never written"):
        assert_overwritten(buffer, view)
    view[...] = np.nan  # (a result may be NaN: written all the same)
    assert_overwritten(buffer, view)
    # parts that are documented as left alone must still hold the pre-fill
    buffer, view = banded((3, 4), np.float64, ALIGNED, SENTINEL)
    untouched = np.zeros((3, 4), dtype=bool)
    untouched[:, 3] = True
    view[:, :3] = 1.0
    assert_overwritten(buffer, view, untouched=untouched)
    view[1, 3] = 2.0
    with pytest.raises(AssertionError, match="documented as left alone"):
        assert_overwritten(buffer, view, untouched=untouched)
    view[1, 3] = np.array(prefill_bits(np.float64), dtype=np.int64).view(np.float64)
    view[0, 0] = view[0, 3]
    with pytest.raises(AssertionError, match="1 elements never written, the first at flat index 0"):
        assert_overwritten(buffer, view, untouched=untouched)


def test_bit_for_bit_comparison_tells_zeros_and_nans_apart():
    a = np.array([0.0, 1.0, np.nan])
    assert_same_bits(a, a.copy())
    with pytest.raises(AssertionError, match="1 of 3 elements differ"):
        assert_same_bits(np.array([-0.0, 1.0, np.nan]), a)
    with pytest.raises(AssertionError):
        assert_same_bits(a.astype(np.float32), a)


def test_host_results_of_a_module_are_banded_while_the_block_runs():
    with banded_host_results(spectrum, ODD) as results:
        out = spectrum.np.empty((2, 3, 5), dtype=np.float64)
        status = spectrum.np.empty(4, dtype=np.int32)
        zeros = spectrum.np.zeros((2, 2))
        assert spectrum.np.float64 is np.float64
    assert spectrum.np is np and len(results) == 2 and not zeros.any()
    assert out.shape == (2, 3, 5) and status.shape == (4,) and status.dtype == np.int32
    for (buffer, view), array in zip(results, (out, status)):
        assert np.shares_memory(view, array)
        assert_bands_intact(buffer, view)
        with pytest.raises(AssertionError, match="never written"):
            assert_overwritten(buffer, view)
    out[...] = 1.0
    assert_overwritten(*results[0])


# ----------------------------------------------------------------------------- the table
def test_every_device_entry_has_a_guard_band_case_or_is_exempt():
    """A later ``*_device`` entry without a case in tests/guard_band_cases.py fails here."""
    names = device_entry_names()
    assert len(names) == len(set(names)) and "rn_potgnn_forward_device" in names and "rn_bm_moments_device" in names
    for name in names:
        assert (name in ENTRIES) != (name in EXEMPT), f"{name}: one guard-band case in ENTRIES, or a reason in EXEMPT"
    assert sorted(list(ENTRIES) + list(EXEMPT)) == names, "the table names an entry the library does not have"


def test_the_table_is_filled_in():
    import tests.test_guard_bands_gpu as cases
    for name, entry in ENTRIES.items():
        assert entry.device, f"{name}: an entry without a device pointer belongs in EXEMPT"
        assert entry.access.startswith(("element-wide:", "wider, safe:", "refused:")), name
        assert callable(getattr(cases, entry.test, None)), f"{name}: tests/test_guard_bands_gpu.py has no {entry.test}"
        assert entry.bitwise or entry.repeat_bar, f"{name}: an entry without bit-identical repeats names its repeat bar"
    for name, reason in EXEMPT.items():
        assert "host memory" in reason, name


def test_every_case_names_the_entries_it_calls():
    """Each test of the GPU file passes the entries it covers to ``run_case``, which asserts that they were called:
    the table's ``test`` column must agree with that text."""
    import inspect

    import tests.test_guard_bands_gpu as cases
    source = inspect.getsource(cases)
    for name, entry in ENTRIES.items():
        assert f'"{name}"' in source, f"{name} is not named in tests/test_guard_bands_gpu.py"
        body = inspect.getsource(getattr(cases, entry.test))
        helpers = inspect.getsource(cases._measure_case)
        assert f'"{name}"' in body or f'"{name}"' in helpers, f"{entry.test} does not name {name}"
