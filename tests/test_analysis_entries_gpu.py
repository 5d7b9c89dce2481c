"""The device workspaces of the five analysis modules (csrc/entry_runtime.hpp) across calls of one process: a small
call, a larger one that makes every buffer grow and crosses a tile or workgroup boundary of the kernel, then the small
call again into buffers that are now larger than it needs.  All five modules sum without atomics and document
repeatable results, so the third result equals the first bit for bit; anything else is a stale size, a stale pointer or
a stale value left in the workspace.  Shapes: tests/analysis_entries_cases.py.  Needs a real MI355X: run with ``-m gpu``."""
import ctypes as C

import numpy as np
import pytest
import torch

from ramannoodle_amd import _lib, harmonic
from tests.analysis_entries_cases import CALLS, ht_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_default_device_mode():
    torch.set_default_device(None)
    yield


@pytest.mark.parametrize("module", CALLS)
def test_a_small_call_after_a_larger_one_repeats_its_bits(module):
    small, larger = CALLS[module]["small"], CALLS[module]["larger"]
    first = {entry: call() for entry, call in small.items()}
    grown = {entry: call() for entry, call in larger.items()}
    again = {entry: call() for entry, call in small.items()}
    for entry in small:
        assert len(first[entry]) == len(again[entry]) > 0
        for before, after in zip(first[entry], again[entry]):
            assert np.isfinite(before).any()
            np.testing.assert_array_equal(after, before)  # (NaN, the outputs of a degenerate window, equals NaN here)
    # the host entry and the device entry run the same kernels on the same values
    for results in (first, grown):
        for from_host, from_device in zip(results["host"], results["device"]):
            np.testing.assert_array_equal(from_device, from_host)


def _phase_times():
    times = np.full(3, -1.0)
    assert _lib.load().rn_ht_phase_times(C.c_void_p(times.ctypes.data)) == _lib.RN_OK
    return times


def test_the_harmonic_entries_with_profiling_on_and_off():
    """Profiling changes when the device entry waits, not what it writes; the phases are the copies to the device, the
    kernel and the copy to the host, which only the host entry makes."""
    lib = _lib.load()
    inputs, frames = ht_inputs("larger")
    plain = harmonic.synthesize_device(*inputs, frames, device=0).cpu().numpy()
    assert not _phase_times().any()
    assert lib.rn_ht_set_profiling(1) == _lib.RN_OK
    try:
        timed = harmonic.synthesize_device(*inputs, frames, device=0).cpu().numpy()
        device_times = _phase_times()
        downloaded = harmonic.synthesize_download(*inputs, frames, device=0)
        host_times = _phase_times()
    finally:
        assert lib.rn_ht_set_profiling(0) == _lib.RN_OK
    np.testing.assert_array_equal(timed, plain)
    np.testing.assert_array_equal(downloaded, plain)
    print("device entry:", device_times, "host entry:", host_times)
    assert device_times[1] > 0 and device_times[2] == 0
    assert host_times[1] > 0 and host_times[2] > 0
    assert not _phase_times().any()  # switching it off clears them
