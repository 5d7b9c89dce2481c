"""What the entries of the five analysis modules (line-shape fits, multi-peak fits, covariance moments, harmonic
trajectories, band moments) share on the host: the device check, and an error text per module and per thread.  No test
here needs a GPU: every call is refused before it allocates or launches."""
import ctypes as C
import itertools
import threading

import numpy as np
import pytest

from ramannoodle_amd import _lib

NO_SUCH_DEVICE = 4096


def _pointers(arrays):
    return {name: C.c_void_p(array.ctypes.data) for name, array in arrays.items()}


def _fit_arrays(peaks=2):
    """Two fits on two rows of 64 bins: the table of the refusal tests of test_lineshape.py and test_peakfit.py."""
    return {"rows": np.ones((2, 64)), "row_index": np.array([0, 1], dtype=np.int64),
            "first_bin": np.array([10, 10], dtype=np.int64), "num_bins": np.array([33, 33], dtype=np.int64),
            "origin": np.full(2, 100.0), "centres": np.tile([11.0, 22.0], (2, 1)), "widths": np.full((2, peaks), 2.0),
            "out": np.zeros((2, 32)), "status": np.zeros(2, dtype=np.int32), "iterations": np.zeros(2, dtype=np.int32)}


def _lineshape(device, on_device, max_iterations=400):
    arrays = _fit_arrays()
    p = _pointers(arrays)
    entry, tail = ("rn_lineshape_fit_device", (C.c_void_p(None),)) if on_device else ("rn_lineshape_fit", ())
    return getattr(_lib.load(), entry)(device, p["rows"], 2, 64, p["row_index"], p["first_bin"], p["num_bins"], 2,
                                       max_iterations, p["out"], p["status"], p["iterations"], *tail)


def _peakfit(device, on_device, peaks=2):
    arrays = _fit_arrays()
    p = _pointers(arrays)
    entry, tail = ("rn_peakfit_fit_device", (C.c_void_p(None),)) if on_device else ("rn_peakfit_fit", ())
    return getattr(_lib.load(), entry)(device, p["rows"], 2, 64, p["row_index"], p["first_bin"], p["num_bins"], 2, 0, 0,
                                       peaks, p["origin"], p["centres"], p["widths"], 400, p["out"], p["status"],
                                       p["iterations"], *tail)


def _qh(device, on_device, atoms=2):
    """6 frames of 2 atoms in two blocks (test_quasiharmonic.py)."""
    arrays = {"pos": np.full((6, 6), 0.25), "anchor": np.full(6, 0.25), "bounds": np.array([0, 2, 6], dtype=np.int64),
              "joined": np.array([1, 0], dtype=np.int32), "first": np.zeros((2, 6)), "second": np.zeros((2, 2, 6, 6)),
              "counts": np.zeros((2, 2), dtype=np.int64)}
    p = _pointers(arrays)
    entry, tail = ("rn_qh_moments_device", (C.c_void_p(None),)) if on_device else ("rn_qh_moments", ())
    return getattr(_lib.load(), entry)(device, p["pos"], 6, atoms, p["anchor"], p["bounds"], p["joined"], 2, p["first"],
                                       p["second"], p["counts"], *tail)


def _ht(device, on_device, modes=3):
    """2 runs of 4 frames of 2 atoms and 3 modes (test_harmonic_trajectory.py)."""
    arrays = {"ref": np.full(6, 0.25), "D": np.full((3, 6), 0.01), "omega_dt": np.full(3, 0.1), "amp": np.full((2, 3), 0.5),
              "phase": np.full((2, 3), 1.0), "out": np.zeros((2, 4, 6))}
    p = _pointers(arrays)
    entry, tail = ("rn_ht_synthesize_device", (C.c_void_p(None),)) if on_device else ("rn_ht_synthesize", ())
    return getattr(_lib.load(), entry)(device, p["ref"], p["D"], p["omega_dt"], p["amp"], p["phase"], 2, modes, 2, 4, 0,
                                       p["out"], *tail)


def _bm(device, on_device, rows=1):
    """8 frames of 2 atoms, two segments of 6 frames, one row of weights 1 (test_band_modes.py)."""
    arrays = {"pos": np.full((8, 2, 3), 0.25), "lattice": np.eye(3), "masses": np.ones(2),
              "starts": np.array([0, 2], dtype=np.int64), "taper": np.ones(5), "weights": np.ones((1, 2)),
              "moments": np.zeros((1, 6, 6))}
    p = _pointers(arrays)
    entry, tail = ("rn_bm_moments_device", (C.c_void_p(None),)) if on_device else ("rn_bm_moments", ())
    return getattr(_lib.load(), entry)(device, p["pos"], p["lattice"], 8, 2, p["masses"], C.c_void_p(None), 6, p["starts"],
                                       2, p["taper"], p["weights"], rows, 2, 0, p["moments"], *tail)


# module -> (its call, its last_error, two refusals: the keyword that makes the call invalid and the text it leaves)
MODULES = {
    "lineshape": (_lineshape, "rn_lineshape_last_error",
                  [(dict(max_iterations=0), "max_iterations = 0"), (dict(max_iterations=-7), "max_iterations = -7")]),
    "peakfit": (_peakfit, "rn_peakfit_last_error", [(dict(peaks=0), "P = 0 peaks"), (dict(peaks=5), "P = 5 peaks")]),
    "qh": (_qh, "rn_qh_last_error", [(dict(atoms=0), "N = 0 atoms"), (dict(atoms=-1), "N = -1 atoms")]),
    "ht": (_ht, "rn_ht_last_error", [(dict(modes=0), "M = 0 modes"), (dict(modes=-4), "M = -4 modes")]),
    "bm": (_bm, "rn_bm_last_error", [(dict(rows=0), "B = 0 weight rows"), (dict(rows=-2), "B = -2 weight rows")]),
}


def _last_error(module):
    return getattr(_lib.load(), MODULES[module][1])().decode()


def _refuse(module, which=0):
    call, _, refusals = MODULES[module]
    arguments, text = refusals[which]
    assert call(0, False, **arguments) == _lib.RN_ERR_INVALID_ARGUMENT, (module, arguments)
    assert text in _last_error(module), (module, _last_error(module))
    return text


@pytest.mark.parametrize("on_device", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("module", MODULES)
def test_a_device_out_of_range_is_refused_by_every_entry(module, on_device):
    """A valid call with work to do: the device check is the first thing that can refuse it, and it does so before
    anything is allocated or launched (the ``_device`` entries are handed host memory here, and never read it)."""
    assert MODULES[module][0](NO_SUCH_DEVICE, on_device) == _lib.RN_ERR_NO_DEVICE
    assert f"device {NO_SUCH_DEVICE} is not one of the" in _last_error(module)


@pytest.mark.parametrize("first, second", list(itertools.permutations(MODULES, 2)))
def test_the_error_texts_of_two_modules_stay_apart(first, second):
    text = _refuse(first)
    other = _refuse(second)
    assert text in _last_error(first) and other not in _last_error(first)


@pytest.mark.parametrize("module", MODULES)
def test_the_error_text_is_per_thread(module):
    text = _refuse(module, 0)
    seen = []

    def elsewhere():
        seen.append(_last_error(module))  # a new thread starts with no text
        seen.append(_refuse(module, 1))
        seen.append(_last_error(module))

    thread = threading.Thread(target=elsewhere)
    thread.start()
    thread.join()
    assert len(seen) == 3, "the refusal on the second thread did not go as expected"
    assert seen[0] == "" and seen[1] in seen[2]
    assert text in _last_error(module) and seen[1] not in _last_error(module)


def test_the_harmonic_phase_times_are_three_doubles():
    """``millis[3]`` of rn_harmonic.h: a fourth double behind them belongs to the caller."""
    lib = _lib.load()
    times = np.full(4, -7.5)
    assert lib.rn_ht_set_profiling(0) == _lib.RN_OK
    assert lib.rn_ht_phase_times(C.c_void_p(times.ctypes.data)) == _lib.RN_OK
    assert times.tolist() == [0.0, 0.0, 0.0, -7.5]
