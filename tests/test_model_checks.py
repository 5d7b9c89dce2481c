"""Every refusal of ``PotGNN`` and ``InterpolationModel`` that needs no device, against
``tests/golden/model_refusals.json``: the exception type of every case and its text.

The golden file was recorded by running ``collect`` below (``python -m tests.test_model_checks``) on the commit before
the two models were moved onto one set of checks (``ramannoodle_amd/pmodel/_device.py``).  ``NEW_TEXT`` lists the cases
whose text changed on purpose with that move, and their new text: PotGNN's increments entries took the wording of the
interpolation model's, and the interpolation model's mode vectors took PotGNN's acceptance rule (any array-protocol
object numpy turns into a real ``(M,N,3)`` array).

No case reaches the library: a device tensor is stood in for by ``on_device``, a host tensor that answers ``is_cuda``
and ``device`` as a CUDA tensor would -- the checks read nothing else that differs.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN, load_golden
from tests.helpers import product_model_from_golden
from tests.interp_cases import fixture, seeded_case

GOLDEN_FILE = os.path.join(GOLDEN, "model_refusals.json")

NEW_TEXT = {
    "potgnn/group_increments_device/positions: one frame": "group increments needs at least 2 frame(s), not 1",
    "potgnn/mode_increments_device/positions: one frame": "mode increments needs at least 2 frame(s), not 1",
    "potgnn/group_increments_device/out: on the CPU": "out lives on cpu, the result is written on cuda:0",
    "potgnn/mode_increments_device/out: on the CPU": "out lives on cpu, the result is written on cuda:0",
    "potgnn/group_increments_device/out: wrong shape": "out has shape (2, 3, 3), the result is (3, 2, 3, 3)",
    "potgnn/mode_increments_device/out: wrong shape": "out has shape (3, 3, 3), the result is (3, 3, 3, 3)",
    "interp/mode_increments_device/displacements: an __array__ object, then a bad out":
        "out must be a torch.Tensor, not ndarray",
}


class _OnDevice(torch.Tensor):
    is_cuda = True
    device = torch.device("cuda", 0)


class _OnOtherDevice(torch.Tensor):
    is_cuda = True
    device = torch.device("cuda", 1)


def on_device(tensor, cls=_OnDevice):
    return torch.Tensor._make_subclass(cls, tensor)  # pylint: disable=protected-access


class ArrayObject:  # pylint: disable=too-few-public-methods
    """Not an ndarray, list or tuple, but numpy turns it into one."""

    def __init__(self, array):
        self._array = array

    def __array__(self, dtype=None, copy=None):
        return self._array if dtype is None else self._array.astype(dtype)


def _models():
    pot = product_model_from_golden(load_golden("triclinic20"))
    interp = fixture("interp_p1_small")[0].model()
    skew = seeded_case(3, 5, 4, symmetric=False).model()
    return pot, interp, skew


def _shared_cases(tag, model):  # pylint: disable=too-many-locals
    """The cases both models have.  (One call per model: the lambdas close over this call's names.)"""
    cases = []
    n = model.num_atoms
    good = on_device(torch.zeros((4, n, 3), dtype=torch.float64))
    labels = np.arange(n) % 2
    modes = np.ones((2, n, 3))
    entries = {
        "polarizabilities_device": (lambda p, m=model, **kw: m.calc_polarizabilities_device(p, **kw), (4, 3, 3)),
        "group_increments_device": (lambda p, m=model, **kw: m.calc_group_increments_device(p, labels, **kw),
                                    (3, 2, 3, 3)),
        "mode_increments_device": (lambda p, m=model, **kw: m.calc_mode_increments_device(p, modes, modes, **kw),
                                   (3, 3, 3, 3)),
    }
    if tag == "interp":
        entries["jacobian_device"] = (lambda p, m=model, **kw: m.calc_jacobian_device(p, **kw), (4, 6, n, 3))
    for entry, (call, shape) in entries.items():
        few = 1 if "increments" in entry else 0
        positions = {
            "not a tensor": np.zeros((4, n, 3)),
            "on the CPU": torch.zeros((4, n, 3), dtype=torch.float64),
            "float32": on_device(torch.zeros((4, n, 3), dtype=torch.float32)),
            "not contiguous": on_device(torch.zeros((4, 3, n), dtype=torch.float64).transpose(1, 2)),
            "wrong shape": on_device(torch.zeros((4, n + 1, 3), dtype=torch.float64)),
            "another device": on_device(torch.zeros((4, n, 3), dtype=torch.float64), _OnOtherDevice),
            ("one frame" if few else "no frame"): on_device(torch.zeros((few, n, 3), dtype=torch.float64)),
        }
        if tag == "potgnn":  # (PotGNN does not compare the devices, and its evaluation takes an empty batch)
            del positions["another device"]
            if not few:
                del positions["no frame"]
        for what, value in positions.items():
            cases.append((f"{tag}/{entry}/positions: {what}", lambda call=call, value=value: call(value)))
        wide = torch.zeros(shape[:-1] + (6,), dtype=torch.float64)
        outs = {
            "not a tensor": np.zeros(shape),
            "on the CPU": torch.zeros(shape, dtype=torch.float64),
            "float32": on_device(torch.zeros(shape, dtype=torch.float32)),
            "wrong shape": on_device(torch.zeros(shape[1:], dtype=torch.float64)),
            "not contiguous": on_device(wide[..., ::2]),
        }
        for what, value in outs.items():
            cases.append((f"{tag}/{entry}/out: {what}", lambda call=call, value=value: call(good, out=value)))

    def mode_call(disp, proj, m=model, good=good, **kw):
        return m.calc_mode_increments_device(good, disp, proj, **kw)

    bad = modes.copy()
    bad[1, 0, 2] = np.inf
    vectors = {
        "None": None, "a str": "modes", "a torch tensor": torch.ones((2, n, 3), dtype=torch.float64),
        "complex": modes.astype(np.complex128), "non-finite": bad, "wrong shape": np.ones((2, n + 1, 3)),
        "no mode": np.ones((0, n, 3)),
    }
    for what, value in vectors.items():
        cases.append((f"{tag}/mode_increments_device/displacements: {what}",
                      lambda call=mode_call, value=value: call(value, modes)))
        cases.append((f"{tag}/mode_increments_device/projectors: {what}",
                      lambda call=mode_call, value=value: call(modes, value)))
    cases.append((f"{tag}/mode_increments_device/displacements and projectors differ",
                  lambda call=mode_call: call(modes, np.ones((3, n, 3)))))
    cases.append((f"{tag}/mode_increments_device/displacements: an __array__ object, then a bad out",
                  lambda call=mode_call: call(ArrayObject(modes), modes, out=np.zeros((3, 3, 3, 3)))))
    cases.append((f"{tag}/group_increments_device/groups: a float array",
                  lambda m=model, good=good: m.calc_group_increments_device(good, np.zeros(m.num_atoms))))

    ref, disp = np.zeros((n, 3)), np.ones((2, n, 3))
    raman = {
        "ref_positions: wrong shape": lambda m=model: m.calc_raman_tensors(np.zeros((n + 1, 3)), disp),
        "displacements: wrong shape": lambda m=model: m.calc_raman_tensors(ref, np.ones((2, n, 2))),
        "displacements: not an array": lambda m=model: m.calc_raman_tensors(ref, [[0.0] * 3] * n),
        "unknown method": lambda m=model: m.calc_raman_tensors(ref, disp, method="exact"),
        "delta of 0": lambda m=model: m.calc_raman_tensors(ref, disp, delta=0.0),
        "delta of nan": lambda m=model: m.calc_raman_tensors(ref, disp, delta=float("nan")),
        "delta of inf": lambda m=model: m.calc_raman_tensors(ref, disp, delta=float("inf")),
        "partial, ref_positions: wrong shape":
            lambda m=model: m.calc_partial_raman_tensors(np.zeros((n, 2)), disp, labels),
        "partial, displacements: wrong shape":
            lambda m=model: m.calc_partial_raman_tensors(ref, np.ones((n, 3)), labels),
        "partial, groups: unknown": lambda m=model: m.calc_partial_raman_tensors(ref, disp, "elements"),
    }
    for what, call in raman.items():
        cases.append((f"{tag}/raman_tensors/{what}", call))
    for entry in ("calc_group_increments", "calc_mode_increments"):
        args = (labels,) if "group" in entry else (modes, modes)
        cases.append((f"{tag}/{entry}/positions_ts: wrong shape",
                      lambda m=model, entry=entry, args=args: getattr(m, entry)(np.zeros((4, n, 2)), *args)))
    return cases


def _potgnn_cases(pot):
    cases = []
    n = pot.num_atoms
    good = on_device(torch.zeros((4, n, 3), dtype=torch.float64))
    labels, modes = np.arange(n) % 2, np.ones((2, n, 3))
    cases.append(("potgnn/raman_tensors/an unexpected keyword",
                  lambda: pot._check_raman_arguments(np.zeros((n, 3)), modes, bogus=1)))  # pylint: disable=protected-access
    lattices = {
        "on the CPU": torch.zeros((4, 3, 3), dtype=torch.float64),
        "wrong shape": on_device(torch.zeros((3, 3, 3), dtype=torch.float64)),
    }
    for what, value in lattices.items():
        cases.append((f"potgnn/group_increments_device/lattices: {what}",
                      lambda value=value: pot.calc_group_increments_device(good, labels, lattices=value)))
        cases.append((f"potgnn/mode_increments_device/lattices: {what}",
                      lambda value=value: pot.calc_mode_increments_device(good, modes, modes, lattices=value)))
    cases.append(("potgnn/group_increments_device/lattices: sixteen groups and the cell",
                  lambda: pot.calc_group_increments_device(good, np.arange(n) % 16,
                                                           lattices=on_device(torch.zeros((4, 3, 3), dtype=torch.float64)))))
    singular = np.broadcast_to(np.eye(3), (4, 3, 3)).copy()
    singular[2, 1] = singular[2, 0]
    cases.append(("potgnn/calc_group_increments/lattices: singular",
                  lambda: pot.calc_group_increments(np.zeros((4, n, 3)), labels, lattices=singular)))
    cases.append(("potgnn/calc_mode_increments/lattices: wrong shape",
                  lambda: pot.calc_mode_increments(np.zeros((4, n, 3)), modes, modes, lattices=np.zeros((3, 3, 3)))))
    return cases


def _interp_cases(interp, skew):
    cases = []
    n = interp.num_atoms
    good = on_device(torch.zeros((4, n, 3), dtype=torch.float64))
    labels, modes, cells = np.arange(n) % 2, np.ones((2, n, 3)), np.zeros((4, 3, 3))
    given = {
        "calc_polarizabilities": lambda: interp.calc_polarizabilities(np.zeros((4, n, 3)), lattices=cells),
        "calc_polarizabilities_device": lambda: interp.calc_polarizabilities_device(good, lattices=cells),
        "calc_group_increments_device": lambda: interp.calc_group_increments_device(good, labels, lattices=cells),
        "calc_group_increments": lambda: interp.calc_group_increments(np.zeros((4, n, 3)), labels, lattices=cells),
        "calc_mode_increments_device": lambda: interp.calc_mode_increments_device(good, modes, modes, lattices=cells),
        "calc_mode_increments": lambda: interp.calc_mode_increments(np.zeros((4, n, 3)), modes, modes, lattices=cells),
    }
    for entry, call in given.items():
        cases.append((f"interp/{entry}/lattices given", call))

    n = skew.num_atoms
    good = on_device(torch.zeros((4, n, 3), dtype=torch.float64))
    labels, modes, ref = np.arange(n) % 2, np.ones((2, n, 3)), np.zeros((n, 3))
    asymmetric = {
        "calc_jacobian_device": lambda: skew.calc_jacobian_device(good),
        "calc_group_increments_device": lambda: skew.calc_group_increments_device(good, labels),
        "calc_mode_increments_device": lambda: skew.calc_mode_increments_device(good, modes, modes),
        "calc_partial_raman_tensors": lambda: skew.calc_partial_raman_tensors(ref, modes, labels),
        "calc_raman_tensors, analytic": lambda: skew.calc_raman_tensors(ref, modes, method="analytic"),
    }
    for entry, call in asymmetric.items():
        cases.append((f"interp/{entry}/asymmetric tables", call))
    return cases


def _cases(pot, interp, skew):
    """``(name, call)``: every ``call()`` raises before anything reaches the library."""
    return _shared_cases("potgnn", pot) + _shared_cases("interp", interp) + _potgnn_cases(pot) + _interp_cases(interp, skew)


def collect():
    """``{name: [exception type, text]}`` of every case (``["none", ""]`` for a call that returns)."""
    found = {}
    for name, call in _cases(*_models()):
        assert name not in found, name
        try:
            call()
            found[name] = ["none", ""]
        except Exception as exc:  # pylint: disable=broad-except
            found[name] = [type(exc).__name__, str(exc)]
    return found


@pytest.fixture(scope="module")
def refusals():
    with open(GOLDEN_FILE, encoding="utf-8") as handle:
        return collect(), json.load(handle)


def test_the_cases_are_the_recorded_ones(refusals):
    found, golden = refusals
    assert sorted(found) == sorted(golden)
    assert set(NEW_TEXT) <= set(golden)
    assert "none" not in {kind for kind, _ in golden.values()}  # (every case is a refusal)


def test_exception_types_match_the_record(refusals):
    found, golden = refusals
    differ = {name: (found[name][0], golden[name][0]) for name in golden if found[name][0] != golden[name][0]}
    assert not differ


def test_texts_match_the_record(refusals):
    found, golden = refusals
    differ = {name: (found[name][1], golden[name][1]) for name in golden
              if name not in NEW_TEXT and found[name][1] != golden[name][1]}
    assert not differ


@pytest.mark.parametrize("name", sorted(NEW_TEXT))
def test_deliberate_differences_have_their_new_text(refusals, name):
    found, golden = refusals
    assert found[name] == ["ValueError", NEW_TEXT[name]]
    assert golden[name][0] == "ValueError" and golden[name][1] != NEW_TEXT[name]


def test_mode_arrays_takes_array_protocol_objects():
    """The widening itself: what numpy turns into a real ``(M,N,3)`` array passes, for both models."""
    from ramannoodle_amd.pmodel._device import mode_arrays
    modes = np.arange(24.0).reshape(2, 4, 3)
    disp, proj = mode_arrays(ArrayObject(modes), ArrayObject(modes.astype(np.int64)), 4)
    assert disp.dtype == proj.dtype == np.float64 and disp.flags.c_contiguous
    assert np.array_equal(disp, modes) and np.array_equal(proj, modes)
    with pytest.raises(ValueError, match="must hold real numbers"):
        mode_arrays(ArrayObject(modes.astype(np.complex128)), modes, 4)


if __name__ == "__main__":
    with open(GOLDEN_FILE, "w", encoding="utf-8") as out:
        json.dump(collect(), out, indent=1, sort_keys=True)
        out.write("\n")
