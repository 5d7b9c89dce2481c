"""The status code and the ``rn_potgnn_last_error`` text of every public ``rn_potgnn_*`` entry for arguments it refuses
(or, for an empty batch, accepts without doing anything), against ``tests/golden/abi_errors.json``.

The golden file was recorded by running ``collect`` below on the library of the commit before the entries were moved
onto shared argument checks (csrc/api.hip: check_batch, check_train_batch, check_pending, check_types); the calls are
made in one fixed order because the text of the last error is handle state that a successful call leaves alone.  For a
call on a null handle only the code is compared: its text is the process-wide text of the last failed create, which
other tests write.  Every case returns before device work is queued.  Needs a real MI355X: run with ``-m gpu``.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN, load_golden
from tests.helpers import product_model_from_golden

pytestmark = pytest.mark.gpu

MAX_GROUPS = 16  # kMaxGroups of csrc/kernels.hpp
SENTINEL = -12345.0
REL = 1e-5  # test_gpu_parity's bar


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        return C.c_void_p(a.data_ptr())
    return C.c_void_p(a.ctypes.data)


def collect(lib, model):
    """Run every refused / empty call on ``model``'s handle; returns ([name, rc, text], ...) in call order."""
    h = model._ensure_handle()
    n, k, fe = model.num_atoms, model._num_atom_types, model._fe
    g = load_golden("triclinic20")
    rng = np.random.default_rng(7)
    dev = torch.device("cuda")

    def host(shape, dtype=np.float64):  # an output: sentinel-filled
        return np.full(shape, SENTINEL, dtype=dtype)

    def device(shape, dtype=torch.float64):
        return torch.full(shape, SENTINEL, dtype=dtype, device=dev)

    pos = np.ascontiguousarray(g["pos_batch"][:3], dtype=np.float64)  # 3 frames: one more than the chunk of 2
    lat = np.ascontiguousarray(np.broadcast_to(g["lattice"], (3, 3, 3)), dtype=np.float64)
    types = np.zeros((2, n), dtype=np.int32)
    disp = rng.standard_normal((2, n, 3))
    labels = (np.arange(n) % 2).astype(np.int32)
    dvec6 = np.ones((3, 6), dtype=np.float32)
    dvec6_64 = np.ones((3, 6), dtype=np.float64)
    weights = np.zeros(lib.rn_potgnn_weight_count(C.byref(_config(model))), dtype=np.float32)
    d_pos = torch.tensor(pos, device=dev)
    d_lat32 = torch.tensor(lat, device=dev, dtype=torch.float32)
    d_lat64 = torch.tensor(lat, device=dev)
    d_types = torch.zeros((3, n), dtype=torch.int32, device=dev)
    d_dvec6 = torch.ones((3, 6), dtype=torch.float32, device=dev)
    d_dvec6_64 = torch.ones((3, 6), dtype=torch.float64, device=dev)
    outs = {
        "alpha": host((3, 9)), "vec6": host((3, 6), np.float32), "vec6_64": host((3, 6)), "raman": host((2, 2, 9)),
        "jac": host((6, n, 3)), "mean": host(fe, np.float32), "var": host(fe, np.float32), "mean64": host(fe),
        "var64": host(fe), "grads": host(weights.size, np.float32), "grads64": host(weights.size), "dpos": host((3, n, 3)),
        "dlat": host((3, 9)), "wout": host(weights.size, np.float32),
        "d_alpha": device((3, 9)), "d_vec6": device((3, 6), torch.float32), "d_dpos": device((3, n, 3)),
        "d_dlat": device((3, 9)), "d_out": device((2, 2, 9)),
    }
    o = {key: _ptr(v) for key, v in outs.items()}
    P = {"pos": _ptr(pos), "lat": _ptr(lat), "types": _ptr(types), "disp": _ptr(disp), "labels": _ptr(labels),
         "dvec6": _ptr(dvec6), "dvec6_64": _ptr(dvec6_64), "weights": _ptr(weights), "d_pos": _ptr(d_pos),
         "d_lat32": _ptr(d_lat32), "d_lat64": _ptr(d_lat64), "d_types": _ptr(d_types), "d_dvec6": _ptr(d_dvec6),
         "d_dvec6_64": _ptr(d_dvec6_64)}

    def untouched():
        for key, v in outs.items():
            same = bool((v == SENTINEL).all())
            assert same, f"a refused or empty call wrote to {key}"

    log = []

    def call(name, fn, *args, handle=h, ok=False):
        rc = getattr(lib, fn)(handle, *args)
        text = lib.rn_potgnn_last_error(handle) if handle is not None else b""  # (process-wide without a handle: not compared)
        log.append([name, int(rc), text.decode() if text else ""])
        if ok:  # an empty batch: accepted, nothing touched
            assert rc == 0, name
            untouched()

    def sweep(fn, good, nulls, s_at=None, empty=True):
        """`good`: the argument list of an accepted call; each index of `nulls` set to None in turn; with `s_at`, the
        frame count at that index set to -1 and (``empty``) to 0; and a null handle."""
        call(f"{fn}/null handle", fn, *good, handle=None)
        for i in nulls:
            call(f"{fn}/null arg {i}", fn, *(None if j == i else a for j, a in enumerate(good)))
        if s_at is not None:
            call(f"{fn}/S=-1", fn, *(-1 if j == s_at else a for j, a in enumerate(good)))
            if empty:
                call(f"{fn}/S=0", fn, *(0 if j == s_at else a for j, a in enumerate(good)), ok=True)
                call(f"{fn}/S=0, every pointer null", fn, *(0 if j == s_at else (None if isinstance(a, C.c_void_p) else a)
                                                             for j, a in enumerate(good)), ok=True)

    # ---- evaluation entries (S >= 0)
    sweep("rn_potgnn_forward_device", [P["d_pos"], 2, o["d_alpha"], o["d_vec6"], None, 1], [0], s_at=1)
    sweep("rn_potgnn_forward_device_f64", [P["d_pos"], 2, o["d_alpha"], None, 1], [0, 2], s_at=1)
    sweep("rn_potgnn_calc_polarizabilities", [P["pos"], 2, o["alpha"]], [0, 2], s_at=1)
    sweep("rn_potgnn_calc_polarizabilities_f64", [P["pos"], 2, o["alpha"]], [0, 2], s_at=1)
    sweep("rn_potgnn_calc_polarizabilities_async", [P["pos"], 2, o["alpha"]], [0, 2], s_at=1)
    sweep("rn_potgnn_calc_polarizabilities_to_device", [P["pos"], 2, o["d_alpha"], None], [0, 2], s_at=1)
    sweep("rn_potgnn_forward", [P["pos"], 2, o["vec6"]], [0, 2], s_at=1)
    sweep("rn_potgnn_forward_lattices", [P["lat"], P["pos"], 2, o["vec6"]], [0, 1, 3], s_at=2)
    sweep("rn_potgnn_forward_samples", [P["lat"], P["types"], P["pos"], 2, o["vec6"]], [2, 4], s_at=3)
    sweep("rn_potgnn_forward_samples_f64", [P["lat"], P["types"], P["pos"], 2, o["vec6_64"]], [2, 4], s_at=3)
    sweep("rn_potgnn_forward_samples_device", [P["d_lat32"], P["d_types"], P["d_pos"], 2, o["d_vec6"], None, 1], [2, 4], s_at=3)
    sweep("rn_potgnn_forward_vjp_device", [P["d_lat64"], P["d_types"], P["d_pos"], 2, P["d_dvec6_64"], 0, o["d_dpos"], o["d_dlat"], None],
          [2, 4], s_at=3, empty=False)
    call("rn_potgnn_forward_vjp_device/neither dpos nor dlat", "rn_potgnn_forward_vjp_device", P["d_lat64"], P["d_types"], P["d_pos"], 2,
         P["d_dvec6_64"], 0, None, None, None)
    call("rn_potgnn_forward_vjp_device/S=0", "rn_potgnn_forward_vjp_device", None, None, None, 0, None, 1, o["d_dpos"], None, None, ok=True)
    call("rn_potgnn_forward_vjp_device/S=0, neither", "rn_potgnn_forward_vjp_device", None, None, None, 0, None, 1, None, None, None)
    call("rn_potgnn_wait/null handle", "rn_potgnn_wait", handle=None)

    # ---- an atom type outside [0, K) in the first and in the last position
    # (frames: 2, the chunk -- but 1 for the float64 training entry, whose chunk at a float32 chunk of 2 is one frame)
    for fn, frames, out, extra in (("rn_potgnn_forward_samples", 2, o["vec6"], []), ("rn_potgnn_forward_samples_f64", 2, o["vec6_64"], []),
                                   ("rn_potgnn_train_forward_samples", 2, o["vec6"], [o["mean"], o["var"]]),
                                   ("rn_potgnn_train_forward_samples_f64", 1, o["vec6_64"], [o["mean64"], o["var64"]])):
        for where, value in ((0, k), (frames * n - 1, -1)):
            bad = types.copy()
            bad.reshape(-1)[where] = value
            call(f"{fn}/atom type {value} at {where}", fn, P["lat"], _ptr(bad), P["pos"], frames, out, *extra)

    # ---- Raman tensors and the Jacobian
    sweep("rn_potgnn_raman_tensors", [P["pos"], P["disp"], 2, 0.01, o["raman"]], [0, 1, 4], s_at=2, empty=False)
    call("rn_potgnn_raman_tensors/delta=0", "rn_potgnn_raman_tensors", P["pos"], P["disp"], 2, 0.0, o["raman"])
    call("rn_potgnn_raman_tensors/M=0", "rn_potgnn_raman_tensors", P["pos"], None, 0, 0.01, None, ok=True)
    call("rn_potgnn_raman_tensors/M=0, no reference", "rn_potgnn_raman_tensors", None, None, 0, 0.01, None)
    sweep("rn_potgnn_raman_tensors_analytic", [P["pos"], P["disp"], 2, o["raman"]], [0, 1, 3], s_at=2, empty=False)
    call("rn_potgnn_raman_tensors_analytic/M=0", "rn_potgnn_raman_tensors_analytic", P["pos"], None, 0, None, ok=True)
    sweep("rn_potgnn_alpha_jacobian", [P["pos"], 0, o["jac"]], [0, 2])
    sweep("rn_potgnn_alpha_jacobian", [P["pos"], 1, o["jac"]], [0, 2])

    # ---- weights
    sweep("rn_potgnn_set_weights", [P["weights"], weights.size], [0])
    call("rn_potgnn_set_weights/wrong count", "rn_potgnn_set_weights", P["weights"], weights.size - 1)
    sweep("rn_potgnn_get_weights", [o["wout"], weights.size], [0])
    call("rn_potgnn_get_weights/wrong count", "rn_potgnn_get_weights", o["wout"], weights.size + 1)

    # ---- training: forward entries (a batch of 3 frames against the chunk of 2), backward entries with nothing pending
    t32, t64 = [o["vec6"], o["mean"], o["var"]], [o["vec6_64"], o["mean64"], o["var64"]]
    for fn, good, nulls, s_at in (
            ("rn_potgnn_train_forward", [P["pos"], 2, *t32], [0, 2, 3, 4], 1),
            ("rn_potgnn_train_forward_f64", [P["pos"], 2, *t64], [0, 2, 3, 4], 1),
            ("rn_potgnn_train_forward_samples", [P["lat"], P["types"], P["pos"], 2, *t32], [2, 4, 5, 6], 3),
            ("rn_potgnn_train_forward_samples_f64", [P["lat"], P["types"], P["pos"], 2, *t64], [2, 4, 5, 6], 3),
            ("rn_potgnn_train_forward_samples_device", [P["d_lat32"], P["d_types"], P["d_pos"], 2, o["d_vec6"], None], [2, 4], 3)):
        sweep(fn, good, nulls, s_at=s_at, empty=False)
        call(f"{fn}/S=0", fn, *(0 if j == s_at else a for j, a in enumerate(good)))
        call(f"{fn}/S=3", fn, *(3 if j == s_at else a for j, a in enumerate(good)))

    def backward_entries(tag):
        call(f"rn_potgnn_train_backward/{tag}", "rn_potgnn_train_backward", P["dvec6"], o["grads"])
        call(f"rn_potgnn_train_backward_f64/{tag}", "rn_potgnn_train_backward_f64", P["dvec6_64"], o["grads64"])
        call(f"rn_potgnn_train_backward_device/{tag}", "rn_potgnn_train_backward_device", P["dvec6"])
        call(f"rn_potgnn_train_backward_inputs/{tag}", "rn_potgnn_train_backward_inputs", P["dvec6"], o["grads"], o["dpos"], o["dlat"])
        call(f"rn_potgnn_train_backward_samples_device/{tag}", "rn_potgnn_train_backward_samples_device", P["d_dvec6"], None)
        call(f"rn_potgnn_train_backward_inputs_device/{tag}", "rn_potgnn_train_backward_inputs_device", P["d_dvec6"], o["d_dpos"], o["d_dlat"], None)

    sweep("rn_potgnn_train_backward", [P["dvec6"], o["grads"]], [0, 1])
    sweep("rn_potgnn_train_backward_f64", [P["dvec6_64"], o["grads64"]], [0, 1])
    sweep("rn_potgnn_train_backward_device", [P["dvec6"]], [0])
    sweep("rn_potgnn_train_backward_inputs", [P["dvec6"], o["grads"], o["dpos"], o["dlat"]], [0])
    call("rn_potgnn_train_backward_inputs/neither dpos nor dlat", "rn_potgnn_train_backward_inputs", P["dvec6"], o["grads"], None, None)
    sweep("rn_potgnn_train_backward_samples_device", [P["d_dvec6"], None], [0])
    sweep("rn_potgnn_train_backward_inputs_device", [P["d_dvec6"], o["d_dpos"], o["d_dlat"], None], [0])
    call("rn_potgnn_train_backward_inputs_device/neither", "rn_potgnn_train_backward_inputs_device", P["d_dvec6"], None, None, None)
    backward_entries("nothing pending, device training off")
    call("rn_potgnn_set_device_training/null handle", "rn_potgnn_set_device_training", 1, handle=None)
    call("rn_potgnn_set_device_training/on", "rn_potgnn_set_device_training", 1)
    backward_entries("nothing pending, device training on")
    call("rn_potgnn_train_forward_samples_device/S=3, device training on", "rn_potgnn_train_forward_samples_device",
         P["d_lat32"], P["d_types"], P["d_pos"], 3, o["d_vec6"], None)
    call("rn_potgnn_set_device_training/off", "rn_potgnn_set_device_training", 0)
    ptr, count = C.c_void_p(), C.c_size_t()
    call("rn_potgnn_gradient_buffer/no gradients", "rn_potgnn_gradient_buffer", C.byref(ptr), C.byref(count))
    call("rn_potgnn_gradient_buffer/null handle", "rn_potgnn_gradient_buffer", C.byref(ptr), C.byref(count), handle=None)
    adam = [1e-3, 0.9, 0.999, 1e-8, 0.0]
    call("rn_potgnn_adam_step/no gradients", "rn_potgnn_adam_step", *adam, 1)
    call("rn_potgnn_adam_step/step 0", "rn_potgnn_adam_step", *adam, 0)
    call("rn_potgnn_adam_step/negative lr", "rn_potgnn_adam_step", -1.0, *adam[1:], 1)
    call("rn_potgnn_adam_step/null handle", "rn_potgnn_adam_step", *adam, 1, handle=None)

    # ---- atom groups
    inc = [P["d_pos"], 3, P["labels"], 2, 0, 0, o["d_out"], None]
    sweep("rn_potgnn_group_increments_device", inc, [0, 2, 6])
    prt = [P["pos"], P["disp"], 2, P["labels"], 2, o["raman"]]
    sweep("rn_potgnn_partial_raman_tensors", prt, [0, 1, 3, 5], s_at=2, empty=False)
    out_of_range, empty_group = labels.copy(), np.zeros(n, dtype=np.int32)
    out_of_range[-1] = 2
    for fn, good, g_at, l_at in (("rn_potgnn_group_increments_device", inc, 3, 2), ("rn_potgnn_partial_raman_tensors", prt, 4, 3)):
        for groups in (0, MAX_GROUPS + 1):
            call(f"{fn}/G={groups}", fn, *(groups if j == g_at else a for j, a in enumerate(good)))
        call(f"{fn}/label out of range", fn, *(_ptr(out_of_range) if j == l_at else a for j, a in enumerate(good)))
        call(f"{fn}/empty group", fn, *(_ptr(empty_group) if j == l_at else a for j, a in enumerate(good)))
    call("rn_potgnn_group_increments_device/S=1", "rn_potgnn_group_increments_device", P["d_pos"], 1, *inc[2:])
    call("rn_potgnn_partial_raman_tensors/M=0", "rn_potgnn_partial_raman_tensors", P["pos"], None, 0, P["labels"], 2, None, ok=True)

    # ---- the small getters / setters and the debug entries
    call("rn_potgnn_set_stat_reducer/null handle", "rn_potgnn_set_stat_reducer", None, None, handle=None)
    call("rn_potgnn_set_profiling/null handle", "rn_potgnn_set_profiling", 0, handle=None)
    call("rn_potgnn_config_flags/null handle", "rn_potgnn_config_flags", handle=None)
    call("rn_potgnn_num_triplets/null handle", "rn_potgnn_num_triplets", handle=None)
    rows, cols = C.c_int64(), C.c_int64()
    stage_out = np.zeros(16, dtype=np.float32)
    call("rn_potgnn_debug_stage/null handle", "rn_potgnn_debug_stage", 0, 0, _ptr(stage_out), 16, C.byref(rows), C.byref(cols), handle=None)
    call("rn_potgnn_debug_stage/null out", "rn_potgnn_debug_stage", 0, 0, None, 16, C.byref(rows), C.byref(cols))
    call("rn_potgnn_debug_triplets/null arg", "rn_potgnn_debug_triplets", None, None, None, None, None)
    call("rn_potgnn_kernel_times/null arg", "rn_potgnn_kernel_times", None, None, None, 0)
    log.append(["rn_potgnn_train_row_count/null handle", int(lib.rn_potgnn_train_row_count(None)), ""])
    untouched()
    return log


def _config(model):
    from ramannoodle_amd import _lib
    return _lib.Config(model.num_atoms, model.num_edges, model._num_atom_types, model._fn, model._fe, model._passes,
                       model._gauss_coefficient, 2, 0)


def test_refused_and_empty_calls_keep_their_codes_and_texts():
    from ramannoodle_amd import _lib
    g = load_golden("triclinic20")
    model = product_model_from_golden(g, max_chunk_structures=2)
    log = collect(_lib.load(), model)
    with open(os.path.join(GOLDEN, "abi_errors.json")) as f:
        want = json.load(f)
    assert [c[0] for c in log] == [c[0] for c in want]
    for got, exp in zip(log, want):
        print(got)
        assert got == exp
    # the refused calls left the handle usable
    pos = g["pos_batch"]
    alpha = model.calc_polarizabilities(pos)
    std_part, ref_part = (alpha - g["mean"]) / g["std"], (g["f32/alpha"] - g["mean"]) / g["std"]
    assert np.abs(std_part - ref_part).max() / max(np.abs(ref_part).max(), 1e-30) < REL
