"""``rn_potgnn_config_flags`` over a small matrix of models and knobs, against ``tests/golden/config_flags.json``, and
the tie between what it reports and what runs.

The flags and the run read one policy (csrc/forward.hip: ``choose``); the golden file was recorded by running
``collect`` below on the library of the commit before that, where the entry derived bits 8-11 on its own.  Models: the
20-atom ``triclinic20`` fixture (narrow kernels: bit 3) and ``hub17`` at Fn = Fe = 64 (the smallest wide graph of
tests/test_c2_pairs_gpu.py and tests/test_node_side_gpu.py: bits 8-11 can be set).  Every combination is read right after
create and again after a ``set_weights`` that trips the split-f16 range guard (the scale of
tests/test_gpu_parity.py::test_split_f16_range_guard_falls_back_to_float32).  ``RN_POTGNN_NODE_CENTRED`` is read once per
process and is not varied.  Needs a real MI355X: run with ``-m gpu``.
"""
import contextlib
import json
import os

import pytest

from tests.conftest import GOLDEN, load_golden
from tests.helpers import product_model_from_golden, sparse_fixture
from tests.test_gpu_parity import _random_model

pytestmark = pytest.mark.gpu

KNOBS = (
    ("default", {}),
    ("fused=0", {"RN_POTGNN_FUSED": "0"}),
    ("edge_ps=0", {"RN_POTGNN_EDGE_PS": "0"}),
    ("node_atom=0", {"RN_POTGNN_NODE_ATOM": "0"}),
    ("node_atom=1", {"RN_POTGNN_NODE_ATOM": "1"}),
    ("pair_rows=0", {"RN_POTGNN_PAIR_ROWS": "0"}),
    ("c2_pairs=0", {"RN_POTGNN_C2_PAIRS": "0"}),
    ("mfma=f32", {"RN_POTGNN_MFMA": "f32"}),
    ("keep_stages=1", {"RN_POTGNN_KEEP_STAGES": "1"}),
    ("keep_stages=2", {"RN_POTGNN_KEEP_STAGES": "2"}),
    # on hub17 only the atom-owning NodeBlock sets bits 9-11: with it, each knob that takes pair rows or the pair kernel away
    ("node_atom=1,pair_rows=0", {"RN_POTGNN_NODE_ATOM": "1", "RN_POTGNN_PAIR_ROWS": "0"}),
    ("node_atom=1,c2_pairs=0", {"RN_POTGNN_NODE_ATOM": "1", "RN_POTGNN_C2_PAIRS": "0"}),
    ("node_atom=1,keep_stages=1", {"RN_POTGNN_NODE_ATOM": "1", "RN_POTGNN_KEEP_STAGES": "1"}),
    ("node_atom=1,keep_stages=2", {"RN_POTGNN_NODE_ATOM": "1", "RN_POTGNN_KEEP_STAGES": "2"}),
    ("node_atom=1,mfma=f32", {"RN_POTGNN_NODE_ATOM": "1", "RN_POTGNN_MFMA": "f32"}),
)
VARIED = sorted({k for _, env in KNOBS for k in env})
RANGE_GUARD_SCALE = 3.0e3  # on the readout's first layer: |h1| may then leave f16's range
C2_PAIRS_BIT = 2048


def _narrow():
    return product_model_from_golden(load_golden("triclinic20"))


def _wide():
    g, cutoff = sparse_fixture("hub17", frames=2)
    return _random_model(g, cutoff, 64, 64, 2, seed=64064)[0]


MODELS = (("triclinic20", _narrow), ("hub17_64x64", _wide))


@contextlib.contextmanager
def _environment(env):
    """The varied knobs set to ``env`` and nothing else (a handle reads them when it is created); restored on exit."""
    saved = {k: os.environ.pop(k, None) for k in VARIED}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _raw_flags(model):
    from ramannoodle_amd import _lib
    return int(_lib.load().rn_potgnn_config_flags(model._ensure_handle()))


def collect():
    """{"model/knob": [flags after create, flags after the range guard tripped]} over MODELS x KNOBS, in one process."""
    out = {}
    for model_name, build in MODELS:
        for knob_name, env in KNOBS:
            with _environment(env):
                model = build()
                created = _raw_flags(model)
                state = model.state_dict()
                state["_to_polarizability_embedding.0.weight"].mul_(RANGE_GUARD_SCALE)
                model.load_state_dict(state)
                out[f"{model_name}/{knob_name}"] = [created, _raw_flags(model)]
    return out


def test_flags_match_the_recorded_matrix():
    got = collect()
    with open(os.path.join(GOLDEN, "config_flags.json")) as f:
        want = json.load(f)
    assert got == want, {key: (got.get(key), want.get(key)) for key in set(got) | set(want) if got.get(key) != want.get(key)}


@pytest.mark.parametrize("knob_name, env", KNOBS, ids=[k for k, _ in KNOBS])
def test_the_pair_kernel_runs_exactly_when_bit_11_says_so(knob_name, env):
    """Wide model, every launch timed, one evaluation of two frames: ``c2_pairs`` launches if and only if bit 11 is set."""
    with _environment(env):
        model = _wide()
        flags = _raw_flags(model)
        model.set_profiling(1)
        model.calc_polarizabilities(sparse_fixture("hub17", frames=2)[0]["pos_batch"])
        launches = model.kernel_times()["c2_pairs"][1]
        model.set_profiling(0)
    assert (launches > 0) == bool(flags & C2_PAIRS_BIT), (knob_name, flags, launches)
