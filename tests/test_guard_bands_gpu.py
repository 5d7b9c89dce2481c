"""Every device-pointer entry on contiguous views inside guarded buffers (tests/guard_bands.py, tests/guard_band_cases.py).

Per case: the plain call on tensors that own their allocations gives ``R0``, which is compared with the host statement of
the entry at the tolerance the entry's own GPU test uses; then, for a view that starts 4096 elements into a buffer (torch's
512-byte alignment) and for one that starts 4097 elements in (aligned to its element only), every device input and every
device or host output lies between guard bands: NaN around the inputs, a sentinel around the outputs, whose interior is
pre-filled with a second sentinel.  The banded result must equal ``R0`` bit for bit (at the entry's own repeat bar where
its header documents atomics: ``guard_band_cases.ENTRIES[...].bitwise``), no band may change, and every element of every
output must have been written, or hold the pre-fill where the header says it is left alone.

Shapes: the smallest of the existing case modules at which every tiled dimension has more than one tile and a partial
last one.  Tolerances are imported where the existing test names them; where it writes a literal, the constant here
cites the test.  Needs a real MI355X: run with ``-m gpu``."""
import contextlib
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

from ramannoodle_amd import _lib, bandmodes, harmonic, lineshape, peakfit, quasiharmonic, replicates, spectrum
from tests.conftest import load_golden
from tests.guard_band_cases import ENTRIES
from tests.guard_bands import (LEADS, NAN, SENTINEL, assert_bands_intact, assert_overwritten, assert_same_bits, banded,
                               banded_host_results)
from tests.helpers import product_model_from_golden
from tests.quasiharmonic_cases import LATTICE, face_frames

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"
_MAP = np.array([0, 3, 4, 3, 1, 5, 4, 5, 2])             # tensor entry 3 r + s -> component (xx, yy, zz, xy, xz, yz)
_VEC_TO_TENSOR = np.array([[0, 3, 4], [3, 1, 5], [4, 5, 2]])
F64_REL = 5e-8        # tests/test_sparse_graphs_gpu.py::test_float64_evaluation_against_the_float64_oracle
SPECTRUM_REL = 1e-10  # tests/test_gpu_parity.py::test_md_spectrum_on_device_matches_host; tests/test_ensemble_spectra.py::TOL
DEFINITION_REL = 1e-10  # tests/test_mode_raman_gpu.py::test_contraction_matches_the_definition; test_interpolation_model_gpu.py
ORACLE_F64 = 1e-9     # tests/test_partial_spectra_gpu.py, test_mode_raman_gpu.py, test_input_gradients.py: float64 vs the oracle
ORACLE_F32 = 5e-5     # the same tests in float32
TRAIN_INPUTS = 1.5e-4  # tests/test_input_gradients.py::test_training_step_input_gradients
TRAIN_OUT = 2e-5      # tests/test_sparse_graphs_gpu.py::test_training_gradients_against_autograd, the float32 outputs
REPEAT_F64_VJP = 1e-13  # tests/test_input_gradients.py::test_chunking_and_repeated_backward
REPEAT_F32 = 1e-5     # tests/test_input_gradients.py::_same_as_plain_step and ::test_cuda_inputs_stay_on_device_...


class _Recorder:  # pylint: disable=too-few-public-methods
    """The loaded library, remembering which entries were asked for."""

    def __init__(self, lib):
        self._lib, self.called = lib, []

    def __getattr__(self, name):
        self.called.append(name)
        return getattr(self._lib, name)


@pytest.fixture(autouse=True)
def library(monkeypatch):
    torch.set_default_device(None)
    recorder = _Recorder(_lib.load())
    monkeypatch.setattr(_lib, "_lib", recorder)
    yield recorder


class Arena:
    """The arrays of one run: tensors that own their allocations (``lead=None``), or views ``lead`` elements into
    guarded buffers."""

    def __init__(self, lead=None):
        self.lead, self.inputs, self.outputs, self.host = lead, [], [], []

    def tensor(self, values, dtype=torch.float64, what="input", row=0):
        """A device input holding ``values``."""
        if self.lead is None:
            return torch.tensor(np.ascontiguousarray(values), dtype=dtype, device=DEVICE)
        buffer, view = banded(values, dtype, self.lead, NAN, device=DEVICE, row=row)
        self.inputs.append((buffer, view, what))
        return view

    def array(self, values, what="host input", row=0):
        """A host input holding ``values`` (float64)."""
        if self.lead is None:
            return np.array(values, dtype=np.float64)
        buffer, view = banded(values, np.float64, self.lead, NAN, row=row)
        self.inputs.append((buffer, view, what))
        return view

    def out(self, shape, dtype=torch.float64, what="out", row=0, untouched=None):
        """A device output, pre-filled; ``untouched``: a mask of the elements the entry leaves alone."""
        buffer, view = banded(tuple(shape), dtype, self.lead or 0, SENTINEL, device=DEVICE, row=row if self.lead else 0)
        self.outputs.append((buffer, view, what, untouched))
        return view

    @contextlib.contextmanager
    def host_results(self, module, zeros=False):
        """The host results ``module`` allocates for its C entries while the block runs are banded too."""
        if self.lead is None:
            yield
            return
        with banded_host_results(module, self.lead, zeros) as results:
            yield
        self.host.extend(results)

    def check(self):
        """No band changed, every output fully written (or left alone where that is the contract)."""
        torch.cuda.synchronize()
        for buffer, view, what in self.inputs:
            assert_bands_intact(buffer, view, f"{what} (lead {self.lead})")
        for buffer, view, what, untouched in self.outputs:
            assert_bands_intact(buffer, view, f"{what} (lead {self.lead})")
            assert_overwritten(buffer, view, f"{what} (lead {self.lead})", untouched)
        for index, (buffer, view) in enumerate(self.host):
            assert_bands_intact(buffer, view, f"host result {index} {view.shape} (lead {self.lead})")
            assert_overwritten(buffer, view, f"host result {index} {view.shape} (lead {self.lead})")


def _host(value):
    return value.detach().cpu().numpy() if isinstance(value, torch.Tensor) else np.asarray(value)


def _rel(got, want):
    got, want = _host(got).astype(np.float64), _host(want).astype(np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def _within(bar):
    """The comparison of an entry whose repeats agree to round-off only: the largest difference over the largest entry."""
    def compare(got, want, what):
        assert _host(got).shape == _host(want).shape, what
        assert np.all(np.isfinite(_host(got))), what
        assert _rel(got, want) <= bar, f"{what}: differs from the plain call by {_rel(got, want):.3e} > {bar:.1e}"
    return compare


def run_case(library, label, call, reference, entries, compare=None, host_results=0):
    """``call(arena)`` makes the entry's call on the arena's arrays and returns ``{name: result}``.  ``R0`` of the plain
    arena goes to ``reference``; each banded run is compared with it (``compare``: ``{name: comparison}`` for results that
    are not compared bit for bit) and checked for its bands and outputs; ``entries`` must have been called, and at least
    ``host_results`` host arrays must have been banded."""
    compare = compare or {}
    plain = Arena()
    r0 = {name: _host(value).copy() for name, value in call(plain).items()}
    plain.check()
    reference(r0)
    apart = 0.0
    for lead in LEADS:
        arena = Arena(lead)
        library.called.clear()
        got = call(arena)
        arena.check()
        assert len(arena.host) >= host_results and len(arena.inputs) + len(arena.outputs) + len(arena.host) > 0
        for buffer, view, *_ in arena.inputs + arena.outputs:
            if isinstance(view, torch.Tensor):  # the entry was handed this very address, `lead` elements into its buffer
                assert view.data_ptr() - buffer.data_ptr() >= lead * view.element_size()
                assert (view.data_ptr() % (2 * view.element_size()) != 0) == (lead % 2 == 1)
        for entry in entries:
            assert entry in ENTRIES and entry in library.called, f"{entry} was not called"
        for name, want in r0.items():
            compare.get(name, assert_same_bits)(_host(got[name]), want, f"{label}: {name} at lead {lead}")
            if name in compare:
                apart = max(apart, _rel(got[name], want))
    how = "bit-identical" if not compare else (f"bit-identical but {', '.join(sorted(compare))}: at most {apart:.1e} apart "
                                               "(the entry's round-off bar)")
    print(f"GUARD | {', '.join(entries)} | {label} | offsets {LEADS[0]}, {LEADS[1]} | {how}, bands intact")


def test_the_arena_reports_an_overrun_and_a_gap_on_the_device():
    """The checks themselves, on tensors: a store one element past a view, a store before it, an element never written."""
    for lead in LEADS:
        arena = Arena(lead)
        out = arena.out((3, 5), what="out")
        out.fill_(1.0)
        arena.check()
        buffer = arena.outputs[0][0]
        end = lead + out.numel()
        buffer[end] = 2.0
        with pytest.raises(AssertionError, match="out .*: written \\+1 elements past the end"):
            arena.check()
        buffer[end] = buffer[end + 1]
        buffer[lead - 2] = float("nan")
        with pytest.raises(AssertionError, match="out .*: written -2 elements before the start"):
            arena.check()
        buffer[lead - 2] = buffer[0]
        arena.check()
        arena = Arena(lead)
        out = arena.out((3, 5), what="out")
        out[:, :4] = 1.0
        with pytest.raises(AssertionError, match="3 elements never written, the first at flat index 4"):
            arena.check()
        source = arena.tensor(np.ones(7), what="positions")
        assert bool(torch.isnan(arena.inputs[0][0][:lead]).all()) and float(source.sum()) == 7.0


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(tensor):
    return None if tensor is None else C.c_void_p(tensor.data_ptr())


# ----------------------------------------------------------------------------- harmonic synthesis
@pytest.mark.parametrize("name", ["66 columns, 17 modes, 257 frames", "129 columns, one mode, 257 frames, three runs"])
def test_harmonic_synthesis(library, name):
    """Tiles of 64 frames x 128 columns x 16 modes; only ``out`` is device memory."""
    from tests.test_harmonic_trajectory_gpu import _case, _worst
    (ref, D, omega_dt, amp, phase), frames, first, want = _case(name)

    def call(arena):
        out = arena.out(want.shape, row=want.shape[2] * 3)
        assert harmonic.synthesize_device(ref, D, omega_dt, amp, phase, frames, first, out=out) is out
        return {"out": out}

    def reference(r0):
        assert _worst(r0["out"], want, amp, D)[0] <= 1.0

    run_case(library, name, call, reference, ["rn_ht_synthesize_device"])


# ----------------------------------------------------------------------------- quasi-harmonic moments
@pytest.mark.parametrize("name", ["129 columns, a chunk and a frame, three blocks", "two frames of one atom"])
def test_quasiharmonic_moments(library, name):
    from tests.quasiharmonic_cases import moment_differences
    from tests.test_quasiharmonic_gpu import TOLERANCE_FIRST, TOLERANCE_SECOND, _case
    positions, anchor, bounds, joined, want = _case(name)

    def call(arena):
        tensor = arena.tensor(positions, what="positions", row=positions[0].size)
        with arena.host_results(quasiharmonic, zeros=True):
            first, second, counts = quasiharmonic.moments_device(tensor, anchor, bounds, joined)
        return {"first": first, "second": second, "counts": counts}

    def reference(r0):
        first, second = moment_differences((r0["first"], r0["second"], r0["counts"]), want)
        assert second <= TOLERANCE_SECOND and first <= TOLERANCE_FIRST

    run_case(library, name, call, reference, ["rn_qh_moments_device"], host_results=3)


# ----------------------------------------------------------------------------- band moments
def test_band_moments(library):
    """66 columns (3N + 6): two column tiles, the second partial; two weight rows; device positions and device alpha."""
    from tests.band_modes_cases import device_case, host_moments, moment_error, weight_sets
    from tests.test_band_modes_gpu import TOLERANCE
    name, weights_name = "20 atoms, W = 34, 2 segments", "every bin, two rows"
    positions, masses, alpha, width, starts, taper = device_case(name)
    weights = weight_sets((width - 1 + 1) // 2 - 1)[weights_name]
    assert len(weights) == 2
    want = host_moments(name, True, weights_name)

    def call(arena):
        d_positions = arena.tensor(positions, what="positions", row=positions[0].size)
        d_alpha = arena.tensor(alpha, what="alpha", row=9)
        with arena.host_results(bandmodes, zeros=True):
            moments = bandmodes.band_moments_device(d_positions, LATTICE, masses, d_alpha, width, starts, taper, weights)
        return {"moments": moments}

    def reference(r0):
        assert moment_error(r0["moments"], want) <= TOLERANCE

    run_case(library, f"{name}, {weights_name}", call, reference, ["rn_bm_moments_device"], host_results=1)


# ----------------------------------------------------------------------------- the interpolation model
def _jacobian_increments(jac, positions):
    """``(mean Jacobian rows (T,6,N,3), minimum-image steps (T,N,3))`` of the trapezoid increments."""
    step = positions[1:] - positions[:-1]
    return 0.5 * (jac[:-1] + jac[1:]), step - np.rint(step)


def _group_increments(jac, positions, labels, groups):
    """``out[t][g][3r+s] = sum_{i in g} 1/2 (J_map(r,s)(t) + J_map(r,s)(t+1))[i] . dx_t[i]`` (include/rn_interp.h)."""
    mean, dx = _jacobian_increments(jac, positions)
    out = np.zeros((len(dx), groups, 9))
    for g in range(groups):
        mask = labels == g
        out[:, g] = np.einsum("tcir,tir->tc", mean[:, :, mask], dx[:, mask])[:, _MAP]
    return out.reshape(len(dx), groups, 3, 3)


def _mode_increments(jac, positions, disp, proj, sigma=None):
    """The definition of ``rn_potgnn_mode_contract_device`` (include/rn_potgnn.h): ``(T, M + 1, 9)``, the rest last."""
    mean, dx = _jacobian_increments(jac, positions)
    sigma = np.ones(9) if sigma is None else sigma
    a = np.einsum("tcir,mir->tcm", mean, disp)
    q = np.einsum("mir,tir->tm", proj, dx)
    modes = sigma[None, None, :] * np.swapaxes(a[:, _MAP], 1, 2) * q[:, :, None]
    total = sigma[None, :] * np.einsum("tcir,tir->tc", mean, dx)[:, _MAP]
    return np.concatenate([modes, (total - modes.sum(axis=1))[:, None]], axis=1)


def _channel_errors(got, want):
    """The largest difference of each channel (axis 1) over the channel's largest entry."""
    got, want = got.reshape(got.shape[0], got.shape[1], -1), want.reshape(want.shape[0], want.shape[1], -1)
    scale = np.abs(want).max(axis=(0, 2))
    assert np.all(scale > 0)
    return np.abs(got - want).max(axis=(0, 2)) / scale


@pytest.mark.parametrize("frames,atoms,dofs", [(33, 67, 130), (17, 5, 15)])
def test_interp_forward_and_jacobian(library, frames, atoms, dofs):
    """Tiles of 16 frames x 64 DOFs x 32 columns of 3N."""
    from tests.interp_cases import seeded_case, seeded_frames
    case = seeded_case(100 * frames + dofs, atoms, dofs)
    positions = seeded_frames(case, frames, frames)
    assert case.breakpoint_gap(positions, orders=(1,)) > 1e-9  # (a kink is a jump of the Jacobian: an input choice)
    want_alpha, want_jac = case.host(positions, jacobian=True)
    model = case.model()

    def call(arena):
        d_positions = arena.tensor(positions, what="positions", row=3 * atoms)
        alpha = arena.out((frames, 3, 3), what="alpha", row=9)
        jac = arena.out((frames, 6, atoms, 3), what="jacobian", row=3 * atoms)
        assert model.calc_polarizabilities_device(d_positions, out=alpha) is alpha
        assert model.calc_jacobian_device(d_positions, out=jac) is jac
        return {"alpha": alpha, "jacobian": jac}

    def reference(r0):
        assert _rel(r0["alpha"], want_alpha) <= DEFINITION_REL and _rel(r0["jacobian"], want_jac) <= DEFINITION_REL

    run_case(library, f"({frames},{atoms},{dofs})", call, reference, ["rn_interp_forward_device", "rn_interp_jacobian_device"])


def test_interp_group_increments(library):
    """67 atoms in groups of 1, 65 and 1: one lane-strided wave per group, one of them over more than 64 atoms."""
    from tests.interp_cases import seeded_case, seeded_frames
    frames, atoms = 18, 67
    case = seeded_case(6701, atoms, 130)
    positions = seeded_frames(case, 6702, frames)
    labels = np.array([0] + [1] * 65 + [2], dtype=np.int32)
    assert case.breakpoint_gap(positions, orders=(1,)) > 1e-9
    want = _group_increments(case.host(positions, jacobian=True)[1], positions, labels, 3)
    model = case.model()

    def call(arena):
        d_positions = arena.tensor(positions, what="positions", row=3 * atoms)
        out = arena.out((frames - 1, 3, 3, 3), row=27)
        assert model.calc_group_increments_device(d_positions, labels, out=out) is out
        return {"out": out}

    def reference(r0):
        assert _channel_errors(r0["out"], want).max() <= DEFINITION_REL

    run_case(library, f"{frames} frames, {atoms} atoms, groups of 1, 65, 1", call, reference,
             ["rn_interp_group_increments_device"])


@pytest.mark.parametrize("rest", [True, False])
def test_interp_mode_increments(library, rest):
    """3N = 33, 17 steps, 65 modes against tiles of 16 steps x 64 modes x 32 columns."""
    from tests.interp_cases import seeded_case, seeded_frames
    frames, atoms, modes = 18, 11, 65
    case = seeded_case(1101, atoms, 20)
    positions = seeded_frames(case, 1102, frames)
    assert case.breakpoint_gap(positions, orders=(1,)) > 1e-9
    rng = np.random.default_rng(1103)
    disp, proj = rng.normal(size=(modes, atoms, 3)), rng.normal(size=(modes, atoms, 3))
    want = _mode_increments(case.host(positions, jacobian=True)[1], positions, disp, proj)[:, :modes + rest]
    model = case.model()

    def call(arena):
        d_positions = arena.tensor(positions, what="positions", row=3 * atoms)
        out = arena.out((frames - 1, modes + rest, 3, 3), row=9 * (modes + rest))
        assert model.calc_mode_increments_device(d_positions, disp, proj, rest=rest, out=out) is out
        return {"out": out}

    def reference(r0):
        assert _channel_errors(r0["out"], want).max() <= DEFINITION_REL

    run_case(library, f"{frames} frames, {atoms} atoms, {modes} modes, rest={rest}", call, reference,
             ["rn_interp_mode_increments_device"])


# ----------------------------------------------------------------------------- the contraction alone
@pytest.mark.parametrize("rest", [1, 0])
def test_mode_contract(library, rest):
    """Handle-free, through ctypes; ``out_channels = M + 3``: the channels past ``M + rest`` keep their pre-fill."""
    from tests.test_mode_raman_gpu import _contraction_case
    frames, atoms, modes = 18, 11, 65
    jac, pos, disp, proj, sigma, want = _contraction_case(frames, atoms, modes)
    np.testing.assert_array_equal(want, _mode_increments(jac, pos, disp, proj, sigma))  # (one definition, two places)
    channels = modes + 3
    sigma = np.ascontiguousarray(sigma)
    untouched = np.zeros((frames - 1, channels, 9), dtype=bool)
    untouched[:, modes + rest:] = True

    def call(arena):
        d_jac = arena.tensor(jac, what="jac", row=3 * atoms)
        d_pos = arena.tensor(pos, what="positions", row=3 * atoms)
        d_disp = arena.tensor(disp, what="disp", row=3 * atoms)
        d_proj = arena.tensor(proj, what="proj", row=3 * atoms)
        out = arena.out((frames - 1, channels, 9), row=9 * channels, untouched=untouched)
        rc = _lib.load().rn_potgnn_mode_contract_device(_p(d_jac), frames, _p(d_pos), atoms, _p(d_disp), _p(d_proj), modes,
                                                        C.c_void_p(sigma.ctypes.data), rest, channels, _p(out), _stream())
        assert rc == _lib.RN_OK
        return {"out": out[:, :modes + rest]}

    def reference(r0):
        assert _channel_errors(r0["out"], want[:, :modes + rest]).max() <= DEFINITION_REL

    run_case(library, f"{frames} frames, {atoms} atoms, {modes} modes, rest={rest}, {channels} channels", call, reference,
             ["rn_potgnn_mode_contract_device"])


# ----------------------------------------------------------------------------- PotGNN evaluation
def _oracle_alpha(oracle64, positions, lattices):
    from oracle import potgnn_oracle as O
    with torch.no_grad():
        vec6 = O.forward(oracle64, torch.tensor(positions, dtype=torch.float64), faithful=False,
                         lattices=None if lattices is None else torch.tensor(lattices, dtype=torch.float64)).numpy()
    return vec6[:, _VEC_TO_TENSOR] * oracle64.std + oracle64.mean


@functools.lru_cache(maxsize=None)
def _evaluation_case(kind):
    """``(model, oracle64, positions[7], lattices[7], oracle alpha for the fixed cell, for the lattices)``.  "narrow":
    the tio2_notebook golden at its widths (5, 14); "wide": the triclinic20 golden's structure at (64, 64)."""
    from oracle import potgnn_oracle as O
    from tests.test_gpu_parity import _random_model
    if kind == "narrow":
        g = load_golden("tio2_notebook")
        model = product_model_from_golden(g).eval()
        oracle = O.model_from_arrays(g)
        oracle.coefficient = model.gauss_coefficient
    else:
        g = load_golden("triclinic20")
        model, oracle = _random_model(g, 3.0, 64, 64, 2, seed=64 * 131 + 64)
        model.eval()
    oracle64 = oracle.to(torch.float64)
    rng = np.random.default_rng(7)
    positions = g["positions"][None] + rng.normal(scale=3e-3, size=(7,) + g["positions"].shape)
    positions = np.ascontiguousarray(positions - np.floor(positions))
    strain = 0.01 * rng.standard_normal((7, 3, 3))
    lattices = np.ascontiguousarray(np.asarray(g["lattice"], dtype=np.float64)[None] @ (np.eye(3)[None] + strain))
    return model, oracle64, positions, lattices, _oracle_alpha(oracle64, positions, None), _oracle_alpha(oracle64, positions,
                                                                                                         lattices)


def _evaluation_reference(oracle64, want, bar):
    def reference(r0):
        got = (r0["alpha"] - oracle64.mean) / oracle64.std
        assert _rel(got, (want - oracle64.mean) / oracle64.std) < bar
    return reference


@pytest.mark.parametrize("with_lattices", [False, True])
@pytest.mark.parametrize("dtype", [None, torch.float64])
@pytest.mark.parametrize("frames", [1, 7])
@pytest.mark.parametrize("kind", ["narrow", "wide"])
def test_potgnn_evaluation(library, kind, frames, dtype, with_lattices):
    from tests.test_gpu_parity import REL
    model, oracle64, positions, lattices, fixed, cells = _evaluation_case(kind)
    flags = model.config_flags()
    assert flags["narrow_kernels"] if kind == "narrow" else flags["fused_edge_block"] and flags["role_split_edge_block"]
    atoms = positions.shape[1]

    def call(arena):
        d_positions = arena.tensor(positions[:frames], what="positions", row=3 * atoms)
        d_lattices = arena.tensor(lattices[:frames], what="lattices", row=9) if with_lattices else None
        out = arena.out((frames, 3, 3), row=9)
        assert model.calc_polarizabilities_device(d_positions, out=out, dtype=dtype, lattices=d_lattices) is out
        return {"alpha": out}

    entry = "rn_potgnn_forward_cells_device" if with_lattices else (
        "rn_potgnn_forward_device_f64" if dtype is torch.float64 else "rn_potgnn_forward_device")
    want = (cells if with_lattices else fixed)[:frames]
    run_case(library, f"{kind}, S = {frames}, {'float64' if dtype else 'float32'}, lattices={with_lattices}", call,
             _evaluation_reference(oracle64, want, F64_REL if dtype else REL), [entry])


@pytest.mark.parametrize("with_lattices", [False, True])
@pytest.mark.parametrize("frames", [1, 7])
@pytest.mark.parametrize("kind", ["narrow", "wide"])
def test_potgnn_evaluation_to_device(library, kind, frames, with_lattices):
    """Host positions (and lattices) in, ``out`` in HBM: the host inputs are banded as well."""
    from tests.test_gpu_parity import REL
    model, oracle64, positions, lattices, fixed, cells = _evaluation_case(kind)
    atoms = positions.shape[1]

    def call(arena):
        h_positions = arena.array(positions[:frames], what="host positions", row=3 * atoms)
        h_lattices = arena.array(lattices[:frames], what="host lattices", row=9) if with_lattices else None
        out = arena.out((frames, 3, 3), row=9)
        assert model.calc_polarizabilities_to_device(h_positions, out=out, lattices=h_lattices) is out
        return {"alpha": out}

    entry = "rn_potgnn_calc_polarizabilities_cells_to_device" if with_lattices else "rn_potgnn_calc_polarizabilities_to_device"
    want = (cells if with_lattices else fixed)[:frames]
    run_case(library, f"{kind}, S = {frames}, lattices={with_lattices}", call, _evaluation_reference(oracle64, want, REL),
             [entry])


# ----------------------------------------------------------------------------- forward_samples_device, forward_vjp_device
def _samples_case(name="triclinic20"):
    """``(g, model, float32 oracle, positions[3], strained lattices[3], mixed species[3], atom types[3])``."""
    from tests.test_input_gradients import _case, _inputs
    g, model, oracle = _case(name)
    pos, lat, zs = _inputs(g, model, 3, strained=True, mixed=True)
    types = np.ascontiguousarray(model.atom_type_map[zs], dtype=np.int32)
    assert types.min() >= 0
    return g, model, oracle, np.ascontiguousarray(pos), np.ascontiguousarray(lat), zs, types


def test_potgnn_forward_samples(library):
    """Through ctypes on the model's handle, as ``PotGNN._forward_on_device`` calls it (the front end copies its inputs):
    float32 lattices, int32 atom types, float64 positions in, float32 6-vectors out; element alignment is 4 bytes."""
    from oracle import potgnn_oracle as O
    from tests.test_gpu_parity import REL
    _, model, oracle, pos, lat, zs, types = _samples_case()
    with torch.no_grad():
        front_end = model(torch.tensor(lat, device=DEVICE), torch.tensor(zs, device=DEVICE), torch.tensor(pos, device=DEVICE))
        want = O.forward(oracle.to(torch.float64), torch.tensor(pos), faithful=False, lattices=torch.tensor(lat),
                         atomic_numbers=zs).numpy()
    assert front_end.is_cuda and front_end.dtype == torch.float32
    handle = model._ensure_handle()

    def call(arena):
        d_lat = arena.tensor(lat.reshape(3, 9), torch.float32, "lattices", row=9)
        d_types = arena.tensor(types, torch.int32, "atom types", row=types.shape[1])
        d_pos = arena.tensor(pos, what="positions", row=pos[0].size)
        out = arena.out((3, 6), torch.float32, "vec6", row=6)
        rc = _lib.load().rn_potgnn_forward_samples_device(handle, _p(d_lat), _p(d_types), _p(d_pos), 3, _p(out), _stream(), 1)
        _lib.check(rc, handle, "rn_potgnn_forward_samples_device")
        return {"vec6": out}

    def reference(r0):
        assert_same_bits(r0["vec6"], front_end, "the ctypes call against PotGNN.forward")
        assert _rel(r0["vec6"], want) < REL

    run_case(library, "triclinic20, S = 3, strained cells, mixed species", call, reference,
             ["rn_potgnn_forward_samples_device"])


@pytest.mark.parametrize("float64", [False, True])
def test_potgnn_forward_vjp(library, float64):
    """``d_dvec6`` in, ``d_dpos`` and ``d_dlat`` out, through ctypes as ``PotGNN._input_gradients`` calls it.  The
    reverse pass accumulates with atomics (``guard_band_cases.ENTRIES``): the gradients are compared at the bar of the
    entry's own repeat tests."""
    from tests.test_input_gradients import _device_grads, _oracle_grads
    _, model, oracle, pos, lat, zs, types = _samples_case()
    if float64:
        model.double()
    v = np.random.default_rng(5).standard_normal((3, 6))
    want_pos, want_lat = _oracle_grads(oracle, pos, lat, zs, v)
    _, front_pos, front_lat = _device_grads(model, pos, lat, zs, v, where="cuda")
    handle = model._ensure_handle()
    atoms = pos.shape[1]
    bar = REPEAT_F64_VJP if float64 else REPEAT_F32

    def call(arena):
        d_lat = arena.tensor(lat.reshape(3, 9), what="lattices", row=9)
        d_types = arena.tensor(types, torch.int32, "atom types", row=atoms)
        d_pos = arena.tensor(pos, what="positions", row=3 * atoms)
        d_dvec6 = arena.tensor(v, what="dvec6", row=6)
        dpos = arena.out((3, atoms, 3), what="dpos", row=3 * atoms)
        dlat = arena.out((3, 9), what="dlat", row=9)
        rc = _lib.load().rn_potgnn_forward_vjp_device(handle, _p(d_lat), _p(d_types), _p(d_pos), 3, _p(d_dvec6), int(float64),
                                                      _p(dpos), _p(dlat), _stream())
        _lib.check(rc, handle, "rn_potgnn_forward_vjp_device")
        return {"dpos": dpos, "dlat": dlat}

    def reference(r0):
        assert _rel(r0["dpos"], front_pos) <= bar and _rel(r0["dlat"].reshape(3, 3, 3), front_lat) <= bar
        oracle_bar = ORACLE_F64 if float64 else ORACLE_F32
        assert _rel(r0["dpos"], want_pos) < oracle_bar and _rel(r0["dlat"].reshape(3, 3, 3), want_lat) < oracle_bar

    run_case(library, f"triclinic20, S = 3, float64={float64}", call, reference, ["rn_potgnn_forward_vjp_device"],
             compare={"dpos": _within(bar), "dlat": _within(bar)})


# ----------------------------------------------------------------------------- PotGNN increments
@functools.lru_cache(maxsize=None)
def _increments_case():
    """The triclinic20 product model, six frames of the variable-cell tests' MD series with their lattices, five modes, and
    the Jacobians ``d alpha / d x`` ``(S,3,3,N,3)`` and ``d alpha / d L`` ``(S,3,3,3,3)`` by autograd through the
    float64 oracle, for the fixed cell and for the lattices."""
    from oracle import potgnn_oracle as O
    from ramannoodle_amd.spectrum import group_labels, mode_projectors
    from tests.test_variable_cell_gpu import _series
    g = load_golden("triclinic20")
    model = product_model_from_golden(g).eval()
    oracle = O.model_from_arrays(g)
    oracle.coefficient = model.gauss_coefficient
    oracle64 = oracle.to(torch.float64)
    positions, lattices = (np.ascontiguousarray(x[:6]) for x in _series(4.0, 33))
    std = np.asarray(g["std"])[None, :, :, None, None]
    jacobians = {}
    for cells in (False, True):
        x = torch.tensor(positions, dtype=torch.float64, requires_grad=True)
        lat = torch.tensor(lattices if cells else np.broadcast_to(g["lattice"], (6, 3, 3)).copy(), dtype=torch.float64,
                           requires_grad=True)
        out = O.forward(oracle64, x, faithful=False, grad=True, lattices=lat)
        grads = [torch.autograd.grad(out[:, c].sum(), (x, lat), retain_graph=True) for c in range(6)]
        jacobians[cells] = (std * np.stack([gx.numpy() for gx, _ in grads], axis=1)[:, _VEC_TO_TENSOR],
                            std * np.stack([gl.numpy() for _, gl in grads], axis=1)[:, _VEC_TO_TENSOR])
    labels, groups = group_labels("species", g["atomic_numbers"])
    disp, proj = mode_projectors(g["ph/displacements"][:5], g["lattice"], np.ones(model.num_atoms))
    return model, positions, lattices, jacobians, labels, groups, disp, proj


def _oracle_channels(kind, cells):
    """The increments ``(5, channels, 3, 3)`` of the definitions of include/rn_potgnn.h from the oracle's Jacobians."""
    _, positions, lattices, jacobians, labels, groups, disp, proj = _increments_case()
    jac_x, jac_l = jacobians[cells]
    mean = 0.5 * (jac_x[:-1] + jac_x[1:])
    step = positions[1:] - positions[:-1]
    dx = step - np.round(step)
    if kind == "group":
        channels = [np.einsum("tabnk,tnk->tab", mean[..., labels == k, :], dx[:, labels == k]) for k in range(groups)]
    else:
        modes = np.einsum("tabir,mir->tmab", mean, disp) * np.einsum("mir,tir->tm", proj, dx)[:, :, None, None]
        channels = [modes[:, m] for m in range(len(disp))] + [np.einsum("tabir,tir->tab", mean, dx) - modes.sum(axis=1)]
    if cells:
        channels.append(np.einsum("tabij,tij->tab", 0.5 * (jac_l[:-1] + jac_l[1:]), np.diff(lattices, axis=0)))
    return np.stack(channels, axis=1)


@pytest.mark.parametrize("variant", ["whole", "lattices", "chunked"])
@pytest.mark.parametrize("kind", ["group", "modes"])
def test_potgnn_increments(library, kind, variant):
    """Six frames, groups by species / five modes and the rest, in float64; "chunked": a workspace limit that forces
    several chunks, whose one-frame carry-over reads the banded tensor at a chunk edge.  The Jacobian rows come from the
    reverse pass, which accumulates with atomics: compared at ``tests/test_chunk_walk_gpu.py::TOLERANCE``."""
    from tests.test_chunk_walk_gpu import TOLERANCE
    model, positions, lattices, _, _, groups, disp, proj = _increments_case()
    cells = variant == "lattices"
    want = _oracle_channels(kind, cells)
    atoms = positions.shape[1]

    def entry_call(d_positions, d_lattices, out, limit):
        if kind == "group":
            return model.calc_group_increments_device(d_positions, "species", out=out, workspace_limit=limit,
                                                      lattices=d_lattices)
        return model.calc_mode_increments_device(d_positions, disp, proj, out=out, workspace_limit=limit, lattices=d_lattices)

    limit = 0
    if variant == "chunked":  # the smallest power-of-two workspace one step fits in, as test_chunking_agrees finds it
        probe, limit = Arena(), 1 << 16
        d_positions = probe.tensor(positions)
        while True:
            try:
                entry_call(d_positions, None, None, limit)
                break
            except MemoryError:
                limit <<= 1
                assert limit <= 1 << 32
        torch.cuda.synchronize()

    def call(arena):
        d_positions = arena.tensor(positions, what="positions", row=3 * atoms)
        d_lattices = arena.tensor(lattices, what="lattices", row=9) if cells else None
        out = arena.out(want.shape, row=9 * want.shape[1])
        assert entry_call(d_positions, d_lattices, out, limit) is out
        return {"out": out}

    def reference(r0):
        assert r0["out"].shape == (5, (groups if kind == "group" else 6) + cells, 3, 3)
        assert _rel(r0["out"], want) < ORACLE_F64
        for channel in range(want.shape[1]):
            assert _rel(r0["out"][:, channel], want[:, channel]) < ORACLE_F64, channel

    entry = {"group": "rn_potgnn_group_increments_cells_device" if cells else "rn_potgnn_group_increments_device",
             "modes": "rn_potgnn_mode_increments_device"}[kind]
    run_case(library, f"triclinic20, 6 frames, {kind}, {variant}" + (f" (workspace_limit {limit})" if limit else ""), call,
             reference, [entry], compare={"out": _within(TOLERANCE[True])})


# ----------------------------------------------------------------------------- device-resident training
def _training_model():
    from tests.test_gpu_parity import _load_train_case
    g, model, _, _, _ = _load_train_case()
    model.enable_device_training()
    model.train()
    return g, model


def test_potgnn_device_training(library):
    """The three device-resident training entries through ctypes, as ``PotGNN._train_forward_on_device`` and
    ``_train_backward_on_device`` call them, against those two methods on a twin model: a step with input gradients,
    then a step without.  The 6-vectors are compared bit for bit; the gradients, which the reverse pass accumulates
    with atomics, at the bar of ``tests/test_input_gradients.py::_same_as_plain_step``."""
    from oracle import potgnn_oracle as O
    from tests.test_input_gradients import _inputs, _oracle_grads
    g, twin = _training_model()
    pos, lat, zs = _inputs(g, twin, 3, strained=True, mixed=True)
    pos, lat = np.ascontiguousarray(pos), np.ascontiguousarray(lat)
    types = np.ascontiguousarray(twin.atom_type_map[zs], dtype=np.int32)
    atoms = pos.shape[1]
    v = np.random.default_rng(5).standard_normal((3, 6)).astype(np.float32)
    oracle = O.model_from_arrays(g)
    oracle.coefficient = twin.gauss_coefficient
    with torch.no_grad():
        want_out = O.forward(oracle.to(torch.float64), torch.tensor(pos), faithful=False, train=True,
                             lattices=torch.tensor(lat), atomic_numbers=zs).numpy()
    want_pos, want_lat = _oracle_grads(oracle, pos, lat, zs, v.astype(np.float64), train=True)

    # the twin: the front end's own two methods
    tensors = (torch.tensor(lat, device=DEVICE), torch.tensor(zs, device=DEVICE), torch.tensor(pos, device=DEVICE))
    cotangent = torch.tensor(v, device=DEVICE)
    twin_out = twin._train_forward_on_device(*tensors)
    twin_pos, twin_lat = twin._train_backward_on_device(cotangent, want_pos=True, want_lat=True)
    torch.cuda.synchronize()
    twin_with_inputs = twin.device_gradients().clone()
    twin_out_again = twin._train_forward_on_device(*tensors)
    twin._train_backward_on_device(cotangent)
    torch.cuda.synchronize()
    twin_plain = twin.device_gradients().clone()
    front = {"vec6": twin_out, "dpos": twin_pos, "dlat": twin_lat, "gradients with inputs": twin_with_inputs,
             "vec6 again": twin_out_again, "gradients": twin_plain}

    def call(arena):
        _, model = _training_model()
        handle = model._ensure_handle()
        lib = _lib.load()
        d_lat = arena.tensor(lat.reshape(3, 9), torch.float32, "lattices", row=9)
        d_types = arena.tensor(types, torch.int32, "atom types", row=atoms)
        d_pos = arena.tensor(pos, what="positions", row=3 * atoms)
        d_dvec6 = arena.tensor(v, torch.float32, "dvec6", row=6)
        results = {}
        for step in ("", " again"):
            out = arena.out((3, 6), torch.float32, "vec6" + step, row=6)
            model._install_reducer(handle)
            rc = lib.rn_potgnn_train_forward_samples_device(handle, _p(d_lat), _p(d_types), _p(d_pos), 3, _p(out), _stream())
            _lib.check(rc, handle, "rn_potgnn_train_forward_samples_device")
            model._device_batches_tracked += 1
            model._device_ahead = True
            results["vec6" + step] = out
            if not step:
                dpos = arena.out((3, atoms, 3), what="dpos", row=3 * atoms)
                dlat = arena.out((3, 9), what="dlat", row=9)
                rc = lib.rn_potgnn_train_backward_inputs_device(handle, _p(d_dvec6), _p(dpos), _p(dlat), _stream())
                _lib.check(rc, handle, "rn_potgnn_train_backward_inputs_device")
                torch.cuda.synchronize()
                results.update({"dpos": dpos, "dlat": dlat, "gradients with inputs": model.device_gradients().clone()})
            else:
                rc = lib.rn_potgnn_train_backward_samples_device(handle, _p(d_dvec6), _stream())
                _lib.check(rc, handle, "rn_potgnn_train_backward_samples_device")
                torch.cuda.synchronize()
                results["gradients"] = model.device_gradients().clone()
        return results

    close = _within(REPEAT_F32)

    def reference(r0):
        for name in ("vec6", "vec6 again"):
            assert_same_bits(r0[name], front[name], f"{name}: the ctypes call against the front end")
            assert _rel(r0[name], want_out) <= TRAIN_OUT
        for name in ("dpos", "dlat", "gradients with inputs", "gradients"):
            close(r0[name], _host(front[name]), f"{name}: the ctypes call against the front end")
        assert _rel(r0["dpos"], want_pos) < TRAIN_INPUTS and _rel(r0["dlat"].reshape(3, 3, 3), want_lat) < TRAIN_INPUTS

    run_case(library, "triclinic20_train, S = 3, strained cells, mixed species", call, reference,
             ["rn_potgnn_train_forward_samples_device", "rn_potgnn_train_backward_inputs_device",
              "rn_potgnn_train_backward_samples_device"],
             compare={name: close for name in ("dpos", "dlat", "gradients with inputs", "gradients")})


# ----------------------------------------------------------------------------- the spectrum reducers
TIMESTEP = 1.5
SERIES = {4: (4, 1), 258: (130, 64)}  # frames: (segment_steps, hop): the last segment ends on the last frame
RUN_LENGTHS = [5, 7]                   # one joined tensor; segments of 5 frames, 2 apart: the last ends on the last frame
RUN_SEGMENTS = (5, 2)
INCIDENT, SCATTERED = np.array([1.0, 0.0, 0.0]), np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


def _alpha_series(frames, seed=0):
    rng = np.random.default_rng(frames + seed)
    t = np.arange(frames)[:, None, None]
    alpha = rng.normal(size=(frames, 3, 3)) * 0.1 + np.sin(0.05 * t * (1 + np.arange(9).reshape(3, 3)))
    return alpha + np.swapaxes(alpha, 1, 2)


def _increment_series(rows, channels, seed=0):
    rng = np.random.default_rng(1000 * rows + channels + seed)
    t = np.arange(rows)[:, None, None, None]
    phase = np.arange(channels)[None, :, None, None]
    incr = 0.02 * rng.normal(size=(rows, channels, 3, 3)) + 0.05 * np.cos(0.07 * t * (1 + np.arange(9).reshape(3, 3)) + phase)
    return incr + np.swapaxes(incr, 2, 3)


def _position_series(frames, atoms=5):
    """Wrapped positions on the cell faces and a lattice per frame, so that ``d_lattices`` is a series as well."""
    rng = np.random.default_rng(frames)
    strain = 0.005 * rng.standard_normal((frames, 3, 3))
    return face_frames(atoms, frames, seed=frames), LATTICE[None] @ (np.eye(3)[None] + strain), rng.uniform(1.0, 4.0, atoms)


def _measure_case(library, label, make, methods, entries, modules=(spectrum,)):
    """``make(arena)`` builds the device class on the arena's tensors; ``methods``: ``{name: f(object, host)}`` returning
    an array.  The host statement of each method is the same method with ``host=True``."""
    def call(arena):
        measured = {}
        with contextlib.ExitStack() as stack:
            for module in modules:
                stack.enter_context(arena.host_results(module))
            instance = make(arena)
            for name, method in methods.items():
                measured[name] = method(instance, False)
        return measured

    def reference(r0):
        instance = make(Arena())
        for name, method in methods.items():
            want = method(instance, True)
            assert r0[name].shape == want.shape and np.all(np.isfinite(r0[name])), name
            assert np.abs(r0[name] - want).max() <= SPECTRUM_REL * np.abs(want).max(), name

    run_case(library, label, call, reference, entries, host_results=len(methods))


@pytest.mark.parametrize("frames", list(SERIES))
def test_md_raman(library, frames):
    width, hop = SERIES[frames]
    alpha = _alpha_series(frames)
    _measure_case(
        library, f"DeviceMDRamanSpectrum, {frames} frames, segments of {width} every {hop}",
        lambda arena: spectrum.DeviceMDRamanSpectrum(arena.tensor(alpha, what="alpha", row=9), TIMESTEP),
        {"measure": lambda s, host: s.measure(host=host)[1],
         "measure_polarized": lambda s, host: s.measure_polarized(INCIDENT, SCATTERED, host=host)[1],
         "measure_segments": lambda s, host: s.measure_segments(width, hop, host=host)[1],
         "measure_segments rows": lambda s, host: s.measure_segments(width, hop, average=False, host=host)[1]},
        ["rn_md_raman_intensities_device", "rn_md_raman_polarized_device", "rn_md_raman_segments_device"])


def test_md_raman_ensemble(library):
    alpha = _alpha_series(sum(RUN_LENGTHS))
    _measure_case(
        library, f"DeviceMDRamanEnsemble, one tensor with run_lengths {RUN_LENGTHS}",
        lambda arena: spectrum.DeviceMDRamanEnsemble(arena.tensor(alpha, what="alpha", row=9), TIMESTEP, RUN_LENGTHS),
        {"measure_segments": lambda s, host: s.measure_segments(*RUN_SEGMENTS, host=host)[1],
         "measure_segments rows": lambda s, host: s.measure_segments(*RUN_SEGMENTS, average=False, host=host)[1]},
        ["rn_md_raman_segments_at_device"])


@pytest.mark.parametrize("frames", list(SERIES))
def test_md_raman_replicates(library, frames):
    width, hop = SERIES[frames]
    alpha = _alpha_series(frames)
    _measure_case(
        library, f"measure_segment_replicates, {frames} frames, segments of {width} every {hop}",
        lambda arena: spectrum.DeviceMDRamanSpectrum(arena.tensor(alpha, what="alpha", row=9), TIMESTEP),
        {"replicates": lambda s, host: replicates.measure_segment_replicates(s, width, hop, replicates=5, seed=3,
                                                                             host=host)[1]},
        ["rn_md_raman_segment_replicates_device"])


@pytest.mark.parametrize("frames", list(SERIES))
def test_md_partial(library, frames):
    width, hop = SERIES[frames]
    incr = _increment_series(frames - 1, 3)
    _measure_case(
        library, f"DevicePartialMDRamanSpectrum, {frames} frames, 3 groups, segments of {width} every {hop}",
        lambda arena: spectrum.DevicePartialMDRamanSpectrum(arena.tensor(incr, what="increments", row=27), TIMESTEP),
        {"measure": lambda s, host: s.measure(host=host)[1],
         "measure_polarized": lambda s, host: s.measure_polarized(INCIDENT, SCATTERED, host=host)[1],
         "measure_segments": lambda s, host: s.measure_segments(width, hop, host=host)[1]},
        ["rn_md_raman_partial_device", "rn_md_raman_partial_segments_device"])


def _joined_increments(channels):
    """Increments of the joined frames of ``RUN_LENGTHS``; the row across the run boundary is never read: it holds NaN."""
    incr = _increment_series(sum(RUN_LENGTHS) - 1, channels)
    incr[RUN_LENGTHS[0] - 1] = np.nan
    return incr


def test_md_partial_ensemble(library):
    incr = _joined_increments(3)
    _measure_case(
        library, f"DevicePartialMDRamanEnsemble, one tensor with run_lengths {RUN_LENGTHS}, NaN across the boundary",
        lambda arena: spectrum.DevicePartialMDRamanEnsemble(arena.tensor(incr, what="increments", row=27), TIMESTEP,
                                                            RUN_LENGTHS),
        {"measure_segments": lambda s, host: s.measure_segments(*RUN_SEGMENTS, host=host)[1],
         "measure_segments rows": lambda s, host: s.measure_segments(*RUN_SEGMENTS, average=False, host=host)[1]},
        ["rn_md_raman_partial_segments_device"])


def _vdos_methods(width, hop):
    return {"measure_segments": lambda s, host: s.measure_segments(width, hop, host=host)[1],
            "measure_segments rows": lambda s, host: s.measure_segments(width, hop, average=False, host=host)[1]}


@pytest.mark.parametrize("frames", list(SERIES))
def test_md_vdos(library, frames):
    width, hop = SERIES[frames]
    positions, lattices, masses = _position_series(frames)
    labels = np.array([0, 1, 0, 1, 1])
    _measure_case(
        library, f"DeviceVibrationalDensityOfStates, {frames} frames, 5 atoms, 2 groups, a lattice per frame",
        lambda arena: spectrum.DeviceVibrationalDensityOfStates(
            arena.tensor(positions, what="positions", row=15), TIMESTEP, arena.tensor(lattices, what="lattices", row=9),
            masses, labels, 2),
        {"measure": lambda s, host: s.measure(host=host)[1], **_vdos_methods(width, hop)}, ["rn_md_vdos_device"])


def test_md_vdos_ensemble(library):
    positions, lattices, masses = _position_series(sum(RUN_LENGTHS))
    _measure_case(
        library, f"DeviceVibrationalDensityOfStatesEnsemble, one tensor with run_lengths {RUN_LENGTHS}",
        lambda arena: spectrum.DeviceVibrationalDensityOfStatesEnsemble(
            arena.tensor(positions, what="positions", row=15), TIMESTEP, arena.tensor(lattices, what="lattices", row=9),
            masses, run_lengths=RUN_LENGTHS),
        _vdos_methods(*RUN_SEGMENTS), ["rn_md_vdos_device"])


@pytest.mark.parametrize("frames", list(SERIES))
def test_md_mode_vdos(library, frames):
    width, hop = SERIES[frames]
    positions, lattices, masses = _position_series(frames)
    vectors = np.random.default_rng(9).normal(size=(4, 5, 3))
    _measure_case(
        library, f"DeviceModeVibrationalDensityOfStates, {frames} frames, 5 atoms, 4 modes, a lattice per frame",
        lambda arena: spectrum.DeviceModeVibrationalDensityOfStates(
            arena.tensor(positions, what="positions", row=15), TIMESTEP, arena.tensor(lattices, what="lattices", row=9),
            vectors, masses),
        {"measure": lambda s, host: s.measure(host=host)[1], **_vdos_methods(width, hop)}, ["rn_md_mode_vdos_device"])


def _all_bins(frames_per_segment):
    """One band over every bin of segments of that many frames, and one over the first bin alone."""
    n = frames_per_segment - 1
    axis = (np.fft.fftfreq(n, TIMESTEP) * spectrum._PER_FS_TO_CM1)[1:(n + 1) // 2]
    return np.array([[0.0, 2.0 * axis[-1]], [0.0, 1.5 * axis[0]]])


@pytest.mark.parametrize("frames", list(SERIES))
def test_md_modes(library, frames):
    width, hop = SERIES[frames]
    incr = _increment_series(frames - 1, 3, seed=1)
    _measure_case(
        library, f"DeviceModeMDRamanSpectrum, {frames} frames, 3 channels, segments of {width} every {hop}",
        lambda arena: spectrum.DeviceModeMDRamanSpectrum(arena.tensor(incr, what="increments", row=27), TIMESTEP),
        {"measure": lambda s, host: s.measure(host=host)[1],
         "measure_polarized": lambda s, host: s.measure_polarized(INCIDENT, SCATTERED, host=host)[1],
         "measure_segments": lambda s, host: s.measure_segments(width, hop, host=host)[1],
         "measure_interference": lambda s, host: s.measure_interference(_all_bins(frames), host=host)[1],
         "measure_interference of segments": lambda s, host: s.measure_interference(_all_bins(width), width, hop,
                                                                                      host=host)[1]},
        ["rn_md_raman_modes_device", "rn_md_raman_mode_matrix_device"])


def test_md_modes_ensemble(library):
    incr = _joined_increments(3)
    _measure_case(
        library, f"DeviceModeMDRamanEnsemble, one tensor with run_lengths {RUN_LENGTHS}, NaN across the boundary",
        lambda arena: spectrum.DeviceModeMDRamanEnsemble(arena.tensor(incr, what="increments", row=27), TIMESTEP,
                                                         RUN_LENGTHS),
        {"measure_segments": lambda s, host: s.measure_segments(*RUN_SEGMENTS, host=host)[1],
         "measure_interference": lambda s, host: s.measure_interference(_all_bins(RUN_SEGMENTS[0]), *RUN_SEGMENTS,
                                                                        host=host)[1]},
        ["rn_md_raman_modes_device", "rn_md_raman_mode_matrix_device"])


# ----------------------------------------------------------------------------- line-shape fits
def _fit_arrays(fits):
    """The arrays of a fit result, by field name."""
    return {field.name: getattr(fits, field.name) for field in dataclasses.fields(fits)
            if isinstance(getattr(fits, field.name), np.ndarray)}


def _fit_windows(capacity):
    """Five fits (a table that ends inside a workgroup of four waves) on windows of 63, 65 and ``capacity + 1`` bins, one
    per row; the last window ends on the last bin of the last row.  ``(bins, [(first, n)])``."""
    sizes = [63, 65, capacity + 1, 65, 63]
    bins = capacity + 24
    firsts = [3, 8, 5, 11, bins - 63]
    return bins, list(zip(firsts, sizes))


@pytest.mark.parametrize("kind", ["lorentzians", "peaks"])
def test_line_shape_fits(library, kind):
    from tests.lineshape_cases import axis, lorentzian, window
    from tests.peakfit_cases import axis_from, model as peaks_model
    if kind == "lorentzians":
        from tests.lineshape_cases import fits_deviation
        from tests.test_lineshape_gpu import NOISY_BOUND as bound
        bins, table = _fit_windows(lineshape.window_capacity())
        w = axis(bins)
    else:
        from tests.peakfit_cases import fits_deviation as peaks_deviation
        from tests.test_peakfit_gpu import NOISY_MEASURED
        bound = 20.0 * NOISY_MEASURED[2]
        bins, table = _fit_windows(peakfit.window_capacity())
        w = axis_from(2048.0, bins)
    rows, windows, centres = np.zeros((len(table), bins)), [], []
    for f, (first, n) in enumerate(table):
        g = n / 12.0
        if kind == "lorentzians":
            rows[f, first:first + n] = lorentzian(n, 1.37 * 10.0 ** (f - 2), 0.5 * (n - 1) + 0.3, g, 0.1 * 10.0 ** (f - 2))
        else:
            scale = 1.37 * 10.0 ** (f - 2)
            x0 = np.array([0.3 * n + 0.2, 0.7 * n - 0.3])
            rows[f, first:first + n] = peaks_model(n, [(scale, x0[0], g), (0.6 * scale, x0[1], 0.8 * g)], 0.1 * scale, 0.0,
                                                   "lorentzian", 2048.0 + first)
            centres.append(w[first] + (w[1] - w[0]) * (x0 + np.array([0.2, -0.3]) * g))
        windows.append(window(w, first, n))
    windows, centres = np.array(windows), np.array(centres)
    assert table[-1][0] + table[-1][1] == bins

    def fit(source, device=None):
        if kind == "lorentzians":
            return lineshape.fit_lorentzians(w, source, windows, device=device)
        return peakfit.fit_peaks_multi(w, source, windows, centres, device=device)

    host = lineshape.fit_lorentzians_host(w, rows, windows) if kind == "lorentzians" else peakfit.fit_peaks_host(
        w, rows, windows, centres)
    np.testing.assert_array_equal(host.status, 0)

    def call(arena):
        tensor = arena.tensor(rows, what="rows", row=bins)
        with arena.host_results(lineshape if kind == "lorentzians" else peakfit):
            return _fit_arrays(fit(tensor))

    def reference(r0):
        device = fit(torch.tensor(rows, device=DEVICE))
        np.testing.assert_array_equal(device.status, 0)
        for name, value in _fit_arrays(device).items():
            assert_same_bits(r0[name], value, name)
        deviation = fits_deviation(w, device, host) if kind == "lorentzians" else peaks_deviation(device, host)
        assert deviation.max() <= bound

    run_case(library, f"{kind}: 5 fits on windows of {[n for _, n in table]} bins, rows of {bins}", call, reference,
             ["rn_lineshape_fit_device" if kind == "lorentzians" else "rn_peakfit_fit_device"], host_results=3)
