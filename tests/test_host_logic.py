"""Host-side logic of the product (no GPU): graph construction, API contract, spectra,
C-ABI symbol table."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from ramannoodle_amd import _lib
from ramannoodle_amd.dynamics import Phonons, Trajectory
from ramannoodle_amd.exceptions import DeviceError
from ramannoodle_amd.pmodel import PotGNN, graph as G
from ramannoodle_amd.pmodel import polarizability_tensors_to_vectors, polarizability_vectors_to_tensors
from ramannoodle_amd.spectrum import (MDRamanSpectrum, PhononRamanSpectrum, calc_signal_spectrum,
                                      convolve_spectrum, get_bose_einstein_correction,
                                      get_laser_correction)
from ramannoodle_amd.structure import ReferenceStructure, apply_pbc
from tests.conftest import ROOT, load_golden
from tests.helpers import product_model_from_golden


# ----------------------------------------------------------------------------- graph
def test_radius_graph_bit_exact(golden):
    name, g = golden
    edges = G.radius_graph_pbc(g["lattice"], g["positions"], float(g["hp"][0]))
    np.testing.assert_array_equal(edges, g["ref_edge_indexes"][1:])
    # sorted by (a, b), no self loops
    key = edges[0] * len(g["atomic_numbers"]) + edges[1]
    assert np.all(np.diff(key) > 0) and np.all(edges[0] != edges[1])


def test_reference_order_triplets_bit_exact(golden):
    name, g = golden
    trip = G.reference_order_triplets(g["ref_edge_indexes"][1:], len(g["atomic_numbers"]))
    for mine, key in zip(trip, ["i", "j", "idx_i", "idx_j", "idx_k", "slot5", "slot6"]):
        np.testing.assert_array_equal(mine, g["trip/" + key])


def test_atom_type_map(golden):
    name, g = golden
    np.testing.assert_array_equal(G.atom_type_map(g["atomic_numbers"]), g["atom_type_map"])


def test_margin_around_cutoff(golden):
    """Fixtures keep a >= 1e-4 A gap around the cutoff, so edge lists cannot flip on
    float32 round-off (SURVEY hard part 4)."""
    name, g = golden
    lat, pos = g["lattice"], g["positions"]
    d = pos[None] - pos[:, None]
    d = np.where(d % 1 > 0.5, d % 1 - 1, d % 1) @ lat
    dist = np.sqrt((d**2).sum(-1))
    np.fill_diagonal(dist, 1e9)
    assert np.abs(dist - float(g["hp"][0])).min() > 1e-4


# ----------------------------------------------------------------------------- model shell
def _ref():
    g = load_golden("triclinic20")
    return ReferenceStructure([int(z) for z in g["atomic_numbers"]], g["lattice"], g["positions"])


@pytest.mark.parametrize(
    "args, message",
    [
        ((-2.3, 5, 5, 5, 5, 5), "invalid cutoff: -2.3 <= 0"),
        ((2.3, -5, 5, 5, 5, 5), "invalid size_node_embedding: -5 <= 0"),
        ((2.3, 5, 0, 5, 5, 5), "invalid size_edge_embedding: 0 <= 0"),
        ((2.3, 5, 5, -1, 5, 5), "invalid num_message_passes: -1 <= 0"),
        ((2.3, 5, 5, 5, -0.5, 5), "invalid gaussian_filter_start: -0.5 < 0"),
        ((2.3, 5, 5, 5, 3, 2), "invalid gaussian_filter_end: 2 <= gaussian_filter_start"),
    ],
)
def test_constructor_validation_messages(args, message):
    """Same six messages the reference pins (test/tests/torch/test_gnn.py:196-301)."""
    with pytest.raises(ValueError, match=re.escape(message)):
        PotGNN(_ref(), *args, np.zeros((3, 3)), np.ones((3, 3)))


def test_constructor_shape_errors():
    with pytest.raises(ValueError, match=re.escape("mean_polarizability has wrong shape: (3,) != (3,3)")):
        PotGNN(_ref(), 3.0, 4, 4, 1, 0, 5, np.zeros(3), np.ones((3, 3)))
    with pytest.raises(TypeError, match="stddev_polarizability should have type ndarray, not list"):
        PotGNN(_ref(), 3.0, 4, 4, 1, 0, 5, np.zeros((3, 3)), [1, 2, 3])


def test_state_dict_layout_matches_reference(golden):
    name, g = golden
    model = product_model_from_golden(g)
    want = [(k[3:], g[k].shape) for k in g.files if k.startswith("sd/")]
    got = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    assert got == want
    assert model.gauss_coefficient == pytest.approx(float(g["gauss_coefficient"]), rel=0, abs=0)
    np.testing.assert_array_equal(model.ref_edge_indexes, g["ref_edge_indexes"])
    blob = model._weights_blob()
    cfg = _lib.Config(model.num_atoms, model.num_edges, model._num_atom_types, model._fn, model._fe,
                      model._passes, model.gauss_coefficient, 0, 0)
    assert blob.size == _lib.load().rn_potgnn_weight_count(ctypes.byref(cfg))


def test_same_seed_same_initial_weights_as_module_order():
    torch.manual_seed(3)
    a = PotGNN(_ref(), 3.0, 4, 6, 2, 0, 5, np.zeros((3, 3)), np.ones((3, 3))).state_dict()
    torch.manual_seed(3)
    b = PotGNN(_ref(), 3.0, 4, 6, 2, 0, 5, np.zeros((3, 3)), np.ones((3, 3))).state_dict()
    for k in a:
        assert torch.equal(a[k], b[k])


def test_wrong_positions_shape_is_value_error_before_any_device_work():
    model = product_model_from_golden(load_golden("triclinic20"))
    with pytest.raises(ValueError, match=re.escape("positions_batch has wrong shape: (2,5,3) != (_,20,3)")):
        model.calc_polarizabilities(np.zeros((2, 5, 3)))
    with pytest.raises(TypeError, match="positions_batch should have type ndarray, not list"):
        model.calc_polarizabilities([[1.0]])


def test_to_device_refuses_a_host_out_tensor_before_any_device_work():
    """``calc_polarizabilities_to_device`` hands ``out``'s pointer to the library, which writes ``S * 9`` doubles through it
    on the device: a CPU tensor is refused with ``ValueError`` before the handle is created (so on any machine, with or
    without a GPU), and is left untouched."""
    g = load_golden("triclinic20")
    model = product_model_from_golden(g)
    pos = g["pos_batch"][:3]
    out = torch.full((3, 3, 3), -7.0, dtype=torch.float64)
    with pytest.raises(ValueError, match="out lives on cpu"):
        model.calc_polarizabilities_to_device(pos, out=out)
    assert model._handle is None
    assert bool((out == -7.0).all())


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_no_device_fails_loudly():
    model = product_model_from_golden(load_golden("triclinic20"))
    with pytest.raises(DeviceError):
        model.calc_polarizabilities(load_golden("triclinic20")["pos_batch"])


def test_vector_tensor_maps():
    v = torch.arange(12.0).reshape(2, 6)
    t = polarizability_vectors_to_tensors(v)
    assert t.shape == (2, 3, 3) and torch.equal(t, t.transpose(1, 2))
    assert torch.equal(polarizability_tensors_to_vectors(t), v)
    with pytest.raises(ValueError):
        polarizability_vectors_to_tensors(torch.zeros(2, 5))


# ----------------------------------------------------------------------------- C ABI
def test_library_exports_every_declared_symbol():
    declared = set()
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):  # every header of the C ABI
        header = open(os.path.join(ROOT, "include", name)).read()
        header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
        declared |= set(re.findall(r"\b(rn_(?:potgnn|xdatcar|vasprun|host|md)_\w+)\s*\(", header))
    declared -= {"rn_potgnn_reduce_fn"}  # a function-pointer typedef, not an entry point
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    lib = ctypes.CDLL(_lib.library_path())
    for name in declared:
        assert hasattr(lib, name), name
    assert b"gfx950" in _lib.load().rn_potgnn_version()
    # ... and nothing else of the library's own: the dynamic symbols named rn_* are exactly what include/ declares (every
    # header, the entries without a ctypes signature too), and no C++ internal -- namespace rn, or anything that takes a
    # handle -- is exported next to them
    every = set()
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
        every |= set(re.findall(r"\b(rn_\w+)\s*\(", header))
    every -= {"rn_potgnn_reduce_fn"}
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert {s for s in exported if s.startswith("rn_")} == every, {s for s in exported if s.startswith("rn_")} ^ every
    mangled = sorted(s for s in exported if s.startswith("_Z"))
    demangled = subprocess.run(["c++filt"], input="\n".join(mangled), check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(demangled) == len(mangled)
    internal = [d for d in demangled if re.search(r"\brn::", d) or "rn_potgnn" in d]
    assert not internal, internal[:10]


def test_create_rejects_bad_arguments_without_touching_the_gpu():
    lib = _lib.load()
    cfg = _lib.Config(4, 2, 1, 200, 8, 1, -1.0, 0, 0)
    n = lib.rn_potgnn_weight_count(ctypes.byref(cfg))
    w = np.zeros(n, dtype=np.float32)
    ea = np.array([0, 1], dtype=np.int32)
    eb = np.array([1, 0], dtype=np.int32)
    ty = np.zeros(4, dtype=np.int32)
    lat = np.eye(3)
    h = ctypes.c_void_p()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    rc = lib.rn_potgnn_create(ctypes.byref(cfg), p(ea), p(eb), p(ty), p(lat), p(w), n, p(lat), p(lat),
                              ctypes.byref(h))
    assert rc == _lib.RN_ERR_UNSUPPORTED and b"128" in lib.rn_potgnn_last_error(None)
    cfg.size_node_embedding = 8
    n = lib.rn_potgnn_weight_count(ctypes.byref(cfg))
    w = np.zeros(n, dtype=np.float32)
    eb_bad = np.array([1, 1], dtype=np.int32)  # edge (1,1) is a self loop
    rc = lib.rn_potgnn_create(ctypes.byref(cfg), p(ea), p(eb_bad), p(ty), p(lat), p(w), n, p(lat),
                              p(lat), ctypes.byref(h))
    assert rc == _lib.RN_ERR_INVALID_ARGUMENT
    ea_unsorted = np.array([1, 0], dtype=np.int32)
    rc = lib.rn_potgnn_create(ctypes.byref(cfg), p(ea_unsorted), p(ea), p(ty), p(lat), p(w), n,
                              p(lat), p(lat), ctypes.byref(h))
    assert rc == _lib.RN_ERR_INVALID_ARGUMENT and b"sorted" in lib.rn_potgnn_last_error(None)
    rc = lib.rn_potgnn_create(ctypes.byref(cfg), p(ea), p(eb), p(ty), p(lat), p(w), n - 1, p(lat),
                              p(lat), ctypes.byref(h))
    assert rc == _lib.RN_ERR_INVALID_ARGUMENT


def test_bench_refuses_to_run_without_gpus():
    """bench.py on a machine without a GPU: no CPU fallback, and ``--gpus N`` checks the device count
    before it starts any rank."""
    import subprocess
    import sys
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a GPU-less machine")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--no-cpu"], capture_output=True, text=True,
                         timeout=300)
    assert one.returncode != 0 and "needs a GPU" in one.stderr
    two = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--no-cpu"],
                         capture_output=True, text=True, timeout=300)
    assert two.returncode != 0 and "only 0 GPU(s) visible" in two.stderr
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    clash = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "4", "--no-cpu"], env=env,
                           capture_output=True, text=True, timeout=300)
    assert clash.returncode != 0 and "does not match WORLD_SIZE=2" in clash.stderr


def test_model_copies_and_pickles_carry_host_state_only():
    """``copy.deepcopy(model)`` / ``torch.save(model)`` (both appear around the reference's training
    loop) work on the device model: parameters are copied, the device handle is not."""
    import copy
    import io
    import torch
    from bench import rocksalt
    from ramannoodle_amd.pmodel import PotGNN
    from ramannoodle_amd.structure import ReferenceStructure
    lattice, ref, zs = rocksalt(1, 1, 1)
    model = PotGNN(ReferenceStructure(list(zs), lattice, ref), 3.0, 5, 14, 2, 0.0, 5.0, np.eye(3), np.ones((3, 3)))
    model._handle = ctypes.c_void_p(1234)  # what a live handle looks like to copy / pickle
    try:
        twin = copy.deepcopy(model)
        buffer = io.BytesIO()
        torch.save(model, buffer)
    finally:
        model._handle = None
    buffer.seek(0)
    loaded = torch.load(buffer, weights_only=False)
    for other in (twin, loaded):
        assert other._handle is None and other.num_edges == model.num_edges
        for (ka, va), (kb, vb) in zip(model.state_dict().items(), other.state_dict().items()):
            assert ka == kb and torch.equal(va, vb)
        assert next(other.parameters()) is not next(model.parameters())
        assert isinstance(next(other.parameters()), torch.nn.Parameter)
        assert isinstance(other, torch.nn.Module)


def test_documented_size_limits_raise_not_implemented():
    """The two limits of the device model (DESIGN.md "Limits"): embedding sizes above 128, and
    more outgoing edges per atom than one LDS tile holds in float64 (147 at Fe = 64; the reference's
    ``radius_graph_pbc`` keeps one edge per ordered atom pair, so this needs > 147 atoms inside
    the cutoff sphere).  Both are refused at model creation with NotImplementedError, before
    any device work."""
    from bench import rocksalt
    from ramannoodle_amd.pmodel import PotGNN
    from ramannoodle_amd.structure import ReferenceStructure
    lattice, ref, zs = rocksalt(1, 1, 1)
    small = ReferenceStructure(list(zs), lattice, ref)
    unit = (np.eye(3), np.ones((3, 3)))
    for fn, fe in ((129, 8), (8, 129)):
        model = PotGNN(small, 3.0, fn, fe, 1, 0.0, 5.0, *unit)
        with pytest.raises(NotImplementedError, match="embedding sizes above 128 are not supported"):
            model.calc_polarizabilities(ref[None])
    lattice, ref, zs = rocksalt(4, 4, 2)
    dense = PotGNN(ReferenceStructure(list(zs), lattice, ref), 7.9, 64, 64, 1, 0.0, 5.0, *unit)
    assert dense.num_edges / dense.num_atoms > 149
    with pytest.raises(NotImplementedError,
                       match=r"outgoing edges; more than 147 per atom is unsupported for size_edge_embedding=64"):
        dense.calc_polarizabilities(ref[None])
    # the same graph is accepted at a width whose rows fit (554 per atom at Fe <= 16): creation then
    # proceeds to the device probe, which is what fails on a machine without a GPU
    import torch
    if not torch.cuda.is_available():
        from ramannoodle_amd.exceptions import DeviceError
        ok = PotGNN(ReferenceStructure(list(zs), lattice, ref), 7.9, 8, 16, 1, 0.0, 5.0, *unit)
        with pytest.raises(DeviceError, match="no usable HIP device"):
            ok.calc_polarizabilities(ref[None])


# ----------------------------------------------------------------------------- spectra
def test_phonon_spectrum_matches_reference():
    g = load_golden("triclinic20")
    spec = PhononRamanSpectrum(g["ph/wavenumbers"], g["ph/raman_tensors"])
    w, i = spec.measure()
    np.testing.assert_array_equal(w, g["ph/wavenumbers"])
    np.testing.assert_allclose(i, g["ph/int_raw"], rtol=1e-13)
    w, i = spec.measure(laser_correction=True, laser_wavelength=532,
                        bose_einstein_correction=True, temperature=300)
    np.testing.assert_allclose(i, g["ph/int_corr"], rtol=1e-13)
    with pytest.raises(NotImplementedError):
        spec.measure(orientation=np.eye(3))


def test_md_spectrum_matches_reference():
    g = load_golden("triclinic20")
    spec = MDRamanSpectrum(g["md/alpha_ts"], float(g["md/timestep"]))
    w, i = spec.measure()
    np.testing.assert_allclose(w, g["md/wavenumbers"], rtol=1e-14)
    np.testing.assert_allclose(i, g["md/int_raw"], rtol=1e-10, atol=1e-12 * np.abs(g["md/int_raw"]).max())
    w, i = spec.measure(laser_correction=True, laser_wavelength=532,
                        bose_einstein_correction=True, temperature=300)
    np.testing.assert_allclose(i, g["md/int_corr"], rtol=1e-10, atol=1e-12 * np.abs(g["md/int_corr"]).max())
    s = g["md/alpha_ts"].shape[0]
    assert w.shape == (int(np.ceil((s - 1) / 2)) - 1 + ((s - 1) % 2 == 0) * 0,) or w.size > 0


def test_signal_spectrum_length():
    """Output length ceil(S/2) (test/tests/test_trajectory_spectrum.py:18-32)."""
    for s in (40, 51):
        w, i = calc_signal_spectrum(np.random.default_rng(0).normal(size=s), 1.0)
        assert w.shape == i.shape == (int(np.ceil(s / 2)),)


def test_corrections_and_convolution_errors():
    w = np.array([100.0, 200.0])
    with pytest.raises(ValueError, match="invalid temperature: -1 <= 0"):
        get_bose_einstein_correction(w, -1)
    with pytest.raises(TypeError, match="temperature should have type float, not list"):
        get_bose_einstein_correction(w, [])
    with pytest.raises(ValueError, match="invalid laser_wavenumber: 0 <= 0"):
        get_laser_correction(w, 0)
    with pytest.raises(ValueError, match="unsupported convolution type: triangle"):
        convolve_spectrum(w, w, "triangle")
    ow, oi = convolve_spectrum(w, np.array([1.0, 2.0]), "gaussian", 5)
    assert oi.sum() * (ow[1] - ow[0]) == pytest.approx(3.0, rel=1e-3)
    ow, oi = convolve_spectrum(w, np.array([1.0, 2.0]), "lorentzian", 5, out_wavenumbers=np.linspace(0, 300, 7))
    assert ow.shape == oi.shape == (7,)


def test_convolve_spectrum_against_the_reference_tests_known_answers():
    """The known-answer vectors of the reference's own ``test_convolve_intensities``
    (``test/tests/test_phonon_spectrum.py:404-447``, data under tests/golden/ref_spectrum), with
    that test's tolerance (``np.allclose``)."""
    base = os.path.join(os.path.dirname(__file__), "golden", "ref_spectrum")
    known = np.load(os.path.join(base, "known_spectrum.npz"))
    for function in ("gaussian", "lorentzian"):
        expected = np.load(os.path.join(base, f"known_{function}_spectrum.npz"))
        w, i = convolve_spectrum(known["wavenumbers"], known["intensities"], function)
        assert np.allclose(w, expected["wavenumbers"])
        assert np.allclose(i, expected["intensities"])
        np.testing.assert_allclose(i, expected["intensities"], rtol=1e-9, atol=1e-12 * np.abs(expected["intensities"]).max())


@pytest.mark.parametrize("wavenumbers,intensities,function,width,out_wavenumbers,exception_type,in_reason", [
    # the table of the reference's test_convolve_intensities_exception (test_phonon_spectrum.py:450-541)
    (np.array([1, 2, 3]), [0, 3, 0], "gaussian", 5, None, TypeError, "intensities should have type ndarray, not list"),
    ([1, 2, 3], np.array([0, 3, 0]), "gaussian", 5, None, TypeError, "wavenumbers should have type ndarray, not list"),
    (np.array([1, 2, 3, 4]), np.array([0, 3, 0]), "gaussian", 5, None, ValueError,
     "intensities has wrong shape: (3,) != (4,)"),
    (np.array([[1, 2, 3, 5], [2, 3, 4, 5]]), np.array([0, 3, 0, 4]), "gaussian", 5, None, ValueError,
     "wavenumbers has wrong shape: (2,4) != (_,)"),
    (np.array([1, 2, 3]), np.array([0, 3, 0]), "smoother", 5, None, ValueError, "unsupported convolution type: smoother"),
    (np.array([1, 2, 3]), np.array([0, 3, 0]), "gaussian", -4, None, ValueError, "invalid width: -4 <= 0"),
    (np.array([1, 2, 3]), np.array([0, 3, 0]), "gaussian", "not_a_int", None, TypeError,
     "width should have type float, not str"),
    (np.array([1, 2, 3]), np.array([0, 3, 0]), "gaussian", 5.0, np.array(([1, 2], [1, 2])), ValueError,
     "out_wavenumbers has wrong shape: (2,2) != (_,)"),
])
def test_convolve_spectrum_exceptions_as_the_reference(wavenumbers, intensities, function, width, out_wavenumbers,
                                                       exception_type, in_reason):
    import re
    with pytest.raises(exception_type, match=re.escape(in_reason)):
        convolve_spectrum(wavenumbers, intensities, function, width, out_wavenumbers)


@pytest.mark.parametrize("function,argument,exception_type,in_reason", [
    # test_get_bose_einstein_correction_exception / test_get_laser_correction (test_phonon_spectrum.py:544-618)
    (get_bose_einstein_correction, 300, TypeError, "wavenumbers should have type ndarray, not list"),
    (get_bose_einstein_correction, -300, ValueError, "invalid temperature: -300 <= 0"),
    (get_bose_einstein_correction, "string temperature", TypeError, "temperature should have type float, not str"),
    (get_laser_correction, 600, TypeError, "wavenumbers should have type ndarray, not list"),
    (get_laser_correction, -600, ValueError, "invalid laser_wavenumber: -600 <= 0"),
    (get_laser_correction, "string wavelength", TypeError, "laser_wavenumber should have type float, not str"),
])
def test_correction_exceptions_as_the_reference(function, argument, exception_type, in_reason):
    import re
    with pytest.raises(exception_type, match=re.escape(in_reason)):
        function([1, 2, 3], argument)


# ----------------------------------------------------------------------------- dynamics
class _Raises:
    def calc_polarizabilities(self, positions_batch):
        raise ValueError("positions_batch has wrong shape")


class _Linear:
    """Deterministic stand-in model: alpha = M . mean displacement (host only)."""

    def __init__(self, n):
        rng = np.random.default_rng(5)
        self.w = rng.normal(size=(n * 3, 6))

    def calc_polarizabilities(self, positions_batch):
        v = positions_batch.reshape(positions_batch.shape[0], -1) @ self.w
        return v[:, [[0, 3, 4], [3, 1, 5], [4, 5, 2]]]


def test_dynamics_constructor_and_incompatibility_errors():
    ref = np.zeros((4, 3))
    with pytest.raises(ValueError, match=re.escape("displacements has wrong shape: (2,3,3) != (2,4,3)")):
        Phonons(ref, np.array([1.0, 2.0]), np.zeros((2, 3, 3)))
    ph = Phonons(ref, np.array([1.0, 2.0]), np.zeros((2, 4, 3)))
    with pytest.raises(ValueError, match="polarizability_model and phonons are incompatible"):
        ph.get_raman_spectrum(_Raises())
    with pytest.raises(ValueError, match="timestep must be positive"):
        Trajectory(np.zeros((3, 4, 3)), 0)
    with pytest.raises(TypeError, match="timestep should have type float, not list"):
        Trajectory(np.zeros((3, 4, 3)), [])
    tr = Trajectory(np.zeros((3, 4, 3)) + 1.25, 1.0)
    assert np.allclose(tr.positions_ts, 0.25) and len(tr) == 3 and tr[1].shape == (4, 3)
    with pytest.raises(IndexError, match="trajectory index out of bounds"):
        tr[7]
    with pytest.raises(ValueError, match="polarizability_model and trajectory are incompatible"):
        tr.get_raman_spectrum(_Raises())


def test_phonon_finite_difference_divides_by_delta_not_two_delta():
    n = 4
    model = _Linear(n)
    rng = np.random.default_rng(1)
    ref, disp = rng.uniform(size=(n, 3)), rng.normal(size=(3, n, 3))
    spec = Phonons(ref, np.array([10.0, 20.0, 30.0]), disp).get_raman_spectrum(model)
    expect = 2.0 * (disp.reshape(3, -1) @ model.w)[:, [[0, 3, 4], [3, 1, 5], [4, 5, 2]]]
    np.testing.assert_allclose(spec.raman_tensors, expect, rtol=1e-9, atol=1e-9)


def test_apply_pbc():
    x = np.array([[-0.25, 1.5, 0.0]])
    np.testing.assert_allclose(apply_pbc(x), [[0.75, 0.5, 0.0]])
    with pytest.raises(TypeError):
        apply_pbc("nope")


def test_parameters_apply_and_modes():
    """torch-facing surface of the model shell: Parameters for torch.optim, the notebook's
    `model.apply(init_fn)` idiom (machine-learning.ipynb:198-206), train/eval flags."""
    model = product_model_from_golden(load_golden("triclinic20"))
    assert isinstance(model, torch.nn.Module)  # like the reference's (_gnn.py:418-421)
    params = list(model.parameters())
    assert all(isinstance(p, torch.nn.Parameter) for p in params)
    assert sum(p.numel() for p in params) == 4500  # the reference's parameter count for this model
    names = [k for k, _ in model.named_parameters()]
    assert "_edge_embedding.offset" not in names and "_to_polarizability_embedding.1.running_mean" not in names

    def init_biases(m):
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.uniform_(m.bias, -0.5, 0.5)

    def init_weights(m):
        if isinstance(m, torch.nn.Linear) or isinstance(m, torch.nn.Embedding):
            torch.nn.init.normal_(m.weight, mean=0, std=1)

    before = {k: v.clone() for k, v in model.state_dict().items()}  # (torch's state_dict() aliases the parameters)
    torch.manual_seed(1)
    model.apply(init_biases).apply(init_weights)
    after = {k: v.clone() for k, v in model.state_dict().items()}
    assert not torch.equal(before["_node_embedding.0.weight"], after["_node_embedding.0.weight"])
    assert not torch.equal(before["_edge_blocks.1.c3_linear.bias"], after["_edge_blocks.1.c3_linear.bias"])
    assert torch.equal(before["_node_blocks.0.c1_norm.weight"], after["_node_blocks.0.c1_norm.weight"])
    assert float(after["_to_polarizability_embedding.5.bias"].abs().max()) <= 0.5
    # load_state_dict keeps the Parameter objects (optimisers stay valid)
    model.load_state_dict(before)
    assert all(a is b for a, b in zip(params, model.parameters()))
    assert model.training and not model.eval().training and model.train().training
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    next(model.parameters()).grad = torch.ones_like(next(model.parameters()))
    opt.step()
    assert not torch.equal(model.state_dict()["_node_embedding.0.weight"], before["_node_embedding.0.weight"])


def test_reset_parameters():
    """(reference: test/tests/torch/test_gnn.py:116-120)"""
    model = product_model_from_golden(load_golden("triclinic20"))
    before = {k: v.clone() for k, v in model.state_dict().items()}
    params = list(model.parameters())
    torch.manual_seed(11)
    model.reset_parameters()
    after = model.state_dict()
    assert not torch.equal(before["_node_blocks.0.c1_linear.weight"], after["_node_blocks.0.c1_linear.weight"])
    assert torch.equal(after["_node_blocks.1.final_norm.weight"], torch.ones(8))
    assert torch.equal(after["_to_polarizability_embedding.1.running_var"], torch.ones(12))
    assert all(a is b for a, b in zip(params, model.parameters()))
    torch.manual_seed(11)
    from ramannoodle_amd.pmodel import PotGNN
    g = load_golden("triclinic20")
    fresh = PotGNN(_ref(), 3.0, 8, 12, 2, 0.0, 4.0, g["mean"], g["std"]).state_dict()
    for k in after:
        assert torch.equal(after[k], fresh[k]), k


def test_config1_plumbing_linear_model_phonon_spectrum():
    """BASELINE config 1 (CPU plumbing, no GPU): an 8-atom rocksalt cell, a seeded linear
    ``PolarizabilityModel`` (what an order-1 P1 InterpolationModel evaluates,
    ``pmodel/_interpolation.py:239-244``) and 24 modes through ``Phonons.get_raman_spectrum`` ->
    ``PhononRamanSpectrum.measure``, against what the reference's own classes produced
    (tests/golden/make_golden_r2.py).  Exercises the generic per-mode loop of
    ``dynamics/_phonon.py:93-106`` (the model has no ``calc_raman_tensors``)."""
    from ramannoodle_amd.abstract import PolarizabilityModel
    from ramannoodle_amd.dynamics import Phonons

    g = load_golden("config1_plumbing")

    class LinearModel(PolarizabilityModel):
        def __init__(self):
            self.calls = 0

        def calc_polarizabilities(self, positions_batch):
            self.calls += 1
            d = (positions_batch - g["positions"][None]).reshape(positions_batch.shape[0], -1)
            return g["alpha0"][None] + np.einsum("sk,kij->sij", d, g["coeff"])

    model = LinearModel()
    spectrum = Phonons(g["positions"], g["wavenumbers"], g["displacements"]).get_raman_spectrum(model)
    assert model.calls == 2 * 24  # +-delta per mode, batch of one each (the reference's loop)
    np.testing.assert_allclose(spectrum.raman_tensors, g["raman_tensors"], rtol=0,
                               atol=1e-12 * np.abs(g["raman_tensors"]).max())
    w, i = spectrum.measure()
    np.testing.assert_array_equal(w, g["out_wavenumbers"])
    np.testing.assert_allclose(i, g["int_raw"], rtol=1e-10)
    w, i = spectrum.measure(laser_correction=True, laser_wavelength=522, bose_einstein_correction=True,
                            temperature=300)
    np.testing.assert_allclose(i, g["int_corr"], rtol=1e-10)
    # a model that rejects the shape surfaces as the reference's "incompatible" ValueError
    class Wrong(PolarizabilityModel):
        def calc_polarizabilities(self, positions_batch):
            raise ValueError("positions_batch has wrong shape")

    with pytest.raises(ValueError, match="incompatible"):
        Phonons(g["positions"], g["wavenumbers"], g["displacements"]).get_raman_spectrum(Wrong())


def test_role_split_producers_leave_in_flight_registers_alone():
    """The producers of the role-specialised EdgeBlock (``csrc/kernels_edge_ps.hip``) load their node terms in inline assembly
    and wait for them with a hand-counted ``s_waitcnt vmcnt(5)`` behind the first product.  ``tools/check_ps_isa.py`` compiles
    the file and checks in the ISA of every instantiation that nothing reads, copies or spills those registers before the
    wait (a tied-operand copy in front of a wait on a second code path did exactly that once)."""
    import shutil
    import subprocess
    import sys
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "check_ps_isa.py")], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 violation(s)" in out.stdout and "0 in-flight loads" not in out.stdout


def _tile_rows(atoms, degree):
    """First / end source row of every destination of a tile of `atoms` atoms with `degree` in- and out-edges each."""
    rb = np.repeat(np.arange(atoms) * degree, degree).astype(np.int32)
    return rb, (rb + degree).astype(np.int32)


def test_role_split_schedule_check_on_the_host():
    """The schedule check behind the role-specialised EdgeBlock (``rn_potgnn_debug_ps_schedule``, host-only: it is what
    decides at model creation whether a graph takes ``csrc/kernels_edge_ps.hip``, and with how much lookahead).  On the
    benchmark cell's tile -- 8 atoms with 18 in- and out-edges, 9 rounds of 16 destinations -- the ring must
    hold 5 / 6 / 7 tiles for 1 / 2 / 3 rounds still reading when a step rewrites it, a round's window spans at most 3
    tiles, and a 47-neighbour atom (TiO2 at 5 A) does not fit the 8-tile ring at all."""
    import ctypes as C
    from ramannoodle_amd import _lib
    lib = _lib.load()

    def check(rb, re, back, ring):
        window = C.c_int32(-1)
        rc = lib.rn_potgnn_debug_ps_schedule(C.c_void_p(rb.ctypes.data), C.c_void_p(re.ctypes.data), len(rb), back, ring,
                                             C.byref(window))
        assert rc in (0, 1), rc
        return bool(rc), window.value

    rb, re = _tile_rows(8, 18)
    need = {}
    for back in (1, 2, 3):
        need[back] = next(ring for ring in range(1, 17) if check(rb, re, back, ring)[0])
        assert all(check(rb, re, back, ring)[0] for ring in range(need[back], 17))  # (monotone in the capacity)
    assert need == {1: 5, 2: 6, 3: 7}
    assert check(rb, re, 3, 8) == (True, 3) and check(rb, re, 3, 7) == (True, 3) and not check(rb, re, 3, 6)[0]
    # fewer neighbours (a round of 16 destinations then spans three or four atoms); a ragged tile is decided without a device too
    assert check(*_tile_rows(16, 6), 3, 8) == (True, 3)
    rng = np.random.default_rng(3)
    deg = rng.integers(1, 12, size=10)
    start = np.concatenate([[0], np.cumsum(deg)])
    rb_r = np.repeat(start[:-1], deg).astype(np.int32)
    re_r = np.repeat(start[1:], deg).astype(np.int32)
    assert check(rb_r, re_r, 2, 8)[0]
    # TiO2 at 5 A: 47 out-edges per atom -- a round's window spans seven tiles, two rounds in flight need nine
    assert check(*_tile_rows(4, 47), 2, 8) == (False, 7) and check(*_tile_rows(4, 47), 2, 9)[0]
    assert lib.rn_potgnn_debug_ps_schedule(None, None, 0, 2, 8, None) < 0


# ----------------------------------------------------------------------------- graph plans
_PLAN_GOLDEN = os.path.join(ROOT, "tests", "golden", "graph_plans.npz")
_PLAN_CACHE = {}


def _plans(group, num_cus):
    """Every case of knob group `group` through ``rn_potgnn_debug_plan`` in a child process (tests/plan_worker.py) whose
    environment holds exactly that group's knobs: name -> (shape, edge_a, edge_b, types, flat plan)."""
    import subprocess
    import sys
    import tempfile
    from tests.helpers import PLAN_KNOBS, plan_cases
    if (group, num_cus) not in _PLAN_CACHE:
        env = {k: v for k, v in os.environ.items() if not k.startswith("RN_POTGNN_") or k == "RN_POTGNN_LIB"}
        env.update({"RN_POTGNN_" + k: v for k, v in PLAN_KNOBS[group].items()})
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "plans.npz")
            run = subprocess.run([sys.executable, "-m", "tests.plan_worker", str(group), str(num_cus), out], cwd=ROOT,
                                 env=env, capture_output=True, text=True, timeout=600)
            assert run.returncode == 0, run.stdout + run.stderr
            flat = dict(np.load(out))
        cases = plan_cases(PLAN_KNOBS[group])
        assert sorted(flat) == sorted(c[0] for c in cases)
        _PLAN_CACHE[(group, num_cus)] = {name: (shape, ea, eb, types, flat[name]) for name, shape, ea, eb, types in cases}
    return _PLAN_CACHE[(group, num_cus)]


def _parse_plan(flat, n, e):
    """The layout documented at ``rn_potgnn_debug_plan`` in include/rn_potgnn.h."""
    plan = {"FnP": int(flat[0]), "FeP": int(flat[1])}
    i = 2
    for part in ("tile", "nt", "et", "bt", "pt"):
        length = int(flat[i])
        plan[part] = (flat[i + 1:i + 1 + length], tuple(int(v) for v in flat[i + 1 + length:i + 4 + length]))
        i += length + 4
    for key in ("nt_narrow", "na_num", "na_max_deg", "pt_back", "pt_gram", "T", "use_fused", "reserved0", "reserved1", "use_ps",
                "use_narrow", "use_node_fused", "use_readout_fused", "num_lanes"):
        plan[key] = int(flat[i])
        i += 1
    assert plan["reserved0"] == 0 and plan["reserved1"] == 0
    plan["head"] = flat[:i]
    for key, size in (("out_ptr", n + 1), ("in_ptr", n + 1), ("in_edge", e), ("in_pos", e), ("rev_edge", e), ("trip_off", e + 1)):
        plan[key] = flat[i:i + size]
        i += size
    assert i == len(flat)
    return plan


def _all_plan_groups(num_cus):
    from tests.helpers import PLAN_KNOBS, plan_group_name
    for group, knobs in enumerate(PLAN_KNOBS):
        for name, (shape, ea, eb, types, flat) in _plans(group, num_cus).items():
            yield plan_group_name(knobs) + "/" + name, shape, ea, eb, types, _parse_plan(flat, shape[0], shape[1])


def test_graph_plans_match_the_parent_commit():
    """The host-only planner (csrc/graph_plan.hip) chooses, element for element, the partitions, scalars and kernel family
    that ``rn_potgnn_create`` chose before planning moved out of it.  tests/golden/graph_plans.npz was recorded from that
    parent commit (c6d5589), not from this code: a throw-away patch (not committed) made the parent's ``rn_potgnn_create``
    write the array of ``rn_potgnn_debug_plan`` when it returned, over the case list of tests/helpers.py ``plan_cases`` --
    the fixtures' graphs, the benchmark cells at eight width pairs, 24 ragged graphs, and eleven knob variants in a
    process each.  The file was meant to be taken on an MI355X; no GPU could be had while this was written, so the patch
    also let the parent skip its device probe and device calls and take the CU count (256, an MI355X's, and the parent's
    own value when the query fails) from the environment: the planning code that ran is the parent's, unchanged, on a
    CPU (profiles/plan_refactor_ab.txt: the commit, the patch, the cases, the CU count).  ``num_cus`` is the recorded one,
    so this runs anywhere."""
    golden = np.load(_PLAN_GOLDEN)
    num_cus = int(golden["num_cus"])
    seen = set()
    for key, shape, ea, eb, types, plan in _all_plan_groups(num_cus):
        np.testing.assert_array_equal(plan["head"], golden[key], err_msg=key)
        seen.add(key)
    assert seen == set(golden.files) - {"num_cus", "parent_commit"} and len(seen) >= 4 + 24 + 20 + 22


def test_graph_plan_index_arrays_against_their_definitions():
    """out_ptr / in_ptr are the CSRs over source and destination, in_edge lists each destination's edges ascending, in_pos
    is its inverse, rev_edge[e] the id of (b -> a) or -1, trip_off the running count of b's out-edges other than the one
    back to a -- recomputed here in numpy; for the fixtures T is also the reference-order triplet count."""
    from tests.helpers import PLAN_FIXTURES
    for key, (n, e, _, _, _), ea, eb, types, plan in _all_plan_groups(256):
        ea64, eb64 = ea.astype(np.int64), eb.astype(np.int64)
        deg_out = np.bincount(ea, minlength=n)
        np.testing.assert_array_equal(plan["out_ptr"], np.concatenate([[0], np.cumsum(deg_out)]), err_msg=key)
        np.testing.assert_array_equal(plan["in_ptr"], np.concatenate([[0], np.cumsum(np.bincount(eb, minlength=n))]), err_msg=key)
        in_edge = np.argsort(eb, kind="stable")
        np.testing.assert_array_equal(plan["in_edge"], in_edge, err_msg=key)
        in_pos = np.empty(e, dtype=np.int64)
        in_pos[in_edge] = np.arange(e)
        np.testing.assert_array_equal(plan["in_pos"], in_pos, err_msg=key)
        ids = {(a, b): i for i, (a, b) in enumerate(zip(ea64.tolist(), eb64.tolist()))}
        rev = np.array([ids.get((b, a), -1) for a, b in zip(ea64.tolist(), eb64.tolist())])
        np.testing.assert_array_equal(plan["rev_edge"], rev, err_msg=key)
        per_edge = deg_out[eb] - (rev >= 0)
        np.testing.assert_array_equal(plan["trip_off"], np.concatenate([[0], np.cumsum(per_edge)]), err_msg=key)
        assert plan["T"] == per_edge.sum()
        if key.split("/")[1] in PLAN_FIXTURES:
            assert plan["T"] == len(G.reference_order_triplets(np.stack([ea64, eb64]), n)[2])


def test_graph_plan_partitions_hold_their_invariants():
    """Every partition of every case: ``begin`` runs from 0 to N and rises strictly, the three maxima are those of its tiles,
    ``pt_back`` lies in 2 .. 5 and the producers' schedule check accepts every tile of the role-specialised EdgeBlock at
    that lookahead and the matching ring (8 tiles; 7 with the Gram tables).  The ragged graphs are there for the planner's
    rarer branches, and this test checks that each is taken: (1) the atom-owning NodeBlock refused because it would run more
    than 1.2x the rounds (every even ``ragged``; the benchmark cells take it), (2) a greedy walk that gives one atom with
    more rows than the budget a tile of its own, (3) a search of the role-specialised tiles that stops because one tile
    holds the whole graph (E <= 1024 at 64 x 64: ``ragged04``, ``ragged20``), (4) such a search that ends without a partition
    (``ragged07``, ``ragged11``, ``ragged23``: out-degrees near 50 do not fit the ring)."""
    lib = _lib.load()
    hit = {"atom_refused": [], "atom_taken": [], "single_atom_over_budget": [], "one_tile": [], "no_ps_partition": []}
    for key, (n, e, _, _, _), ea, eb, types, plan in _all_plan_groups(256):
        out_ptr, in_ptr, in_edge = (plan[k].astype(np.int64) for k in ("out_ptr", "in_ptr", "in_edge"))
        for part in ("tile", "nt", "et", "bt", "pt"):
            begin, maxima = plan[part]
            if len(begin) == 0:
                assert maxima == (0, 0, 0) and part in ("et", "bt", "pt"), (key, part)
                continue
            assert begin[0] == 0 and begin[-1] == n and np.all(np.diff(begin) > 0), (key, part)
            rows_out, rows_in = np.diff(out_ptr[begin]), np.diff(in_ptr[begin])
            assert maxima == (rows_out.max(), rows_in.max(), np.diff(begin).max()), (key, part)
            # a greedy walk closes tile t because the first atom of tile t + 1 would exceed the budget, so the budget
            # lies below rows(t) + that atom's rows for every closed tile; a one-atom tile at or above that is over it
            by_in = part == "nt"
            if len(begin) > 2 and not (by_in and plan["nt_narrow"]) and not (part == "tile" and plan["use_narrow"]):
                rows, ptr = (rows_in, in_ptr) if by_in else (rows_out, out_ptr)
                bound = (rows[:-1] + (ptr[begin[1:-1] + 1] - ptr[begin[1:-1]])).min()
                if np.any((np.diff(begin) == 1) & (rows >= bound)):
                    hit["single_atom_over_budget"].append(key + ":" + part)
        assert 2 <= plan["pt_back"] <= 5, key
        begin = plan["pt"][0]
        for t in range(len(begin) - 1):
            dest = eb[in_edge[in_ptr[begin[t]]:in_ptr[begin[t + 1]]]]
            rb = (out_ptr[dest] - out_ptr[begin[t]]).astype(np.int32)
            re_ = (out_ptr[dest + 1] - out_ptr[begin[t]]).astype(np.int32)
            ok = lib.rn_potgnn_debug_ps_schedule(ctypes.c_void_p(rb.ctypes.data), ctypes.c_void_p(re_.ctypes.data), len(rb),
                                                 plan["pt_back"], 7 if plan["pt_gram"] else 8, None)
            assert ok == 1, (key, t)
        if key.startswith("default/") and plan["FnP"] == 64 and plan["FeP"] == 64:
            deg_in = np.diff(in_ptr)
            rounds_atom = sum(int(deg_in[i:i + 16].max()) for i in range(0, n, 16))
            rounds_row = int(((np.diff(in_ptr[plan["nt"][0]]) + 15) // 16).sum())
            if rounds_atom > 1.2 * rounds_row:
                assert plan["na_num"] == 0, key
                hit["atom_refused"].append(key)
            elif plan["na_num"] > 0:
                hit["atom_taken"].append(key)
            if e <= 1024:
                hit["one_tile"].append(key)
            if len(begin) == 0:
                hit["no_ps_partition"].append(key)
    assert all(hit.values()), hit


def test_sparse_structures_keep_their_degenerate_graphs_and_get_a_plan():
    """tests/helpers.py ``sparse_structures()`` -- what tests/test_sparse_graphs_gpu.py runs on -- have the graphs they are
    there for (those tests would pass trivially if a coordinate drifted): N, E, T, species, atoms without an edge, atoms
    of degree 1, destination edges without a triplet, the hub's degree, an edge-free atom alone in the second 16-atom
    tile.  Product graph code equals the oracle's bit for bit, and the planner accepts every one of them at every width
    pair of ``PLAN_WIDTHS`` with partitions that start at 0, end at N, never step back and hold every atom once."""
    from oracle import potgnn_oracle as O
    from tests.helpers import PLAN_WIDTHS, SPARSE_PROPERTIES, sparse_structures
    from tests.plan_worker import debug_plan
    lib = _lib.load()
    structures = sparse_structures()
    assert list(structures) == list(SPARSE_PROPERTIES) == ["dimer", "iso_dimer_iso", "chain5", "hub17", "molecules33"]
    for name, (lattice, positions, zs, cutoff) in structures.items():
        n = len(zs)
        edges = G.radius_graph_pbc(lattice, positions, cutoff)
        trip = G.reference_order_triplets(edges, n)
        degree = np.bincount(edges[0], minlength=n)
        np.testing.assert_array_equal(degree, np.bincount(edges[1], minlength=n), err_msg=name)  # (a -> b comes with b -> a)
        per_edge = np.bincount(trip[5], minlength=edges.shape[1])
        got = dict(N=n, E=edges.shape[1], T=len(trip[2]), K=len(set(zs)), edge_free=int((degree == 0).sum()),
                   triplet_less=int((per_edge == 0).sum()), degree_one=int((degree == 1).sum()))
        assert got == SPARSE_PROPERTIES[name], (name, got)
        o_edges, o_trip, o_map = O.build_topology(lattice, positions, zs, cutoff)
        np.testing.assert_array_equal(edges, o_edges.numpy()[1:], err_msg=name)
        assert len(trip) == len(o_trip) == 7
        for mine, ref in zip(trip, o_trip):
            assert mine.dtype == np.int64
            np.testing.assert_array_equal(mine, ref.numpy(), err_msg=name)
        tmap = G.atom_type_map(zs)
        np.testing.assert_array_equal(tmap, o_map.numpy(), err_msg=name)
        ea, eb = (np.ascontiguousarray(x, dtype=np.int32) for x in edges)
        types = np.ascontiguousarray(tmap[np.asarray(zs)], dtype=np.int32)
        for fn, fe in PLAN_WIDTHS:
            flat = debug_plan(lib, (n, len(ea), got["K"], fn, fe), ea, eb, types, 256)  # (asserts RN_OK)
            plan = _parse_plan(flat, n, len(ea))
            assert plan["T"] == got["T"], (name, fn, fe)
            for part in ("tile", "nt", "et", "bt", "pt"):
                begin, maxima = plan[part]
                if len(begin) == 0:
                    assert part in ("et", "bt", "pt"), (name, fn, fe, part)
                    continue
                assert begin[0] == 0 and begin[-1] == n and np.all(np.diff(begin) >= 0), (name, fn, fe, part, begin)
                owners = np.concatenate([np.arange(lo, hi) for lo, hi in zip(begin[:-1], begin[1:])])
                np.testing.assert_array_equal(owners, np.arange(n), err_msg=f"{name} {fn}/{fe} {part}")
                assert maxima[2] == np.diff(begin).max(), (name, fn, fe, part)
    chain = G.radius_graph_pbc(*structures["chain5"][:2], structures["chain5"][3])
    assert np.bincount(chain[0]).tolist() == [1, 2, 2, 2, 1]
    lattice, positions, zs, cutoff = structures["hub17"]
    degree = np.bincount(G.radius_graph_pbc(lattice, positions, cutoff)[0], minlength=17)
    assert degree[0] == 0 and degree[1] == 14 and degree[16] == 0 and degree[2:16].min() == 3 and degree[2:16].max() == 8


# ----------------------------------------------------------------------------- dense and uneven graphs
CU_LDS_BYTES = 160 * 1024
LDS_FAMILIES = ("edge_agg", "edge_bwd", "edge_narrow", "node_tiled", "edge_ps", "node_atom", "node_fused")
DEGREE_CAPS = {16: 554, 32: 292, 64: 147, 128: 71}  # padded edge width -> most out-edges per atom (DESIGN.md "Limits")


def _plan_lds(lib, shape, ea, eb, types, num_cus=256):
    """``rn_potgnn_debug_plan_lds``: (status, family -> (float32 bytes, float64 bytes), error text)."""
    n, e, k, fn, fe = shape
    cfg = _lib.Config(n, e, k, fn, fe, 2, -1.0, 0, 0)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    out, count = np.full(2 * len(LDS_FAMILIES), -1, dtype=np.int64), ctypes.c_size_t(0)
    rc = lib.rn_potgnn_debug_plan_lds(ctypes.byref(cfg), p(ea), p(eb), p(types), num_cus, p(out), out.size, ctypes.byref(count))
    if rc != _lib.RN_OK:
        return rc, None, lib.rn_potgnn_last_error(None).decode()
    assert count.value == out.size and np.all(out >= 0)
    return rc, {f: (int(out[2 * i]), int(out[2 * i + 1])) for i, f in enumerate(LDS_FAMILIES)}, ""


def _dense_graph(name):
    """(edge_a, edge_b, atom types, species) of one of ``dense_structures()``, by the product's host graph code."""
    from tests.helpers import dense_structures
    lattice, positions, zs, cutoff = dense_structures()[name]
    edges = G.radius_graph_pbc(lattice, positions, cutoff)
    tmap = G.atom_type_map(zs)
    ea, eb = (np.ascontiguousarray(x, dtype=np.int32) for x in edges)
    return ea, eb, np.ascontiguousarray(tmap[np.asarray(zs)], dtype=np.int32), int((tmap >= 0).sum())


def _dense_plan(lib, name, fn, fe):
    from tests.plan_worker import debug_plan
    ea, eb, types, k = _dense_graph(name)
    return _parse_plan(debug_plan(lib, (len(types), len(ea), k, fn, fe), ea, eb, types, 256), len(types), len(ea))


def _planned_edge_width(lib, fn, fe):
    """The padded edge width the library plans a model of these widths at: FeP of ``rn_potgnn_debug_plan`` on a two-atom graph."""
    from tests.plan_worker import debug_plan
    ea, eb = np.array([0, 1], dtype=np.int32), np.array([1, 0], dtype=np.int32)
    return int(debug_plan(lib, (2, 2, 1, fn, fe), ea, eb, np.zeros(2, dtype=np.int32), 256)[1])


def _star_ring(degree):
    """Atom 0 joined to atoms 1 .. degree, both ways, and those joined in a ring: a hub of that degree among atoms of
    degree 3, which the greedy tile walks pack many to a tile."""
    leaves = np.arange(1, degree + 1)
    after, before = leaves % degree + 1, (leaves - 2) % degree + 1
    pairs = np.concatenate([np.stack([np.zeros(degree, dtype=np.int64), leaves], 1), np.stack([leaves, np.zeros(degree, dtype=np.int64)], 1),
                            np.stack([leaves, after], 1), np.stack([leaves, before], 1)])
    pairs = np.unique(pairs, axis=0)  # (sorted by (a, b))
    return pairs[:, 0].astype(np.int32), pairs[:, 1].astype(np.int32), np.zeros(degree + 1, dtype=np.int32)


def test_dense_structures_keep_their_pinned_graphs():
    """tests/helpers.py ``dense_structures()`` -- what tests/test_dense_graphs_gpu.py runs on: N, E, T and the smallest and
    largest degree are the pinned ones; the hubs' degrees are exactly the caps of the widths they are named after; the
    float32 and the float64 edge lists agree, and no pair distance lies within 1e-3 A of the cutoff (the frames' noise is
    2e-3 of a cell edge in fractional terms only on paper: the graph is frozen from the reference positions); the
    product's graph code equals the oracle's bit for bit."""
    from oracle import potgnn_oracle as O
    from tests.helpers import BLOB_ATOMS, DENSE_PROPERTIES, HUB_SHELL, dense_structures
    structures = dense_structures()
    assert list(structures) == list(DENSE_PROPERTIES) == ["blob_gas", "blob_ring", "hub_cap128", "hub_cap64"]
    assert HUB_SHELL == {"hub_cap128": DEGREE_CAPS[128], "hub_cap64": DEGREE_CAPS[64]}
    for name, (lattice, positions, zs, cutoff) in structures.items():
        n = len(zs)
        assert cutoff == 3.0 and cutoff < 0.5 * min(np.linalg.norm(np.linalg.inv(lattice), axis=0) ** -1)  # (under half of every cell height)
        edges = G.radius_graph_pbc(lattice, positions, cutoff)
        np.testing.assert_array_equal(edges, G.radius_graph_pbc(lattice, positions, cutoff, dtype=np.float64), err_msg=name)
        f = positions[None] - positions[:, None]
        dist = np.linalg.norm((f - np.round(f)) @ lattice, axis=-1)[np.triu_indices(n, 1)]
        assert np.abs(dist - cutoff).min() > 1e-3, (name, np.abs(dist - cutoff).min())
        trip = G.reference_order_triplets(edges, n)
        degree = np.bincount(edges[0], minlength=n)
        np.testing.assert_array_equal(degree, np.bincount(edges[1], minlength=n), err_msg=name)
        got = dict(N=n, E=edges.shape[1], T=len(trip[2]), min_degree=int(degree.min()), max_degree=int(degree.max()))
        assert got == DENSE_PROPERTIES[name], (name, got)
        o_edges, o_trip, o_map = O.build_topology(lattice, positions, zs, cutoff)
        np.testing.assert_array_equal(edges, o_edges.numpy()[1:], err_msg=name)
        for mine, ref in zip(trip, o_trip):
            np.testing.assert_array_equal(mine, ref.numpy(), err_msg=name)
        np.testing.assert_array_equal(G.atom_type_map(zs), o_map.numpy(), err_msg=name)
        if name in BLOB_ATOMS:  # every 16-atom group mixes the ball's degree with the molecules'
            for i in range(0, n - 15, 16):
                assert degree[i:i + 16].max() == got["max_degree"] and degree[i:i + 16].min() <= 2, (name, i)
        else:  # the hub sits in the middle of the atom order
            assert int(degree.argmax()) == HUB_SHELL[name] // 2 and np.sort(degree)[-2] < degree.max() // 2


def test_dense_structures_reach_the_planner_branches_they_are_there_for():
    """The planner's size-dependent branches, by name, on geometric graphs that kernels then run on (the ``ragged`` cases
    above are graphs no geometry produces): the role-specialised ring refusing a graph with the fused path on; the
    atom-owning NodeBlock refused by the 1.2x rule; one-atom tiles at the degree cap; a narrow tile above 128 rows (the
    four-wave form); the reverse EdgeBlock with and without a partition of its own."""
    lib = _lib.load()
    ring = _dense_plan(lib, "blob_ring", 64, 64)
    assert ring["use_fused"] == 1 and ring["use_ps"] == 0 and len(ring["pt"][0]) == 0
    assert _dense_plan(lib, "blob_ring", 5, 14)["use_narrow"] == 1
    from tests.helpers import BLOB_ATOMS, dense_structures
    import tests.helpers as H
    smaller = dict(BLOB_ATOMS, blob_ring=BLOB_ATOMS["blob_ring"] - 1)  # (the smallest such ball: one atom fewer and the ring takes it)
    try:
        H.BLOB_ATOMS, kept = smaller, H.BLOB_ATOMS
        assert _dense_plan(lib, "blob_ring", 64, 64)["use_ps"] == 1
    finally:
        H.BLOB_ATOMS = kept
    assert dense_structures()["blob_ring"][1].shape[0] == BLOB_ATOMS["blob_ring"] + 35

    gas = _dense_plan(lib, "blob_gas", 64, 64)
    assert gas["use_fused"] == 1 and gas["use_ps"] == 1 and gas["use_node_fused"] == 1 and len(gas["bt"][0]) == 0
    assert gas["pt_back"] == 3 and gas["pt"][1] == (58, 58, 4)  # (DESIGN.md quotes the lookahead)
    deg_in = np.diff(gas["in_ptr"])
    rounds_atom = sum(int(deg_in[i:i + 16].max()) for i in range(0, len(deg_in), 16))
    rounds_row = int(((np.diff(gas["in_ptr"][gas["nt"][0]]) + 15) // 16).sum())
    assert gas["na_num"] == 0 and rounds_atom > 1.2 * rounds_row, (rounds_atom, rounds_row)

    for fn, fe in ((40, 100), (64, 128)):
        hub = _dense_plan(lib, "hub_cap128", fn, fe)
        assert (hub["FnP"], hub["FeP"]) == (64, 128) and hub["tile"][1] == (71, 71, 1) and len(hub["tile"][0]) == 73
    assert _dense_plan(lib, "hub_cap128", 64, 64)["use_ps"] == 1
    cap64 = _dense_plan(lib, "hub_cap64", 64, 64)
    assert cap64["tile"][1] == (147, 147, 1) and len(cap64["tile"][0]) == 149 and cap64["use_fused"] == 0 and len(cap64["bt"][0]) == 0
    assert _dense_plan(lib, "hub_cap64", 24, 20)["head"].tolist() == cap64["head"].tolist()  # (widened onto the same plan)
    narrow = _dense_plan(lib, "hub_cap64", 5, 14)
    assert narrow["use_narrow"] == 1 and narrow["tile"][1][:2] == (147, 147) and narrow["tile"][1][2] > 1 and len(narrow["bt"][0]) > 0
    assert _dense_plan(lib, "blob_gas", 5, 14)["tile"][1][0] <= 128  # (the two-wave form next to it)


def test_every_planned_kernel_fits_the_compute_unit():
    """Accepted => fits: for every graph ``rn_potgnn_create`` accepts, each kernel family of the plan asks for at most the
    163840 bytes of LDS a CU has, in float32 and in float64 -- by ``rn_potgnn_debug_plan_lds``, which calls the kernels' own
    footprint functions.  Over the dense structures at every width pair of ``PLAN_WIDTHS`` plus 24/20, 40/50 and 40/100, and
    over a star-plus-ring graph whose hub's degree runs over [cap - 4, cap] of each padded width (its low-degree atoms
    share tiles: a partition's maxima mix the hub's rows with another tile's atoms, which the planner answers with
    one-atom tiles).  One more edge than the cap is refused with RN_ERR_UNSUPPORTED at the PLANNED width: 24 / 20 runs 64
    wide, so 148 neighbours are refused there although 20 pads to 32."""
    from tests.helpers import DENSE_PROPERTIES, PLAN_WIDTHS
    lib = _lib.load()
    planned = {w: _planned_edge_width(lib, *w) for w in PLAN_WIDTHS + ((24, 20), (40, 50), (40, 100), (8, 20))}
    assert planned[(24, 20)] == 64 and planned[(8, 20)] == 32 and planned[(40, 100)] == 128 and planned[(5, 14)] == 16
    for name, props in DENSE_PROPERTIES.items():
        ea, eb, types, k = _dense_graph(name)
        for fn, fe in PLAN_WIDTHS + ((24, 20), (40, 50), (40, 100)):
            rc, lds, text = _plan_lds(lib, (len(types), len(ea), k, fn, fe), ea, eb, types)
            if props["max_degree"] > DEGREE_CAPS[planned[(fn, fe)]]:
                assert rc == _lib.RN_ERR_UNSUPPORTED and f"more than {DEGREE_CAPS[planned[(fn, fe)]]} per atom" in text, (name, fn, fe, text)
                continue
            assert rc == _lib.RN_OK, (name, fn, fe, text)
            assert lds["edge_agg"][1] > 0 and max(max(v) for v in lds.values()) <= CU_LDS_BYTES, (name, fn, fe, lds)
    for (fn, fe), fep in (((5, 14), 16), ((64, 16), 16), ((8, 20), 32), ((64, 64), 64), ((24, 20), 64), ((40, 100), 128), ((128, 128), 128)):
        cap = DEGREE_CAPS[fep]
        for degree in range(cap - 4, cap + 1):
            ea, eb, types = _star_ring(degree)
            rc, lds, text = _plan_lds(lib, (degree + 1, len(ea), 1, fn, fe), ea, eb, types)
            assert planned[(fn, fe)] == fep and rc == _lib.RN_OK, (fn, fe, degree, text)
            assert max(max(v) for v in lds.values()) <= CU_LDS_BYTES, (fn, fe, degree, lds)
        assert lds["edge_agg"][1] > CU_LDS_BYTES - (2 * fep * 8 + 36), (fn, fe, lds)  # (at the cap: one more row would not fit)
        ea, eb, types = _star_ring(cap + 1)
        rc, lds, text = _plan_lds(lib, (cap + 2, len(ea), 1, fn, fe), ea, eb, types)
        assert rc == _lib.RN_ERR_UNSUPPORTED, (fn, fe, lds)
        assert text == f"atom 0 has {cap + 1} outgoing edges; more than {cap} per atom is unsupported for size_edge_embedding={fe}"
    # a directed graph with more in-edges than out-edges at one atom: the destination tables count too
    ea = np.arange(1, 7001, dtype=np.int32)
    rc, _, text = _plan_lds(lib, (7001, 7000, 1, 64, 64), ea, np.zeros(7000, dtype=np.int32), np.zeros(7001, dtype=np.int32))
    assert rc == _lib.RN_ERR_UNSUPPORTED and "7000 incoming edges" in text and "163840 available" in text, text


def test_debug_plan_rejects_what_create_rejects():
    """The bad inputs of ``test_create_rejects_bad_arguments_without_touching_the_gpu`` (and the documented size limits)
    through ``rn_potgnn_debug_plan``: the same status codes and texts, from the same code."""
    lib = _lib.load()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    ea, eb, ty = np.array([0, 1], dtype=np.int32), np.array([1, 0], dtype=np.int32), np.zeros(4, dtype=np.int32)
    out, count = np.zeros(64, dtype=np.int32), ctypes.c_size_t(0)

    def plan(cfg, a, b, t=ty):
        rc = lib.rn_potgnn_debug_plan(ctypes.byref(cfg), p(a), p(b), p(t), 256, p(out), out.size, ctypes.byref(count))
        return rc, lib.rn_potgnn_last_error(None)

    cfg = _lib.Config(4, 2, 1, 200, 8, 1, -1.0, 0, 0)
    rc, text = plan(cfg, ea, eb)
    assert rc == _lib.RN_ERR_UNSUPPORTED and text == b"embedding sizes above 128 are not supported (Fn=200, Fe=8)"
    cfg.size_node_embedding = 8
    rc, text = plan(cfg, ea, np.array([1, 1], dtype=np.int32))
    assert rc == _lib.RN_ERR_INVALID_ARGUMENT and text == b"edge 1 = (1,1) is out of range or a self loop"
    rc, text = plan(cfg, np.array([1, 0], dtype=np.int32), ea)
    assert rc == _lib.RN_ERR_INVALID_ARGUMENT and text == b"edges must be strictly sorted by (a, b); violated at edge 1"
    rc, text = plan(cfg, ea, eb, np.array([0, 0, 1, 0], dtype=np.int32))
    assert rc == _lib.RN_ERR_INVALID_ARGUMENT and text == b"atom 2 has type 1 outside [0,1)"
    assert lib.rn_potgnn_debug_plan(ctypes.byref(cfg), None, p(eb), p(ty), 256, p(out), out.size, ctypes.byref(count)) \
        == _lib.RN_ERR_INVALID_ARGUMENT and lib.rn_potgnn_last_error(None) == b"null argument"
    cfg.num_edges = 0
    rc, text = plan(cfg, ea, eb)
    assert rc == _lib.RN_ERR_INVALID_ARGUMENT and text.startswith(b"reference graph has no edges")
    cfg.num_edges, cfg.num_atoms = 2, 0
    assert plan(cfg, ea, eb) == (_lib.RN_ERR_INVALID_ARGUMENT, b"invalid configuration (non-positive size)")
    # more out-edges than one LDS tile holds: 75 from one atom at Fe = 128 (71 fit)
    many = _lib.Config(80, 75, 1, 8, 128, 1, -1.0, 0, 0)
    star_a, star_b, star_ty = np.zeros(75, dtype=np.int32), np.arange(1, 76, dtype=np.int32), np.zeros(80, dtype=np.int32)
    rc, text = plan(many, star_a, star_b, star_ty)
    assert rc == _lib.RN_ERR_UNSUPPORTED
    assert text == b"atom 0 has 75 outgoing edges; more than 71 per atom is unsupported for size_edge_embedding=128"
    # the same texts come from rn_potgnn_create
    h, lat = ctypes.c_void_p(), np.eye(3)
    n = lib.rn_potgnn_weight_count(ctypes.byref(many))
    w = np.zeros(n, dtype=np.float32)
    rc = lib.rn_potgnn_create(ctypes.byref(many), p(star_a), p(star_b), p(star_ty), p(lat), p(w), n, p(lat), p(lat),
                              ctypes.byref(h))
    assert rc == _lib.RN_ERR_UNSUPPORTED and lib.rn_potgnn_last_error(None) == text
    # a valid graph: the size query, then the plan; no device is needed
    cfg = _lib.Config(4, 2, 1, 8, 8, 1, -1.0, 0, 0)
    assert lib.rn_potgnn_debug_plan(ctypes.byref(cfg), p(ea), p(eb), p(ty), 256, None, 0, ctypes.byref(count)) \
        == _lib.RN_ERR_INVALID_ARGUMENT and count.value > 0
    assert plan(cfg, ea, eb)[0] == _lib.RN_OK and out[0] == 16 and out[1] == 16
    assert lib.rn_potgnn_debug_plan(ctypes.byref(cfg), p(ea), p(eb), p(ty), 0, p(out), out.size, ctypes.byref(count)) \
        == _lib.RN_ERR_INVALID_ARGUMENT


def test_committed_profile_records_are_fresh():
    """`bench.py` prints `roofline.traffic` / `issue_frac` from PMC / SQ passes committed under profiles/rNN/ -- next to a
    FRESH timing.  Every record carries the git blob hash of the kernel source it was taken on and is refused when that file
    has changed since; this test fails as soon as a kernel edit leaves the newest records behind, so
    that the profile is re-taken (tools/profile.sh + tools/make_profile_json.py) before the change is committed."""
    import json
    import bench
    shapes = {"perf": (256, 4608, 64, 64), "parity": (256, 4608, 5, 14)}
    for name, shape in (("edge_ps_traffic.json", "perf"), ("edge_ps_issue.json", "perf"), ("node_atom_traffic.json", "perf"),
                        ("edge_narrow_traffic.json", "parity"), ("edge_narrow_issue.json", "parity"),
                        ("node_narrow_traffic.json", "parity")):
        rec = bench.committed_profile(name, *shapes[shape])
        assert rec is not None, f"{name}: no record of this shape whose kernel source is the one in this tree"
        assert rec["_path"].startswith("profiles/r06"), rec["_path"]
    # a record without a stamp, or with a foreign one, is refused
    stale = os.path.join(bench.ROOT, "profiles", "r05", "edge_ps_traffic.json")
    assert "kernel_source" not in json.load(open(stale))
    older = bench.PROFILE_ROUNDS
    try:
        bench.PROFILE_ROUNDS = ("r05",)
        assert bench.committed_profile("edge_ps_traffic.json", 256, 4608, 64, 64) is None
    finally:
        bench.PROFILE_ROUNDS = older


# ----------------------------------------------------------------------------- packed weight layout
_PACKED_GOLDEN = os.path.join(ROOT, "tests", "golden", "packed_weights.npz")
_PACKED_CACHE = {}


def _weight_cfg(shape):
    k, fn, fe, passes = shape
    return _lib.Config(4, 2, k, fn, fe, passes, -1.0, 0, 0)


def _pack(shape, blob):
    """``rn_potgnn_debug_pack_weights``: (packed, mask, writers, flags), size query first."""
    lib, cfg, count = _lib.load(), _weight_cfg(shape), ctypes.c_size_t(0)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    rc = lib.rn_potgnn_debug_pack_weights(ctypes.byref(cfg), p(blob), blob.size, None, None, None, None, 0, ctypes.byref(count))
    assert rc == _lib.RN_ERR_INVALID_ARGUMENT and count.value > 0, lib.rn_potgnn_last_error(None)
    n = count.value
    packed, mask, writers = np.full(n, 7, dtype=np.float32), np.full(n, 7, dtype=np.uint8), np.full(n, 7, dtype=np.uint8)
    flags = np.full(1 + shape[3], 7, dtype=np.int32)
    rc = lib.rn_potgnn_debug_pack_weights(ctypes.byref(cfg), p(blob), blob.size, p(packed), p(mask), p(writers), p(flags), n,
                                          ctypes.byref(count))
    assert rc == _lib.RN_OK and count.value == n, lib.rn_potgnn_last_error(None)
    return packed, mask, writers, flags


def _unpack(shape, packed, buffers):
    lib, cfg, count = _lib.load(), _weight_cfg(shape), ctypes.c_size_t(0)
    out = np.full(lib.rn_potgnn_weight_count(ctypes.byref(cfg)), 7, dtype=np.float32)
    rc = lib.rn_potgnn_debug_unpack_weights(ctypes.byref(cfg), ctypes.c_void_p(packed.ctypes.data), packed.size, int(buffers),
                                            ctypes.c_void_p(out.ctypes.data), out.size, ctypes.byref(count))
    assert rc == _lib.RN_OK and count.value == out.size, lib.rn_potgnn_last_error(None)
    return out


def _packed_cases():
    """name -> (shape, blob, packed, mask, writers, flags), packed once for the tests below."""
    from tests.helpers import weight_layout_cases
    if not _PACKED_CACHE:
        for name, shape, blob in weight_layout_cases():
            _PACKED_CACHE[name] = (shape, blob) + _pack(shape, blob)
    return _PACKED_CACHE


def _digest(packed):
    import hashlib
    canon = packed.copy()
    canon[np.isnan(canon)] = np.nan  # one NaN pattern: a centred copy of an infinite weight is inf - inf
    return np.frombuffer(hashlib.sha256(canon.tobytes()).digest(), dtype=np.uint8)


def test_packed_weights_match_the_parent_commit():
    """The host-only packer (csrc/weight_layout.hip) writes, bit for bit, the packed blob, the trainable mask and the flags
    (split-f16 range guard; folded gate per pass) that ``pack_weights``, ``trainable_mask``, ``mfma_f16_range_ok`` and the
    loop of ``refresh_pass_flags`` in what was then csrc/api.hip (now csrc/forward.hip) produced before they moved out of it.  tests/golden/packed_weights.npz was
    recorded from that parent commit (b687cbc), not from this code: a throw-away harness (not committed) compiled the
    parent's function text, unchanged, around a minimal handle and ran it on a CPU over tests/helpers.py
    ``weight_layout_cases`` (profiles/weight_layout_ab.txt: the commit, the harness, the cases, the file size).  A packed
    blob of the product shape is 3 MB of incompressible floats, so the file keeps the blob itself for the three narrow
    shapes and a SHA-256 of its bytes for every case; masks and flags are kept in full."""
    golden = np.load(_PACKED_GOLDEN)
    cases = _packed_cases()
    assert sorted({k.split("/")[0] for k in golden.files}) == sorted(cases)
    kept = 0
    for name, (shape, blob, packed, mask, writers, flags) in cases.items():
        np.testing.assert_array_equal(mask, golden[name + "/mask"], err_msg=name)
        np.testing.assert_array_equal(flags, golden[name + "/flags"], err_msg=name)
        if name + "/packed" in golden.files:
            np.testing.assert_array_equal(packed, golden[name + "/packed"], err_msg=name)
            kept += 1
        np.testing.assert_array_equal(_digest(packed), golden[name + "/sha256"], err_msg=name)
    assert kept == 3
    # the three flag cases each flip one decision of the tame blob they start from
    flags = {name: list(c[5]) for name, c in cases.items()}
    assert flags["flags_base"] == [1, 1, 1] and flags["flags_c2_inf"] == [0, 1, 1]
    assert flags["flags_readout_bound"] == [0, 1, 1] and flags["flags_small_gamma"] == [1, 1, 0]


def test_unpack_inverts_pack():
    """``unpack(pack(w)) == w`` exactly with the buffers switch on (``rn_potgnn_get_weights``); with it off (a gradient
    download) the state dict's buffers come back as zeros and every parameter is still exact."""
    from tests.helpers import STATE_DICT_BUFFERS, state_dict_slices
    for name, (shape, blob, packed, mask, writers, flags) in _packed_cases().items():
        np.testing.assert_array_equal(_unpack(shape, packed, True), blob, err_msg=name)
        want = blob.copy()
        for key, s in state_dict_slices(*shape).items():
            if key in STATE_DICT_BUFFERS:
                want[s] = 0.0
        assert np.count_nonzero(want != blob) > 0
        np.testing.assert_array_equal(_unpack(shape, packed, False), want, err_msg=name)


def test_packed_layout_is_consistent_with_itself():
    """Per shape: the mask has one 1 per parameter element of the state dict; no packed entry is reached by two state-dict
    elements, by two derived ranges, or by both (readout bias 0 is scattered into its padded copy and the plain one is
    derived from it, so not even that pair overlaps); every state-dict element is stored exactly once; and RN_OK itself
    says that the three ranges ``rn_potgnn_adam_step`` fetches in one piece are contiguous (``PackedLayout::c3_norm_1``,
    ``mfma_scales``, ``readout`` throw otherwise)."""
    from tests.helpers import STATE_DICT_BUFFERS, state_dict_sizes
    lib = _lib.load()
    for name, (shape, blob, packed, mask, writers, flags) in _packed_cases().items():
        count = lib.rn_potgnn_weight_count(ctypes.byref(_weight_cfg(shape)))
        buffers = sum(n for key, n in state_dict_sizes(*shape) if key in STATE_DICT_BUFFERS)
        assert count == blob.size and buffers == 3 * shape[2]
        assert set(np.unique(mask)) <= {0, 1} and int(mask.sum()) == count - buffers, name
        scattered, derived = writers & 15, writers >> 4
        assert scattered.max() == 1 and int(scattered.sum()) == count, name
        assert derived.max() == 1 and not np.any((scattered > 0) & (derived > 0)), name
        assert np.all(scattered[mask == 1] == 1)
        # an entry nobody writes is padding (zero), the row of ones, or device-computed (zero on the host)
        idle = packed[(scattered == 0) & (derived == 0)]
        assert np.all((idle == 0.0) | (idle == 1.0)), name


def test_weight_count_matches_the_reference_state_dict(golden):
    """``rn_potgnn_weight_count`` -- the sum over the library's table of state-dict tensors -- equals the element count of
    the state dict the reference model itself wrote into the fixture: every floating-point tensor of it (its one integer
    entry, BatchNorm's step counter ``num_batches_tracked``, is no weight; the Python layer keeps it)."""
    name, g = golden
    hp = g["hp"]
    k = int((G.atom_type_map(g["atomic_numbers"]) >= 0).sum())
    cfg = _lib.Config(len(g["atomic_numbers"]), 2, k, int(hp[1]), int(hp[2]), int(hp[3]), -1.0, 0, 0)
    sd = {key: g[key] for key in g.files if key.startswith("sd/")}
    assert [key for key, v in sd.items() if v.dtype.kind != "f"] == ["sd/_to_polarizability_embedding.1.num_batches_tracked"]
    assert _lib.load().rn_potgnn_weight_count(ctypes.byref(cfg)) == sum(v.size for v in sd.values() if v.dtype.kind == "f")


def test_debug_weight_entries_reject_what_create_rejects():
    """Null pointers, a wrong weight count and an unsupported width through ``rn_potgnn_debug_pack_weights`` /
    ``rn_potgnn_debug_unpack_weights``: the status codes and texts of ``rn_potgnn_create``, from the same code."""
    lib = _lib.load()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    cfg, count = _weight_cfg((2, 8, 8, 1)), ctypes.c_size_t(0)
    n = lib.rn_potgnn_weight_count(ctypes.byref(cfg))
    w = np.zeros(n, dtype=np.float32)
    packed, _, _, _ = _pack((2, 8, 8, 1), w)
    mask, flags, out = np.zeros(packed.size, dtype=np.uint8), np.zeros(2, dtype=np.int32), np.zeros(n, dtype=np.float32)

    def pack(cfg_ref, weights, num):
        rc = lib.rn_potgnn_debug_pack_weights(cfg_ref, weights, num, p(packed), p(mask), None, p(flags), packed.size,
                                              ctypes.byref(count))
        return rc, lib.rn_potgnn_last_error(None)

    def unpack(cfg_ref, blob, num, capacity=out.size):
        rc = lib.rn_potgnn_debug_unpack_weights(cfg_ref, blob, num, 1, p(out), capacity, ctypes.byref(count))
        return rc, lib.rn_potgnn_last_error(None)

    assert pack(None, p(w), n) == (_lib.RN_ERR_INVALID_ARGUMENT, b"null argument")
    assert pack(ctypes.byref(cfg), None, n) == (_lib.RN_ERR_INVALID_ARGUMENT, b"null argument")
    assert unpack(None, p(packed), packed.size) == (_lib.RN_ERR_INVALID_ARGUMENT, b"null argument")
    assert unpack(ctypes.byref(cfg), None, packed.size) == (_lib.RN_ERR_INVALID_ARGUMENT, b"null argument")
    assert lib.rn_potgnn_debug_pack_weights(ctypes.byref(cfg), p(w), n, p(packed), p(mask), None, p(flags), packed.size, None) \
        == _lib.RN_ERR_INVALID_ARGUMENT
    text = b"weights has %d floats, expected %d" % (n - 1, n)
    assert pack(ctypes.byref(cfg), p(w), n - 1) == (_lib.RN_ERR_INVALID_ARGUMENT, text)
    # the same text comes from rn_potgnn_create
    ea, eb, ty, lat, h = np.array([0, 1], dtype=np.int32), np.array([1, 0], dtype=np.int32), np.zeros(4, dtype=np.int32), \
        np.eye(3), ctypes.c_void_p()
    rc = lib.rn_potgnn_create(ctypes.byref(cfg), p(ea), p(eb), p(ty), p(lat), p(w), n - 1, p(lat), p(lat), ctypes.byref(h))
    assert rc == _lib.RN_ERR_INVALID_ARGUMENT and lib.rn_potgnn_last_error(None) == text
    wide = _weight_cfg((2, 200, 8, 1))
    text = b"embedding sizes above 128 are not supported (Fn=200, Fe=8)"
    assert pack(ctypes.byref(wide), p(w), n) == (_lib.RN_ERR_UNSUPPORTED, text)
    assert unpack(ctypes.byref(wide), p(packed), packed.size) == (_lib.RN_ERR_UNSUPPORTED, text)
    none = _weight_cfg((2, 8, 8, 0))
    assert pack(ctypes.byref(none), p(w), n) == (_lib.RN_ERR_INVALID_ARGUMENT, b"invalid configuration (non-positive size)")
    # a packed blob of the wrong length, and the size query of the inverse
    rc, text = unpack(ctypes.byref(cfg), p(packed), packed.size - 4)
    assert rc == _lib.RN_ERR_INVALID_ARGUMENT and text == b"packed has %d floats, expected %d" % (packed.size - 4, packed.size)
    rc, _ = unpack(ctypes.byref(cfg), p(packed), packed.size, capacity=n - 1)
    assert rc == _lib.RN_ERR_INVALID_ARGUMENT and count.value == n
    assert unpack(ctypes.byref(cfg), p(packed), packed.size)[0] == _lib.RN_OK
