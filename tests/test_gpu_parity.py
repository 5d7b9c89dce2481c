"""Parity of the HIP path (through the C ABI) against the golden fixtures produced by the
reference and against the CPU oracle.  Needs a real MI355X: run with ``-m gpu``.

Tolerances (float32 path): per-stage intermediates atol 2e-5 on O(1) values; final
polarizabilities within 1e-5 relative (the north-star bar); indices bit-exact.
"""
import os

import numpy as np
import pytest
import torch

from tests.conftest import load_golden
from tests.helpers import product_model_from_golden

pytestmark = pytest.mark.gpu

REL = 1e-5


def _rel_err(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.fixture
def staged(monkeypatch):
    monkeypatch.setenv("RN_POTGNN_KEEP_STAGES", "1")


def test_device_loaded():
    assert torch.cuda.is_available()
    from ramannoodle_amd import _lib
    assert b"gfx950" in _lib.load().rn_potgnn_version()


def test_triplet_indices_bit_exact(golden):
    name, g = golden
    model = product_model_from_golden(g)
    trip = model.triplets()
    for mine, key in zip(trip, ["i", "j", "idx_i", "idx_j", "idx_k", "slot5", "slot6"]):
        np.testing.assert_array_equal(mine, g["trip/" + key], err_msg=key)
    # device order: grouped by destination edge, ascending source edge == scatter order
    raw = model.device_triplets_raw()
    key = raw[3].astype(np.int64) * (model.num_edges + 1) + raw[4]
    assert np.all(np.diff(key) > 0)


def test_stages_match_reference(golden, staged):
    name, g = golden
    model = product_model_from_golden(g)
    pos = g["pos_batch"][:5]
    s = pos.shape[0]
    lat = torch.tensor(g["lattice"]).expand(s, 3, 3)
    zs = torch.tensor(g["atomic_numbers"]).expand(s, -1)
    model.eval()  # a fresh model is in training mode, like a torch Module
    out = model.forward(lat, zs, torch.tensor(pos)).numpy()
    n, e = model.num_atoms, model.num_edges
    if "f32/unit" in g.files:
        geo = model.debug_stage(0)
        np.testing.assert_allclose(geo[:, :3], g["f32/unit"][: s * e], rtol=0, atol=2e-6)
        np.testing.assert_allclose(geo[:, 3:], g["f32/dist"][: s * e], rtol=2e-6, atol=0)
    for p in range(int(g["hp"][3]) + 1):
        if f"f32/node{p}" in g.files:
            np.testing.assert_allclose(model.debug_stage(1, p), g[f"f32/node{p}"][: s * n], rtol=0,
                                       atol=2e-5, err_msg=f"node{p}")
        if f"f32/edge{p}" in g.files:
            np.testing.assert_allclose(model.debug_stage(2, p), g[f"f32/edge{p}"][: s * e], rtol=0,
                                       atol=2e-5, err_msg=f"edge{p}")
    if "f32/pol_emb" in g.files:
        ref = g["f32/pol_emb"][: s * e]
        np.testing.assert_allclose(model.debug_stage(3), ref, rtol=0, atol=2e-5 * max(1.0, np.abs(ref).max()))
    np.testing.assert_allclose(out, g["f32/forward"][:s], rtol=0,
                               atol=REL * np.abs(g["f32/forward"]).max())


def test_calc_polarizabilities_matches_reference_and_oracle(golden):
    from oracle import potgnn_oracle as O
    name, g = golden
    model = product_model_from_golden(g)
    pos = g["pos_batch"]
    alpha = model.calc_polarizabilities(pos)
    assert alpha.dtype == np.float64 and alpha.shape == (pos.shape[0], 3, 3)
    np.testing.assert_array_equal(alpha, np.swapaxes(alpha, 1, 2))
    np.testing.assert_array_equal(model.calc_polarizabilities(pos, progress=True), alpha)  # the reference's tqdm bar, opt-in
    # standardised part within 1e-5 relative; de-standardised alpha likewise
    std_part = (alpha - g["mean"]) / g["std"]
    ref_part = (g["f32/alpha"] - g["mean"]) / g["std"]
    assert _rel_err(std_part, ref_part) < REL
    assert _rel_err(alpha, g["f32/alpha"]) < REL
    orc = O.calc_polarizabilities(O.model_from_arrays(g), pos[:8], faithful=False)
    assert _rel_err(alpha[:8], orc) < REL
    if "f64/alpha" in g.files:
        assert _rel_err(alpha, g["f64/alpha"]) < REL


def test_batch_size_independence_and_edge_cases():
    """Results do not depend on chunking (reference: test_gnn.py:76-113,163-193);
    S = 0 and S = 1 work."""
    g = load_golden("rocksalt64_s205")
    whole = product_model_from_golden(g)
    chunked = product_model_from_golden(g, max_chunk_structures=7)
    pos = g["pos_batch"]
    a = whole.calc_polarizabilities(pos)
    b = chunked.calc_polarizabilities(pos)
    np.testing.assert_array_equal(a, b)
    assert _rel_err(a, g["f32/alpha"]) < REL
    assert whole.calc_polarizabilities(pos[:0]).shape == (0, 3, 3)
    np.testing.assert_array_equal(whole.calc_polarizabilities(pos[17:18])[0], a[17])
    # permuting frames permutes results
    perm = np.random.default_rng(0).permutation(pos.shape[0])
    np.testing.assert_array_equal(whole.calc_polarizabilities(pos[perm]), a[perm])
    # determinism (segmented reductions, no atomics)
    np.testing.assert_array_equal(whole.calc_polarizabilities(pos), a)


def test_forward_with_per_sample_lattices():
    """``forward(lattice[S,3,3], atomic_numbers, positions)`` with a different lattice per sample
    (_gnn.py:603-611) against the reference's output on six strained cells; other species are
    refused with the documented NotImplementedError."""
    g, r = load_golden("triclinic20"), load_golden("triclinic20_r2")
    model = product_model_from_golden(g).eval()
    s = r["lat/positions"].shape[0]
    zs = torch.tensor(g["atomic_numbers"]).expand(s, -1)
    out = model.forward(torch.tensor(r["lat/lattices"]), zs, torch.tensor(r["lat/positions"])).numpy()
    scale = np.abs(r["lat/forward"]).max()
    assert np.abs(out - r["lat/forward"]).max() < REL * scale
    assert np.abs(out - r["lat/forward64"]).max() < REL * scale
    same = model.forward(torch.tensor(g["lattice"]).expand(s, 3, 3), zs, torch.tensor(r["lat/positions"])).numpy()
    np.testing.assert_array_equal(same[0], out[0])          # sample 0 carries the reference lattice
    assert np.abs(same[1:] - out[1:]).max() > 1e3 * REL * scale  # the others really differ


def test_forward_with_per_sample_atomic_numbers():
    """``forward(lattice, atomic_numbers[S,N], positions)`` with species that differ between samples
    (``_convert_to_atom_type`` + node embedding per (sample, atom), ``_gnn.py:541-557,642-643``)
    against the reference's float32 and float64 outputs: pairs of atoms swapped, one species
    replaced, half of the samples on a strained lattice as well."""
    g, r = load_golden("triclinic20"), load_golden("triclinic20_r3")
    model = product_model_from_golden(g).eval()
    zs, lat, pos = r["zs/atomic_numbers"], r["zs/lattices"], r["zs/positions"]
    out = model.forward(torch.tensor(lat), torch.tensor(zs), torch.tensor(pos)).numpy()
    scale = np.abs(r["zs/forward64"]).max()
    assert np.abs(out - r["zs/forward"]).max() < REL * scale
    assert np.abs(out - r["zs/forward64"]).max() < REL * scale
    ref_zs = np.broadcast_to(g["atomic_numbers"], zs.shape)
    plain = model.forward(torch.tensor(lat), torch.tensor(ref_zs.copy()), torch.tensor(pos)).numpy()
    np.testing.assert_array_equal(plain[0], out[0])               # sample 0 carries the reference species
    assert np.abs(plain[1:] - out[1:]).max() > 1e3 * REL * scale  # the others really differ
    for i in range(len(zs)):  # sample by sample = the batch (test_gnn.py:76-113)
        one = model.forward(torch.tensor(lat[i:i + 1]), torch.tensor(zs[i:i + 1]), torch.tensor(pos[i:i + 1])).numpy()
        np.testing.assert_array_equal(one[0], out[i])
    unknown = zs.copy()
    unknown[2, 5] = 79  # the model has no atom type for gold: the reference's Embedding raises IndexError
    with pytest.raises(IndexError):
        model.forward(torch.tensor(lat), torch.tensor(unknown), torch.tensor(pos))


def test_forward_computes_in_the_dtype_of_the_models_parameters():
    """The reference's ``forward`` computes in the dtype its parameters were built with (``_gnn.py:493-494, 617-665``): a
    model constructed under ``torch.set_default_dtype(torch.float64)`` -- or turned with ``.double()`` -- evaluates in double.
    Against the reference's own float64 ``forward`` outputs (fixtures made by the reference under that default): the plain
    batch, a lattice per sample, species per sample; host tensors and CUDA tensors.  Tolerance 1e-7 of the largest output:
    the device keeps float32 master weights and float32 Gaussian offsets (exactly widened), the reference under that default
    builds its offsets in float64 -- measured 4e-8 here, against 1e-6 for the float32 kernels."""
    F64 = 1e-7
    g, r2, r3 = load_golden("triclinic20"), load_golden("triclinic20_r2"), load_golden("triclinic20_r3")
    model32 = product_model_from_golden(g).eval()
    torch.set_default_dtype(torch.float64)
    try:
        model = product_model_from_golden(g).eval()  # parameters float64, as the reference's under this default
    finally:
        torch.set_default_dtype(torch.float32)
    assert next(model.parameters()).dtype == torch.float64 and next(model32.parameters()).dtype == torch.float32
    s = r2["lat/positions"].shape[0]
    zs_ref = torch.tensor(g["atomic_numbers"]).expand(s, -1)
    out = model.forward(torch.tensor(r2["lat/lattices"]), zs_ref, torch.tensor(r2["lat/positions"]))
    assert out.dtype == torch.float64 and not out.is_cuda
    scale = np.abs(r2["lat/forward64"]).max()
    assert np.abs(out.numpy() - r2["lat/forward64"]).max() < F64 * scale
    out32 = model32.forward(torch.tensor(r2["lat/lattices"]), zs_ref, torch.tensor(r2["lat/positions"]))
    assert out32.dtype == torch.float32 and np.abs(out32.numpy() - r2["lat/forward64"]).max() < REL * scale
    assert np.abs(out32.numpy().astype(np.float64) - out.numpy()).max() > 0  # (two arithmetics: the test can tell them apart)
    zs, lat, pos = r3["zs/atomic_numbers"], r3["zs/lattices"], r3["zs/positions"]
    out = model.forward(torch.tensor(lat), torch.tensor(zs), torch.tensor(pos)).numpy()
    assert np.abs(out - r3["zs/forward64"]).max() < F64 * np.abs(r3["zs/forward64"]).max()
    if "f64/forward" in g.files:  # the fixture's own batch on the reference lattice and species
        n = min(4, g["pos_batch"].shape[0])
        plain = model.forward(torch.tensor(g["lattice"]).expand(n, 3, 3), torch.tensor(g["atomic_numbers"]).expand(n, -1),
                              torch.tensor(g["pos_batch"][:n])).numpy()
        assert np.abs(plain - g["f64/forward"][:n]).max() < F64 * np.abs(g["f64/forward"]).max()
    # CUDA tensors in, a float64 CUDA tensor out
    dev = model.forward(torch.tensor(lat, device="cuda"), torch.tensor(zs, device="cuda"), torch.tensor(pos, device="cuda"))
    assert dev.is_cuda and dev.dtype == torch.float64
    np.testing.assert_array_equal(dev.cpu().numpy(), out)
    # .double() on a float32 model does the same, .float() brings the float32 kernels back
    turned = product_model_from_golden(g).eval().double()
    np.testing.assert_array_equal(turned.forward(torch.tensor(lat), torch.tensor(zs), torch.tensor(pos)).numpy(), out)
    assert turned.float().forward(torch.tensor(lat), torch.tensor(zs), torch.tensor(pos)).dtype == torch.float32


def test_calc_polarizabilities_in_float64(golden):
    """``calc_polarizabilities`` evaluates in ``torch.get_default_dtype()`` (``_gnn.py:705-710``):
    under a float64 default (or ``dtype=torch.float64``) the kernels instantiated for ``double`` run
    and reproduce the reference's float64 results far below float32 round-off."""
    name, g = golden
    if "f64/alpha" not in g.files:
        pytest.skip("fixture has no float64 run")
    model = product_model_from_golden(g)
    pos = g["pos_batch"]
    a64 = model.calc_polarizabilities(pos, dtype=torch.float64)
    # (5e-8, not 1e-12: the fixture's float64 reference model was BUILT under a float64 default, so its
    #  Gaussian coefficient -0.5 / (mu_1 - mu_0)^2 comes from a float64 linspace, while its offsets --
    #  like every weight -- are the float32 state widened; here the coefficient is derived from those
    #  float32 offsets.  Measured 5.9e-9 on tio2_notebook, whose 5/13 spacing is inexact in float32.)
    assert _rel_err(a64, g["f64/alpha"]) < 5e-8, name
    a32 = model.calc_polarizabilities(pos)
    assert _rel_err(a32, g["f64/alpha"]) < REL and np.abs(a32 - a64).max() > 0
    torch.set_default_dtype(torch.float64)
    try:
        np.testing.assert_array_equal(model.calc_polarizabilities(pos), a64)
    finally:
        torch.set_default_dtype(torch.float32)
    np.testing.assert_array_equal(model.calc_polarizabilities(pos), a32)  # and back
    with pytest.raises(ValueError, match="unsupported evaluation dtype"):
        model.calc_polarizabilities(pos, dtype=torch.float16)


@pytest.mark.parametrize("fn, fe", [(40, 100), (24, 20), (12, 40), (64, 64), (5, 14)])
def test_float64_evaluation_at_other_widths(fn, fe):
    """The float64 entry (``rowgemm_f64_mfma_kernel`` projections at K = 16 .. 128, the ``double`` aggregation
    kernels) against the oracle evaluated in float64, with per-sample species on the way (``forward``)."""
    from oracle import potgnn_oracle as O
    g = load_golden("triclinic20")
    model, oracle = _random_model(g, 3.0, fn, fe, 2, seed=fn * 13 + fe)
    pos = g["pos_batch"][:3]
    got = model.calc_polarizabilities(pos, dtype=torch.float64)
    want = O.calc_polarizabilities(oracle.to(torch.float64), pos, faithful=False)
    assert _rel_err(got, np.asarray(want)) < 1e-10, (fn, fe)
    got32 = model.calc_polarizabilities(pos)
    assert _rel_err((got32 - oracle.mean) / oracle.std, (np.asarray(want) - oracle.mean) / oracle.std) < REL


def test_forward_on_positions_far_outside_the_unit_cell():
    """Positions drawn from N(0,1), as in the reference's own batch test
    (``test/tests/torch/test_gnn.py:83-113``): fractional coordinates up to +-3.  Against the
    reference's float32 and float64 outputs, whole batch and one structure at a time."""
    g, r = load_golden("triclinic20"), load_golden("triclinic20_randn")
    model = product_model_from_golden(g).eval()
    s = r["positions"].shape[0]
    lat = torch.tensor(g["lattice"], dtype=torch.float32).expand(s, 3, 3)
    zs = torch.tensor(g["atomic_numbers"]).expand(s, -1)
    pos = torch.tensor(r["positions"])
    out = model.forward(lat, zs, pos).numpy()
    scale = np.abs(r["forward64"]).max()
    assert np.abs(out - r["forward"]).max() < REL * scale
    assert np.abs(out - r["forward64"]).max() < REL * scale
    for i in range(s):
        one = model.forward(lat[i:i + 1], zs[i:i + 1], pos[i:i + 1]).numpy()
        np.testing.assert_array_equal(one[0], out[i])
    alpha = model.calc_polarizabilities(r["positions"].astype(np.float64))
    assert _rel_err(alpha, r["calc"]) < REL


@pytest.mark.parametrize("batch_size", [50, 100, 180])
def test_forward_and_calc_polarizabilities_agree(batch_size):
    """The property the reference's own ``test_calc_polarizabilities`` asserts
    (``test/tests/torch/test_gnn.py:170-193``): with mean 0 and stddev 1, ``forward`` (standardised
    6-vectors -> tensors) and ``calc_polarizabilities`` give the same numbers on N(0,1) positions,
    for batch sizes below, at and above the reference's 100-structure sub-batch."""
    from ramannoodle_amd.pmodel import polarizability_vectors_to_tensors
    g = load_golden("triclinic20")
    model = product_model_from_golden(g, mean=np.zeros((3, 3)), stddev=np.ones((3, 3))).eval()
    torch.manual_seed(batch_size)
    pos = torch.randn(batch_size, model.num_atoms, 3)
    lat = torch.tensor(g["lattice"], dtype=torch.float32).expand(batch_size, 3, 3)
    zs = torch.tensor(g["atomic_numbers"]).expand(batch_size, -1)
    forward = polarizability_vectors_to_tensors(model.forward(lat, zs, pos).detach().clone()).numpy()
    calc = model.calc_polarizabilities(pos.detach().clone().numpy())
    assert np.allclose(forward, calc, atol=1e-6)


def test_device_resident_entry_point():
    g = load_golden("rocksalt64_parity")
    model = product_model_from_golden(g)
    pos = torch.tensor(g["pos_batch"], device="cuda")
    out = model.calc_polarizabilities_device(pos, synchronize=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), model.calc_polarizabilities(g["pos_batch"]))


def test_narrow_kernels_do_not_depend_on_their_tiling(monkeypatch):
    """The narrow EdgeBlock / NodeBlock (documented widths) give the same bits whatever the atom tiles: the default two-wave
    tiles, four-wave tiles, tiles of 400 rows (several destinations per lane: the uniform-trip-count loop), one-atom tiles,
    and the opt-in forms that only move data differently (rows to HBM through LDS; the scalar-FMA readout is a different
    summation order and agrees to round-off, as does the folded-scale loop)."""
    g = load_golden("rocksalt64_parity")
    pos = np.concatenate([g["pos_batch"]] * 3)
    base = product_model_from_golden(g).calc_polarizabilities(pos)
    scale = np.abs(base).max()
    for knobs, exact in (({"RN_POTGNN_NARROW_TILE_ROWS": "256"}, True), ({"RN_POTGNN_NARROW_TILE_ROWS": "400"}, True),
                         ({"RN_POTGNN_NARROW_TILE_ROWS": "18"}, True), ({"RN_POTGNN_NODE_TILE_ROWS": "64"}, True),
                         ({"RN_POTGNN_NODE_RING": "2"}, True), ({"RN_POTGNN_NARROW_STAGE": "1"}, True),
                         ({"RN_POTGNN_READOUT_MFMA": "0"}, False), ({"RN_POTGNN_NARROW_FOLD": "1"}, False)):
        for key, value in knobs.items():
            monkeypatch.setenv(key, value)
        got = product_model_from_golden(g).calc_polarizabilities(pos)
        for key in knobs:
            monkeypatch.delenv(key)
        if exact:
            np.testing.assert_array_equal(got, base, err_msg=str(knobs))
        else:
            assert np.abs(got - base).max() < 2e-6 * scale, knobs


@pytest.mark.parametrize("fixture", ["rocksalt64_parity", "rocksalt64_perf"])
def test_host_entry_stages_float32_positions_bit_identically(fixture, monkeypatch):
    """The host entry casts the caller's float64 positions to float32 while it stages them into page-locked memory and
    sends them through in pieces (``rn_potgnn_calc_polarizabilities`` / ``..._to_device``).  The reference casts before
    any arithmetic (``_gnn.py:709``), so every batch size and every piece size must give the bits of a float64 upload to
    the device-resident entry -- for the narrow kernels (documented widths) and for the wide ones."""
    g = load_golden(fixture)
    rng = np.random.default_rng(12)
    base = np.asarray(g["pos_batch"], dtype=np.float64)
    pos = (base[rng.integers(0, base.shape[0], 301)] + 1e-3 * rng.standard_normal((301,) + base.shape[1:])) % 1.0
    reference = product_model_from_golden(g).calc_polarizabilities_device(torch.tensor(pos, device="cuda"),
                                                                          synchronize=True).cpu().numpy()
    for piece in (None, "1", "7", "64", "1000"):
        if piece is None:
            monkeypatch.delenv("RN_POTGNN_HOST_PIECE", raising=False)
        else:
            monkeypatch.setenv("RN_POTGNN_HOST_PIECE", piece)
        model = product_model_from_golden(g)
        for count in (1, 5, 301):
            np.testing.assert_array_equal(model.calc_polarizabilities(pos[:count]), reference[:count])
        on_device = model.calc_polarizabilities_to_device(pos)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(on_device.cpu().numpy(), reference)
        assert on_device.is_cuda and on_device.dtype == torch.float64
    # back-to-back calls that return before their work is done: every call's staging and device buffers are its own until
    # its copies and kernels are through with them
    monkeypatch.delenv("RN_POTGNN_HOST_PIECE", raising=False)
    model = product_model_from_golden(g)
    batches = [pos[::-1].copy(), pos.copy(), (pos[:150] + 0.25) % 1.0, pos[100:].copy()]
    want = [model.calc_polarizabilities(b) for b in batches]
    outs = [model.calc_polarizabilities_to_device(b) for b in batches]  # no synchronisation in between
    mixed = model.calc_polarizabilities(pos)                              # ... and the synchronous entry right behind them
    torch.cuda.synchronize()
    for got, ref in zip(outs, want):
        np.testing.assert_array_equal(got.cpu().numpy(), ref)
    np.testing.assert_array_equal(mixed, reference)
    # a non-contiguous / float32 caller array goes through the same checks and conversion as before
    np.testing.assert_array_equal(product_model_from_golden(g).calc_polarizabilities(pos[::2].astype(np.float32)),
                                  product_model_from_golden(g).calc_polarizabilities_device(
                                      torch.tensor(pos[::2].astype(np.float32).astype(np.float64), device="cuda"),
                                      synchronize=True).cpu().numpy())


def test_phonon_raman_tensors_float64_and_spectrum():
    from ramannoodle_amd.dynamics import Phonons
    g = load_golden("triclinic20")
    model = product_model_from_golden(g)
    ph = Phonons(g["positions"], g["ph/wavenumbers"], g["ph/displacements"])
    spec = ph.get_raman_spectrum(model)
    ref = g["ph/raman_tensors"]
    assert _rel_err(spec.raman_tensors, ref) < REL
    w, i = spec.measure()
    np.testing.assert_allclose(i, g["ph/int_raw"], rtol=5e-5, atol=REL * g["ph/int_raw"].max())
    w, i = spec.measure(laser_correction=True, laser_wavelength=532,
                        bose_einstein_correction=True, temperature=300)
    np.testing.assert_allclose(i, g["ph/int_corr"], rtol=5e-5, atol=REL * g["ph/int_corr"].max())


def test_md_trajectory_spectrum():
    """MD Raman spectrum end to end (wrap -> device alpha(t) in float32 -> MDRamanSpectrum.measure)
    against the reference.  The intensities are built from differences of alpha(t), so float32
    round-off of alpha is amplified: the reference's own float32 and float64 spectra differ by
    3e-6 of the spectrum's scale on this trajectory (``md64/ref_f32_vs_f64``).  The device's
    float32 spectrum must be as close to the float64 reference as that, and within the north
    star's 1e-5 of both reference spectra."""
    from ramannoodle_amd.dynamics import Trajectory
    g, r = load_golden("triclinic20"), load_golden("triclinic20_r2")
    model = product_model_from_golden(g)
    spec = Trajectory(g["md/positions"], float(g["md/timestep"])).get_raman_spectrum(model)
    assert _rel_err(spec.polarizability_ts, g["md/alpha_ts"]) < REL
    assert _rel_err(spec.polarizability_ts, r["md64/alpha_ts"]) < REL
    w, i = spec.measure()
    np.testing.assert_allclose(w, g["md/wavenumbers"], rtol=1e-12)
    scale = np.abs(r["md64/int_raw"]).max()
    err64 = np.abs(i - r["md64/int_raw"]).max() / scale
    err32 = np.abs(i - g["md/int_raw"]).max() / scale
    print(f"MD spectrum: device f32 vs reference f64 {err64:.2e}, vs reference f32 {err32:.2e}, "
          f"reference f32 vs f64 {float(r['md64/ref_f32_vs_f64']):.2e}")
    assert err64 < REL and err32 < REL


@pytest.mark.parametrize("steps", [3, 4, 258, 4097, 10_000])
def test_md_spectrum_on_device_matches_host(steps):
    """the device reduction of a polarizability time series (one batched FFT,
    one weighted power spectrum, two more FFTs) against the host restatement of
    MDRamanSpectrum.measure, odd and even lengths, with and without corrections."""
    from ramannoodle_amd.spectrum import MDRamanSpectrum
    rng = np.random.default_rng(steps)
    t = np.arange(steps)[:, None, None]
    alpha = rng.normal(size=(steps, 3, 3)) * 0.1 + np.sin(0.05 * t * (1 + np.arange(9).reshape(3, 3)))
    alpha = alpha + np.swapaxes(alpha, 1, 2)
    spectrum = MDRamanSpectrum(alpha, 1.5)
    for kwargs in ({}, {"laser_correction": True, "laser_wavelength": 532, "bose_einstein_correction": True,
                        "temperature": 250}):
        w_host, i_host = spectrum.measure(**kwargs)
        w_dev, i_dev = spectrum.measure(device=0, **kwargs)
        assert w_dev.shape == w_host.shape == i_dev.shape
        np.testing.assert_array_equal(w_dev, w_host)
        if len(i_host):
            assert np.abs(i_dev - i_host).max() < 1e-10 * np.abs(i_host).max()


def test_md_spectrum_on_device_matches_reference_fixture():
    """Same reduction on the reference's own polarizability time series: its spectrum
    (``md/int_raw``, ``md/int_corr`` of the fixture) to 1e-9 of the spectrum's scale."""
    from ramannoodle_amd.spectrum import MDRamanSpectrum
    g = load_golden("triclinic20")
    spectrum = MDRamanSpectrum(g["md/alpha_ts"], float(g["md/timestep"]))
    w, i = spectrum.measure(device=0)
    np.testing.assert_allclose(w, g["md/wavenumbers"], rtol=1e-12)
    assert np.abs(i - g["md/int_raw"]).max() < 1e-9 * np.abs(g["md/int_raw"]).max()
    w_host, i_host = spectrum.measure()
    assert np.abs(i_host - g["md/int_raw"]).max() < 1e-9 * np.abs(g["md/int_raw"]).max()


def test_md_spectrum_device_resident_and_plan_cache():
    """SURVEY 8f item 3 as designed: ``Trajectory.get_raman_spectrum(model, on_device=True)`` keeps
    alpha(t) in HBM and ``measure`` reduces it there (``rn_md_raman_intensities_device``, cached
    hipFFT plans): same spectrum as the host path from the same alpha(t); more series lengths than
    the plan cache holds, revisited, still give the right answer."""
    from ramannoodle_amd.dynamics import Trajectory
    from ramannoodle_amd.spectrum import DeviceMDRamanSpectrum, MDRamanSpectrum
    g = load_golden("triclinic20")
    model = product_model_from_golden(g)
    traj = Trajectory(g["md/positions"], float(g["md/timestep"]))
    on_host = traj.get_raman_spectrum(model)
    on_dev = traj.get_raman_spectrum(model, on_device=True)
    assert isinstance(on_dev, DeviceMDRamanSpectrum) and on_dev._device_ts.is_cuda
    for kwargs in ({}, {"laser_correction": True, "laser_wavelength": 532, "bose_einstein_correction": True,
                        "temperature": 250}):
        w_h, i_h = on_host.measure(**kwargs)
        w_d, i_d = on_dev.measure(**kwargs)
        np.testing.assert_array_equal(w_d, w_h)
        assert np.abs(i_d - i_h).max() < 1e-10 * np.abs(i_h).max()
        w_x, i_x = on_dev.measure(host=True, **kwargs)  # host reduction of the same device series
        assert np.abs(i_x - i_h).max() < 1e-12 * np.abs(i_h).max()
    np.testing.assert_array_equal(on_dev.polarizability_ts, on_host.polarizability_ts)
    rng = np.random.default_rng(1)
    series = {}
    for steps in (50, 51, 64, 100, 257, 1000, 50, 257, 51):  # 6 lengths > 4 cache entries, then revisits
        if steps not in series:
            a = rng.normal(size=(steps, 3, 3))
            series[steps] = a + np.swapaxes(a, 1, 2)
        a = series[steps]
        w_h, i_h = MDRamanSpectrum(a, 0.7).measure()
        w_d, i_d = DeviceMDRamanSpectrum(torch.tensor(a, device="cuda"), 0.7).measure()
        np.testing.assert_array_equal(w_d, w_h)
        assert np.abs(i_d - i_h).max() < 1e-10 * np.abs(i_h).max(), steps
    with pytest.raises(ValueError, match="incompatible"):
        Trajectory(g["md/positions"][:, :-1], 1.0).get_raman_spectrum(model, on_device=True)


def test_streamed_trajectory_files(tmp_path):
    """SURVEY 8f item 4 end to end on the GPU: XDATCAR and vasprun.xml written from one trajectory,
    streamed block by block through page-locked buffers and the pipelined entry point
    (``rn_potgnn_calc_polarizabilities_async``: parse k+2 | copy k+1 | evaluate k) -- same bits as
    evaluating the parsed trajectory in one call."""
    from ramannoodle_amd.io.vasp import vasprun, xdatcar
    g = load_golden("rocksalt64_parity")
    model = product_model_from_golden(g)
    rng = np.random.default_rng(4)
    frames, n = 333, g["positions"].shape[0]
    pos = g["positions"][None] + rng.normal(scale=4e-3, size=(frames, n, 3))  # some coordinates < 0: wrapped
    xd = tmp_path / "XDATCAR"
    with open(xd, "w", encoding="utf-8") as f:
        lat = g["lattice"]
        f.write("cell\n 1.0\n" + "".join("  %.10f %.10f %.10f\n" % tuple(r) for r in lat))
        f.write(" Mg O\n %d %d\n" % (n // 2, n - n // 2))
        for k in range(frames):
            f.write(f"Direct configuration= {k + 1}\n" + "".join("  %.12f %.12f %.12f\n" % tuple(r) for r in pos[k]))
    vr = tmp_path / "vasprun.xml"
    with open(vr, "w", encoding="utf-8") as f:
        f.write('<?xml version="1.0"?>\n<modeling>\n <parameters><separator name="ionic"><i name="POTIM"> 1.5</i>'
                "</separator></parameters>\n")
        for k in range(frames):
            f.write(' <structure>\n  <varray name="positions" >\n'
                    + "".join("   <v> %.12f %.12f %.12f </v>\n" % tuple(r) for r in pos[k]) + "  </varray>\n </structure>\n")
        f.write("</modeling>\n")
    parsed = xdatcar.read_positions_ts(xd)
    np.testing.assert_array_equal(parsed, vasprun.read_positions_ts(vr))
    want = model.calc_polarizabilities(parsed - parsed // 1)
    for reader, path in ((xdatcar, xd), (vasprun, vr)):
        for chunk in (64, 1000):
            got = reader.stream_polarizabilities(model, path, chunk_frames=chunk)
            np.testing.assert_array_equal(got, want)
    traj = vasprun.read_trajectory(vr)
    assert traj.timestep == 1.5
    np.testing.assert_array_equal(traj.get_raman_spectrum(model).polarizability_ts, want)
    # the pipelined entry point on its own, pageable memory, three calls in flight
    outs = [np.empty((100, 3, 3)) for _ in range(3)]
    blocks = [np.ascontiguousarray((parsed - parsed // 1)[100 * k:100 * (k + 1)]) for k in range(3)]
    for b, o in zip(blocks, outs):
        model.calc_polarizabilities_async(b, o)
    model.wait()
    np.testing.assert_array_equal(np.concatenate(outs), want[:300])


def test_full_size_properties():
    """Config 2 size (128 atoms, 18 neighbours, perf widths): properties that need no
    oracle -- chunk independence, lattice-translation invariance, symmetric output."""
    from bench import make_workload
    wl = make_workload(num_cells=(4, 2, 2), frames=1000, hparams="perf", seed=22)  # BASELINE config 2 at its full size
    model = wl["model"](max_chunk_structures=0)
    small = wl["model"](max_chunk_structures=37)
    pos = wl["positions"]
    assert pos.shape == (1000, 128, 3) and model.num_edges == 2304
    a = model.calc_polarizabilities(pos)
    np.testing.assert_array_equal(a, small.calc_polarizabilities(pos))
    np.testing.assert_array_equal(a, np.swapaxes(a, 1, 2))
    perm = np.random.default_rng(3).permutation(len(pos))
    np.testing.assert_array_equal(model.calc_polarizabilities(pos[perm]), a[perm])
    shift = np.random.default_rng(1).integers(-2, 3, size=(1,) + pos.shape[1:]).astype(np.float64)
    b = model.calc_polarizabilities(pos[:200] + shift)
    assert _rel_err(b, a[:200]) < REL
    from oracle import potgnn_oracle as O
    orc = O.calc_polarizabilities(wl["oracle"](), pos[:2], faithful=False)
    assert _rel_err(a[:2], orc) < REL


def test_config3_full_size_properties_at_the_documented_widths():
    """BASELINE config 3's cell and trajectory at full size (256 atoms, 10 000 frames) on the reference's documented
    hyper-parameters (Fn = 5, Fe = 14: the narrow kernels, edge rows in destination order): frames are independent -- a
    permutation of the batch permutes the result bit-exactly, pieces give the bits of the whole whatever the work chunks --,
    the host entry (float32 staging) and the device-resident entry (float64 positions) agree bit for bit, outputs are
    symmetric and finite, lattice translations change nothing beyond float32 round-off, and the first frames match the
    oracle."""
    from bench import make_workload
    from oracle import potgnn_oracle as O
    wl = make_workload(num_cells=(4, 4, 2), frames=10_000, hparams="parity", seed=33)
    model = wl["model"]()
    pos = wl["positions"]
    assert model.config_flags()["narrow_kernels"] and model.num_edges == 4608 and model.num_triplets == 78336
    a = model.calc_polarizabilities(pos)
    assert a.shape == (10_000, 3, 3) and np.isfinite(a).all()
    np.testing.assert_array_equal(a, np.swapaxes(a, 1, 2))
    perm = np.random.default_rng(7).permutation(len(pos))
    np.testing.assert_array_equal(model.calc_polarizabilities(pos[perm]), a[perm])
    pieces = np.concatenate([model.calc_polarizabilities(pos[lo:hi])
                             for lo, hi in ((0, 1), (1, 778), (778, 4099), (4099, 10_000))])
    np.testing.assert_array_equal(pieces, a)
    resident = model.calc_polarizabilities_device(torch.tensor(pos, device="cuda"), synchronize=True).cpu().numpy()
    np.testing.assert_array_equal(resident, a)
    shift = np.random.default_rng(1).integers(-2, 3, size=(1,) + pos.shape[1:]).astype(np.float64)
    assert _rel_err(model.calc_polarizabilities(pos[:500] + shift), a[:500]) < REL
    assert np.abs(a - a.mean(axis=0)).max() > 1e2 * REL * np.abs(a).max()
    assert _rel_err(a[:3], O.calc_polarizabilities(wl["oracle"](), pos[:3], faithful=False)) < REL


def test_config3_full_size_properties():
    """BASELINE config 3 at full size (256 atoms, E = 4608, T = 78336, 10 000 MD frames, perf widths):
    what must hold without an oracle -- frames are independent (any permutation of the batch
    permutes the result bit-exactly, whatever chunk and lane a frame lands in), pieces of the
    trajectory give the same bits as the whole, outputs are symmetric and finite, and shifting
    atoms by lattice vectors changes nothing beyond float32 round-off."""
    from bench import make_workload
    wl = make_workload(num_cells=(4, 4, 2), frames=10_000, hparams="perf", seed=33)
    model = wl["model"]()
    pos = wl["positions"]
    assert pos.shape == (10_000, 256, 3) and model.num_edges == 4608 and model.num_triplets == 78336
    a = model.calc_polarizabilities(pos)
    assert a.shape == (10_000, 3, 3) and np.isfinite(a).all()
    np.testing.assert_array_equal(a, np.swapaxes(a, 1, 2))
    perm = np.random.default_rng(7).permutation(len(pos))
    np.testing.assert_array_equal(model.calc_polarizabilities(pos[perm]), a[perm])
    pieces = np.concatenate([model.calc_polarizabilities(pos[lo:hi])
                             for lo, hi in ((0, 1), (1, 778), (778, 4099), (4099, 10_000))])
    np.testing.assert_array_equal(pieces, a)
    shift = np.random.default_rng(1).integers(-2, 3, size=(1,) + pos.shape[1:]).astype(np.float64)
    assert _rel_err(model.calc_polarizabilities(pos[:500] + shift), a[:500]) < REL
    # the trajectory is not degenerate: frames differ by far more than the tolerance
    assert np.abs(a - a.mean(axis=0)).max() > 1e2 * REL * np.abs(a).max()
    # the first two frames against the REFERENCE's own float32 and float64 evaluation of this
    # very model and trajectory (tests/golden/perf256_frames.npz) and against the oracle
    ref = load_golden("perf256_frames")
    np.testing.assert_array_equal(pos[:2], ref["positions"])
    state = model.state_dict()
    np.testing.assert_array_equal(state["_edge_blocks.3.c3_linear.weight"][:2, :8].numpy(), ref["probe_weight"])
    for key in ("alpha32", "alpha64"):
        std_got, std_ref = (a[:2] - ref["mean"]) / ref["std"], (ref[key] - ref["mean"]) / ref["std"]
        assert _rel_err(std_got, std_ref) < REL, key
        assert _rel_err(a[:2], ref[key]) < REL, key
    from oracle import potgnn_oracle as O
    assert _rel_err(a[:2], O.calc_polarizabilities(wl["oracle"](), pos[:2], faithful=False)) < REL


def test_config4_full_size_properties():
    """BASELINE config 4 at full size (256 atoms, 768 modes, +-delta = 1536 displaced cells): the
    float64 finite-difference Raman tensors and the analytic reverse-mode ones are two
    independent routes to the same derivative (agreement O(delta^2)); the analytic map is
    linear in the displacement; the spectrum built from them is finite and non-trivial."""
    from bench import make_workload
    from ramannoodle_amd.dynamics import Phonons
    wl = make_workload(num_cells=(4, 4, 2), frames=2, hparams="perf", seed=33)
    model = wl["model"]()
    rng = np.random.default_rng(44)
    n = model.num_atoms
    qmat, _ = np.linalg.qr(rng.normal(size=(3 * n, 3 * n)))
    mass = np.where(np.arange(n) % 2 == 0, 24.305, 15.999)
    disp = (qmat.T.reshape(3 * n, n, 3) / np.sqrt(mass)[None, :, None]) / np.diag(wl["lattice"])[None, None, :]
    ref = wl["positions"][0]  # a thermally displaced frame (the ideal sites are inversion centres)
    spectrum = Phonons(ref, np.linspace(50.0, 900.0, 3 * n), disp).get_raman_spectrum(model)
    fd = spectrum.raman_tensors
    assert fd.shape == (768, 3, 3) and np.isfinite(fd).all()
    analytic = model.calc_raman_tensors(ref, disp, method="analytic")
    scale = np.abs(fd).max()
    assert scale > 0 and np.abs(analytic - fd).max() < 1e-6 * scale
    mix = rng.normal(size=(5, 768))
    combined = model.calc_raman_tensors(ref, np.einsum("km,mnc->knc", mix, disp), method="analytic")
    np.testing.assert_allclose(combined, np.einsum("km,mij->kij", mix, analytic), rtol=0,
                               atol=1e-9 * np.abs(combined).max())
    wavenumbers, intensities = spectrum.measure(laser_correction=True, laser_wavelength=532)
    assert wavenumbers.shape == (768,) and np.isfinite(intensities).all() and intensities.max() > 0


def test_fused_edge_block_equals_unfused(monkeypatch):
    """The opt-in fused EdgeBlock kernel (MFMA projections + triplet stage in one launch) and
    the default kernel chain are two implementations of the same math; so are the two lane
    widths of the aggregation kernel and the interleaved / sequential schedules."""
    from bench import make_workload
    wl = make_workload(num_cells=(2, 2, 2), frames=9, hparams="perf", seed=3)
    monkeypatch.setenv("RN_POTGNN_FUSED", "0")
    m0 = wl["model"]()
    unfused = m0.calc_polarizabilities(wl["positions"])
    assert not m0.config_flags()["fused_edge_block"]
    monkeypatch.setenv("RN_POTGNN_FUSED", "1")
    m1 = wl["model"]()
    fused = m1.calc_polarizabilities(wl["positions"])
    assert m1.config_flags()["fused_edge_block"]
    assert _rel_err(fused, unfused) < 5e-6
    monkeypatch.setenv("RN_POTGNN_FUSED", "0")
    monkeypatch.setenv("RN_POTGNN_VPL", "8")
    wide = wl["model"]().calc_polarizabilities(wl["positions"])
    assert _rel_err(wide, unfused) < 2e-6
    monkeypatch.setenv("RN_POTGNN_VPL", "4")
    monkeypatch.setenv("RN_POTGNN_INTERLEAVE", "0")
    seq = wl["model"]().calc_polarizabilities(wl["positions"])
    np.testing.assert_array_equal(seq, unfused)


@pytest.mark.parametrize("edge_ps", ["1", "0"])
def test_repeated_evaluation_is_bit_identical(monkeypatch, edge_ps):
    """No kernel uses atomics: evaluating the same frames again must give the same bits, whichever
    workgroup a frame lands in.  Perf and parity widths; with the role-specialised EdgeBlock (the default, split
    products on the K = 32 f16 MFMA like every other kernel) and with ``RN_POTGNN_EDGE_PS=0``, which since round 5 hands
    the EdgeBlock of the fused pipeline to the unfused chain (the per-frame fused kernel that was NOT reproducible on the
    K = 32 instruction is retired: ``profiles/r04/mfma_k32.txt`` and git history)."""
    from bench import make_workload
    monkeypatch.setenv("RN_POTGNN_EDGE_PS", edge_ps)
    for hparams, frames in (("perf", 3000), ("parity", 3000)):
        wl = make_workload(num_cells=(4, 4, 2), frames=frames, hparams=hparams, seed=33)
        model = wl["model"]()
        if hparams == "perf":
            assert model.config_flags()["role_split_edge_block"] == (edge_ps == "1")
        first = model.calc_polarizabilities(wl["positions"])
        for _ in range(2):
            np.testing.assert_array_equal(model.calc_polarizabilities(wl["positions"]), first)
        half = model.calc_polarizabilities(wl["positions"][frames // 2:])
        np.testing.assert_array_equal(half, first[frames // 2:])


def test_split_f16_mfma_matches_exact_f32_mfma(monkeypatch):
    """The fused kernels' matrix products run as three split-f16 MFMAs (hi/lo operands, f32
    accumulation) by default; RN_POTGNN_MFMA=f32 selects the exact-f32 MFMA.  Both must agree with
    each other to float32 round-off and with the float64 oracle to the same margin."""
    from bench import make_workload
    from oracle import potgnn_oracle as O
    wl = make_workload(num_cells=(2, 2, 2), frames=6, hparams="perf", seed=3)
    monkeypatch.setenv("RN_POTGNN_MFMA", "f32")
    m32 = wl["model"]()
    a32 = m32.calc_polarizabilities(wl["positions"])
    assert not m32.config_flags()["split_f16_mfma"]
    monkeypatch.delenv("RN_POTGNN_MFMA")
    m16 = wl["model"]()
    a16 = m16.calc_polarizabilities(wl["positions"])
    assert m16.config_flags()["split_f16_mfma"] and m16.config_flags()["fused_edge_block"]
    oracle = wl["oracle"]().to(torch.float64)
    want = O.calc_polarizabilities(oracle, wl["positions"], faithful=False)
    std = lambda a: (a - oracle.mean) / oracle.std  # noqa: E731
    e16, e32 = _rel_err(std(a16), std(want)), _rel_err(std(a32), std(want))
    print(f"standardised alpha vs float64 oracle: split-f16 MFMA {e16:.2e}, exact-f32 MFMA {e32:.2e}, "
          f"between them {_rel_err(std(a16), std(a32)):.2e}")
    assert e16 < REL / 2 and e32 < REL / 2 and _rel_err(std(a16), std(a32)) < REL / 2


@pytest.mark.parametrize("scale", [2.0 ** -12, 2.0 ** -6, 2.0 ** 8, "outlier"])
def test_split_f16_mfma_is_scale_invariant(scale):
    """The split-f16 products must not care about the scale of a weight matrix: every Linear that
    feeds a LayerNorm (c1, c2, c3 of each pass) is multiplied as a whole by 2^-12, 2^-6 or 2^8 -- the
    LayerNorm makes that scale a free parameter of the model, and an unscaled f16 split would carry
    2^-25 ABSOLUTE error per weight -- or gets one entry of 7e4 (beyond f16's largest finite value).
    The fused path on prescaled weights (kernels.hpp: mfma_prescale) must stay as close to the float64
    oracle as in test_split_f16_mfma_matches_exact_f32_mfma and must not fall back to float32."""
    from oracle import potgnn_oracle as O
    g = load_golden("rocksalt64_parity")
    model, oracle = _random_model(g, 3.2, 64, 64, 2, seed=64064)
    state = model.state_dict()
    rng = np.random.default_rng(9)
    for key, value in state.items():
        if key.endswith(("c1_linear.weight", "c2_linear.weight", "c3_linear.weight")):
            if scale == "outlier":
                value[int(rng.integers(value.shape[0])), int(rng.integers(value.shape[1]))] = 7.0e4
            else:
                value.mul_(scale)
        elif key.endswith(("c1_linear.bias", "c2_linear.bias", "c3_linear.bias")) and scale != "outlier":
            value.mul_(scale)
    model.load_state_dict(state)
    oracle.sd = {k: v.clone() for k, v in state.items()}
    oracle = oracle.to(torch.float64)
    rng = np.random.default_rng(5)
    base = g["pos_batch"]
    pos = base[rng.integers(0, len(base), size=5)] + rng.normal(scale=2e-3, size=(5,) + base.shape[1:])
    got = model.calc_polarizabilities(pos)
    flags = model.config_flags()
    assert flags["fused_edge_block"] and flags["split_f16_mfma"] and not flags["mfma_range_fallback"]
    want = O.calc_polarizabilities(oracle, pos, faithful=False)
    err = _rel_err((got - oracle.mean) / oracle.std, (want - oracle.mean) / oracle.std)
    print(f"scale {scale}: standardised alpha vs float64 oracle {err:.2e}")
    assert err < REL / 2


def test_split_f16_range_guard_falls_back_to_float32():
    """What the prescale cannot cover -- readout hidden activations that the weights allow beyond
    f16's range, or a non-finite weight -- makes the handle run the exact-f32 MFMA instantiations and
    say so (``config_flags()["mfma_range_fallback"]``); results then still match the oracle."""
    from oracle import potgnn_oracle as O
    g = load_golden("rocksalt64_parity")
    model, oracle = _random_model(g, 3.2, 64, 64, 1, seed=64164)
    assert model.config_flags()["split_f16_mfma"] and not model.config_flags()["mfma_range_fallback"]
    state = model.state_dict()
    state["_to_polarizability_embedding.0.weight"].mul_(3.0e3)   # |h1| may now reach ~1e5
    model.load_state_dict(state)
    oracle.sd = {k: v.clone() for k, v in state.items()}
    oracle = oracle.to(torch.float64)
    pos = g["pos_batch"][:3]
    got = model.calc_polarizabilities(pos)
    flags = model.config_flags()
    assert flags["fused_edge_block"] and flags["mfma_range_fallback"] and not flags["split_f16_mfma"]
    want = O.calc_polarizabilities(oracle, pos, faithful=False)
    assert _rel_err((got - oracle.mean) / oracle.std, (want - oracle.mean) / oracle.std) < REL


def _random_model(g, cutoff, fn, fe, passes, seed):
    """Product model + oracle with identical random weights on a fixture's geometry."""
    from oracle import potgnn_oracle as O
    from ramannoodle_amd.pmodel import PotGNN
    from ramannoodle_amd.structure import ReferenceStructure
    from bench import synthetic_state
    zs = [int(z) for z in g["atomic_numbers"]]
    ref = ReferenceStructure(zs, g["lattice"], g["positions"])
    rng = np.random.default_rng(seed)
    mean, std = rng.normal(size=(3, 3)), np.abs(rng.normal(size=(3, 3))) + 0.3
    mean, std = mean + mean.T, std + std.T
    torch.manual_seed(seed)
    model = PotGNN(ref, cutoff, fn, fe, passes, 0.0, 5.0, mean, std)
    state = synthetic_state(model, seed)
    # milder Linear weights than the notebook init so that errors are not hidden by saturation
    for k, v in state.items():
        if k.endswith("weight") and v.dim() == 2 and "norm" not in k and "_node_embedding.0" not in k:
            v.mul_(1.0 / np.sqrt(v.shape[1]))
    model.load_state_dict(state)
    edges, trip, tmap = O.build_topology(g["lattice"], g["positions"], zs, cutoff)
    np.testing.assert_array_equal(edges.numpy(), model.ref_edge_indexes)
    oracle = O.OracleModel(g["lattice"], np.array(zs), edges, trip, tmap,
                           {k: v.clone() for k, v in state.items()}, model.gauss_coefficient, fn, fe,
                           passes, mean, std)
    return model, oracle


@pytest.mark.parametrize(
    "case, cutoff, fn, fe, passes",
    [
        ("triclinic20", 3.0, 20, 70, 2),    # pads 32 / 128, 8- and 32-lane groups
        ("triclinic20", 3.4, 33, 17, 1),    # pads 64 / 32
        ("triclinic20", 3.0, 128, 64, 1),   # K = 128 projections (no register prefetch path)
        ("triclinic20", 3.0, 64, 128, 1),
        ("triclinic20", 2.6, 3, 2, 2),      # minimal widths, sparse ragged graph
        ("rocksalt64_parity", 3.2, 16, 16, 3),  # exact (unpadded) 16-wide rows
        ("tio2_notebook", 5.0, 5, 14, 1),   # 47 neighbours per atom, T = 237240
    ],
)
def test_other_widths_and_graphs_against_oracle(case, cutoff, fn, fe, passes):
    """Template paths no fixture exercises (other paddings, lane-group sizes, K = 128, dense and
    ragged graphs): device vs the pinned oracle, indices bit-exact, alpha within 1e-5."""
    from oracle import potgnn_oracle as O
    g = load_golden(case)
    model, oracle = _random_model(g, cutoff, fn, fe, passes, seed=fn * 1000 + fe)
    trip = model.triplets()
    for mine, ref in zip(trip, oracle.trip):
        np.testing.assert_array_equal(mine, ref.numpy())
    pos = g["pos_batch"][:3]
    got = model.calc_polarizabilities(pos)
    want = O.calc_polarizabilities(oracle, pos, faithful=False)
    std_got = (got - oracle.mean) / oracle.std
    std_want = (want - oracle.mean) / oracle.std
    assert _rel_err(std_got, std_want) < REL, (case, fn, fe)


@pytest.mark.parametrize("fn, fe", [(8, 8), (10, 10), (6, 10), (13, 9), (16, 3), (2, 16), (1, 2), (12, 15)])
def test_every_width_up_to_16_takes_the_narrow_kernels(fn, fe):
    """The reference accepts any positive embedding sizes (``_gnn.py:466-473``).  Up to 16 the one-lane-per-row
    kernels serve all of them: exact instantiations for the documented 5 / 14 (and 5 / 5), otherwise the model's
    widths rounded up to multiples of four with the LayerNorm statistics masked.  Against the pinned oracle on
    a ragged graph, three passes."""
    from oracle import potgnn_oracle as O
    g = load_golden("triclinic20")
    model, oracle = _random_model(g, 3.0, fn, fe, 3, seed=fn * 100 + fe)
    pos = g["pos_batch"][:4]
    got = model.calc_polarizabilities(pos)
    assert model.config_flags()["narrow_kernels"]
    want = O.calc_polarizabilities(oracle, pos, faithful=False)
    assert _rel_err((got - oracle.mean) / oracle.std, (want - oracle.mean) / oracle.std) < REL, (fn, fe)


@pytest.mark.parametrize("fn, fe", [(32, 64), (20, 48), (5, 64), (16, 40)])
def test_edge_width_padded_to_64_widens_the_node_width_onto_the_fused_kernels(fn, fe):
    """Fe padded to 64 with a narrower Fn: Fn is padded to 64 as well, so the model runs on the fused MFMA kernels
    (masked LayerNorms) instead of the unfused chain (profiles/r03/width_sweep.txt).  Inference against the
    pinned oracle and the reverse-mode Jacobian against autograd through the float64 oracle, ragged graph."""
    from oracle import potgnn_oracle as O
    g = load_golden("triclinic20")
    model, oracle = _random_model(g, 3.0, fn, fe, 2, seed=fn * 97 + fe)
    pos = g["pos_batch"][:3]
    got = model.calc_polarizabilities(pos)
    assert model.config_flags()["fused_edge_block"]
    want = O.calc_polarizabilities(oracle, pos, faithful=False)
    assert _rel_err((got - oracle.mean) / oracle.std, (want - oracle.mean) / oracle.std) < REL, (fn, fe)
    oracle64 = oracle.to(torch.float64)
    jac_want = O.jacobian(oracle64, pos[1])
    jac_got = model.alpha_jacobian(pos[1], float64=True)
    scale = np.abs(jac_want).max()
    assert np.abs(jac_got - jac_want).max() < 1e-9 * scale, np.abs(jac_got - jac_want).max() / scale


@pytest.mark.parametrize(
    "case, cutoff, fn, fe, passes, frames",
    [
        ("triclinic20", 3.0, 40, 50, 2, 3),       # padded columns in both embeddings
        ("triclinic20", 3.4, 64, 64, 2, 3),       # ragged graph, tiles of unequal size
        ("triclinic20", 2.2, 64, 33, 1, 2),       # atoms with very few neighbours
        ("rocksalt64_parity", 3.2, 64, 64, 2, 21),  # several frames per workgroup
        ("tio2_notebook", 5.0, 64, 64, 1, 2),     # 47 neighbours per atom: one-atom tiles
    ],
)
@pytest.mark.parametrize("fast_gate", [True, False])
def test_fused_edge_block_against_oracle(monkeypatch, case, cutoff, fn, fe, passes, frames, fast_gate):
    """The fused EdgeBlock kernel (MFMA projections + LDS-DMA operand rows + triplet stage in one
    launch) on graphs and widths the bench does not touch, both triplet-loop variants."""
    from oracle import potgnn_oracle as O
    monkeypatch.setenv("RN_POTGNN_FUSED", "1")
    monkeypatch.setenv("RN_POTGNN_NO_FASTG", "0" if fast_gate else "1")
    g = load_golden(case)
    model, oracle = _random_model(g, cutoff, fn, fe, passes, seed=fn * 1000 + fe)
    rng = np.random.default_rng(5)
    base = g["pos_batch"]
    pos = base[rng.integers(0, len(base), size=frames)] + rng.normal(scale=2e-3, size=(frames,) + base.shape[1:])
    got = model.calc_polarizabilities(pos)
    flags = model.config_flags()
    assert flags["fused_edge_block"] and flags["folded_gate_scale"] == fast_gate
    want = O.calc_polarizabilities(oracle, pos, faithful=False)
    std_got = (got - oracle.mean) / oracle.std
    std_want = (want - oracle.mean) / oracle.std
    assert _rel_err(std_got, std_want) < REL, (case, fn, fe)


@pytest.mark.parametrize("knobs", [{"RN_POTGNN_PS_BACK": "1"}, {"RN_POTGNN_EDGE_PS": "0"}, {"RN_POTGNN_NO_FASTG": "1"}])
def test_ring_refused_passes_run_the_unfused_edge_block_in_several_blocks(monkeypatch, knobs):
    """A pass of the fused pipeline that the role-specialised EdgeBlock does not serve -- a graph its ring refuses (forced
    here on TiO2 at 5 A, 47 neighbours per atom, by allowing no ring lookahead at all; the real ring refuses ``blob_ring`` of
    tests/test_dense_graphs_gpu.py, a 66-atom ball, with no knob set), the kernel switched off, a pass without the folded gate scale -- takes the unfused EdgeBlock
    block of frames by block of frames (``forward.hip: edge_unfused_in_blocks``).  With the block forced to 3 frames a 7-frame batch
    walks the multi-block branch (offsets into the node projections, the node rows and the edge rows): against the oracle,
    and bit-equal to the same batch in one block."""
    from oracle import potgnn_oracle as O
    g = load_golden("tio2_notebook")
    for key, value in knobs.items():
        monkeypatch.setenv(key, value)
    cutoff = 5.0 if "RN_POTGNN_PS_BACK" in knobs else 2.0
    rng = np.random.default_rng(9)
    base = g["pos_batch"]
    pos = base[rng.integers(0, len(base), size=7)] + rng.normal(scale=2e-3, size=(7,) + base.shape[1:])
    results = {}
    for block in ("3", None):
        if block is None:
            monkeypatch.delenv("RN_POTGNN_UNFUSED_BLOCK_FRAMES", raising=False)
        else:
            monkeypatch.setenv("RN_POTGNN_UNFUSED_BLOCK_FRAMES", block)
        model, oracle = _random_model(g, cutoff, 64, 64, 2, seed=64064)
        results[block] = model.calc_polarizabilities(pos)
        flags = model.config_flags()
        assert flags["fused_edge_block"] and not flags["role_split_edge_block"]
    np.testing.assert_array_equal(results["3"], results[None])
    want = O.calc_polarizabilities(oracle, pos, faithful=False)
    assert _rel_err((results["3"] - oracle.mean) / oracle.std, (want - oracle.mean) / oracle.std) < REL


@pytest.mark.parametrize("case", ["triclinic20", "rocksalt64_parity", "rocksalt64_perf"])
def test_reverse_mode_jacobian_against_autograd(case):
    """d(vec6)/d(r): device reverse mode vs torch autograd through the float64 oracle."""
    from oracle import potgnn_oracle as O
    g = load_golden(case)
    model = product_model_from_golden(g)
    oracle = O.model_from_arrays(g).to(torch.float64)
    oracle.coefficient = model.gauss_coefficient
    pos = g["pos_batch"][1]
    want = O.jacobian(oracle, pos)
    got64 = model.alpha_jacobian(pos, float64=True)
    scale = np.abs(want).max()
    assert np.abs(got64 - want).max() < 1e-9 * scale, np.abs(got64 - want).max() / scale
    got32 = model.alpha_jacobian(pos, float64=False)
    assert np.abs(got32 - want).max() < 2e-5 * scale, np.abs(got32 - want).max() / scale
    # translating every atom together changes nothing
    assert np.abs(got64.sum(axis=1)).max() < 1e-9 * scale


@pytest.mark.parametrize("case, cutoff, fn, fe", [("tio2_notebook", 5.0, 64, 64), ("tio2_notebook", 5.0, 5, 14),
                                                  ("triclinic20", 3.4, 40, 100), ("triclinic20", 3.0, 24, 20)])
def test_reverse_mode_jacobian_on_other_graphs_and_widths(case, cutoff, fn, fe):
    """The reverse pass where the fixtures do not go: 47 neighbours per atom (one-atom tiles in both EdgeBlock
    kernels), and the unfused chain at padded widths 128 and 32.  float64 against autograd through the oracle,
    float32 against float64."""
    from oracle import potgnn_oracle as O
    g = load_golden(case)
    model, oracle = _random_model(g, cutoff, fn, fe, 1, seed=fn * 7 + fe)
    pos = g["pos_batch"][0]
    want = O.jacobian(oracle.to(torch.float64), pos)
    got64 = model.alpha_jacobian(pos, float64=True)
    scale = np.abs(want).max()
    assert np.abs(got64 - want).max() < 1e-9 * scale, np.abs(got64 - want).max() / scale
    got32 = model.alpha_jacobian(pos, float64=False)
    assert np.abs(got32 - want).max() < 5e-5 * scale, np.abs(got32 - want).max() / scale


def test_analytic_raman_tensors_match_finite_differences():
    """2 (d alpha/d r).d_m vs the reference's float64 +-delta fixture: equal up to O(delta^2)."""
    g = load_golden("triclinic20")
    model = product_model_from_golden(g)
    ref = g["ph/raman_tensors"]
    got = model.calc_raman_tensors(g["positions"], g["ph/displacements"], method="analytic")
    assert _rel_err(got, ref) < 1e-5
    fd = model.calc_raman_tensors(g["positions"], g["ph/displacements"])
    assert _rel_err(fd, ref) < 1e-5
    with pytest.raises(ValueError, match="unsupported method"):
        model.calc_raman_tensors(g["positions"], g["ph/displacements"], method="magic")


def _load_train_case():
    g = load_golden("triclinic20_train")
    model = product_model_from_golden(g)
    s = g["train/target"].shape[0]
    lat = torch.tensor(g["lattice"], dtype=torch.float32).expand(s, 3, 3)
    zs = torch.tensor(g["atomic_numbers"]).expand(s, -1)
    pos = torch.tensor(g["pos_batch"][:s], dtype=torch.float32)
    return g, model, lat, zs, pos


def test_training_step_gradients_match_reference():
    """forward (batch-statistics BatchNorm) + backward on the device against the gradients the
    reference produced for the same batch, weights and MSE targets."""
    g, model, lat, zs, pos = _load_train_case()
    model.train()
    out = model.forward(lat, zs, pos)
    assert out.requires_grad
    np.testing.assert_allclose(out.detach().numpy(), g["train/out"], rtol=0, atol=1e-5)
    loss = torch.nn.MSELoss()(out, torch.tensor(g["train/target"]))
    assert float(loss.detach()) == pytest.approx(float(g["train/loss"]), rel=1e-5)
    loss.backward()
    for name, p in model.named_parameters():
        ref = g["train/grad/" + name]
        assert p.grad is not None, name
        np.testing.assert_allclose(p.grad.numpy(), ref, rtol=0, atol=1.5e-4 * np.abs(ref).max() + 1e-6,
                                   err_msg=name)
    sd = model.state_dict()
    np.testing.assert_allclose(sd["_to_polarizability_embedding.1.running_mean"].numpy(),
                               g["train/running_mean"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(sd["_to_polarizability_embedding.1.running_var"].numpy(),
                               g["train/running_var"], rtol=1e-5, atol=1e-6)
    assert int(sd["_to_polarizability_embedding.1.num_batches_tracked"]) == 1


def test_training_gradients_float64_leg():
    """Why the float32 gradient tolerance is what it is.  The same training step evaluated in float64
    on the device reproduces the REFERENCE's float64 gradients (tests/golden/triclinic20_r2.npz,
    ``train64/*``) to 1e-9 of each parameter's largest gradient; the float32 device gradients are as
    far from that float64 truth as the reference's own float32 run is (``train64/ref_f32_vs_f64``:
    up to 4e-5 of a parameter's largest gradient), within a factor of three."""
    g, model, lat, zs, pos = _load_train_case()
    r = load_golden("triclinic20_r2")
    s = g["train/target"].shape[0]
    # a float64 reference model derives its Gaussian coefficient from a float64 linspace
    # (_gnn.py:63-64; 6e-8 away from the float32 one): give the float64 leg the same number
    model64 = product_model_from_golden(g)
    model64._gauss_coefficient = -0.5 / ((float(g["hp"][5]) - float(g["hp"][4])) / (int(g["hp"][2]) - 1)) ** 2
    out64, loss64, grads64 = model64.train_gradients_f64(g["pos_batch"][:s], g["train/target"])
    np.testing.assert_allclose(out64, r["train64/out"], rtol=0, atol=1e-10)
    assert loss64 == pytest.approx(float(r["train64/loss"]), rel=1e-10)
    worst64 = 0.0
    for name in grads64:
        ref = r["train64/grad/" + name]
        scale = np.abs(ref).max()
        assert np.abs(grads64[name] - ref).max() < 1e-9 * scale + 1e-15, name
        if scale > 1e-12:  # (the bias in front of BatchNorm has no gradient: round-off only, kept out of the summary)
            worst64 = max(worst64, np.abs(grads64[name] - ref).max() / scale)
    model.train()
    out = model.forward(lat, zs, pos)
    torch.nn.MSELoss()(out, torch.tensor(g["train/target"])).backward()
    worst32, worst_ref = 0.0, 0.0
    for name, p in model.named_parameters():
        ref64, ref32 = r["train64/grad/" + name], g["train/grad/" + name]
        scale = np.abs(ref64).max()
        if scale < 1e-12:
            assert np.abs(p.grad.numpy()).max() < 1e-6, name
            continue
        worst32 = max(worst32, np.abs(p.grad.numpy() - ref64).max() / scale)
        worst_ref = max(worst_ref, np.abs(ref32 - ref64).max() / scale)
    print(f"gradients vs reference float64: device f64 {worst64:.1e}, device f32 {worst32:.1e}, "
          f"reference f32 {worst_ref:.1e} (max over parameters of max|diff| / max|grad|)")
    assert worst32 < 3 * worst_ref and worst32 < 1.5e-4


def test_training_step_at_config5_shape():
    """BASELINE config 5's shape: 256-atom cell, Fn = Fe = 64, P = 4, a mini-batch of 32 structures.
    The float64 device step against float64 autograd through the oracle (1e-8; measured on the full
    batch of 32 once: every parameter within 1e-8, 205 s of oracle time), and the float32 device
    step (the product path) against the float64 device step."""
    from bench import make_workload
    from oracle import potgnn_oracle as O
    wl = make_workload(num_cells=(4, 4, 2), frames=32, hparams="perf", seed=55)
    model = wl["model"]()
    pos = wl["positions"]
    rng = np.random.default_rng(55)
    targets = rng.normal(size=(32, 6))
    # float64 device step vs float64 autograd through the oracle on a sub-batch of 6 (the oracle's
    # autograd over 32 structures of this size takes minutes and ~25 GB of host memory)
    sub64 = model.train_gradients_f64(pos[:6], targets[:6])
    oracle = wl["oracle"]().to(torch.float64)
    o_out, o_loss, o_grads = O.train_gradients(oracle, pos[:6], targets[:6])
    np.testing.assert_allclose(sub64[0], o_out, rtol=0, atol=1e-9 * np.abs(o_out).max())
    assert sub64[1] == pytest.approx(o_loss, rel=1e-9)
    for name, ref in o_grads.items():
        scale = np.abs(ref).max()
        assert np.abs(sub64[2][name] - ref).max() < 1e-8 * scale + 1e-12, name
    # the full mini-batch of 32: float32 device step (the product path) vs the float64 device step
    out64, loss64, grads64 = model.train_gradients_f64(pos, targets)
    model.train()
    s = pos.shape[0]
    lat = torch.tensor(wl["lattice"], dtype=torch.float32).expand(s, 3, 3)
    zs = torch.tensor(model._ref_structure.atomic_numbers).expand(s, -1)
    out = model.forward(lat, zs, torch.tensor(pos, dtype=torch.float32))
    torch.nn.MSELoss()(out, torch.tensor(targets, dtype=torch.float32)).backward()
    np.testing.assert_allclose(out.detach().numpy(), out64, rtol=0, atol=2e-5 * np.abs(out64).max())
    worst = 0.0
    for name, p in model.named_parameters():
        scale = np.abs(grads64[name]).max()
        if scale < 1e-12:
            continue
        worst = max(worst, np.abs(p.grad.numpy() - grads64[name]).max() / scale)
    print(f"config-5 shape, batch 32: float32 vs float64 device gradients, worst {worst:.1e} of a parameter's max")
    assert worst < 1e-4  # measured 1.1e-5


def test_training_gradients_with_a_widened_node_width():
    """Fn = 12 / Fe = 40: Fe pads to 64, so Fn is padded to 64 as well (fused kernels, masked LayerNorms) and
    every parameter gradient has to come back through the padding: float64 device step against float64 autograd
    through the oracle, float32 device step (fused taped forward, split-f16 reverse products) against that."""
    from oracle import potgnn_oracle as O
    g = load_golden("triclinic20")
    model, oracle = _random_model(g, 3.0, 12, 40, 2, seed=1240)
    pos = g["pos_batch"][:5]
    rng = np.random.default_rng(7)
    targets = rng.normal(size=(5, 6))
    out64, loss64, grads64 = model.train_gradients_f64(pos, targets)
    o_out, o_loss, o_grads = O.train_gradients(oracle.to(torch.float64), pos, targets)
    np.testing.assert_allclose(out64, o_out, rtol=0, atol=1e-9 * np.abs(o_out).max())
    assert loss64 == pytest.approx(o_loss, rel=1e-9)
    for name, ref in o_grads.items():
        scale = np.abs(ref).max()
        assert np.abs(grads64[name] - ref).max() < 1e-8 * scale + 1e-12, name
    model.train()
    lat = torch.tensor(g["lattice"], dtype=torch.float32).expand(5, 3, 3)
    zs = torch.tensor(model._ref_structure.atomic_numbers).expand(5, -1)
    out = model.forward(lat, zs, torch.tensor(pos, dtype=torch.float32))
    assert model.config_flags()["fused_edge_block"]
    torch.nn.MSELoss()(out, torch.tensor(targets, dtype=torch.float32)).backward()
    for name, p in model.named_parameters():
        scale = np.abs(grads64[name]).max()
        if scale < 1e-12:
            continue
        assert np.abs(p.grad.numpy() - grads64[name]).max() < 2e-4 * scale, name


@pytest.mark.parametrize("fn, fe", [(40, 100), (24, 20), (8, 20), (100, 30)])
def test_training_gradients_on_the_unfused_chain(fn, fe):
    """Widths the fused and narrow kernels do not serve (padded 64/128, 32/32, 16/32, 128/32): the reverse pass with
    K = 16 .. 128 products -- split-f16 row products where K is a multiple of 64, the exact-f32 kernels otherwise,
    the weight-gradient kernel with one to four 32-column tiles: float32 device gradients against the float64
    device step, which is itself pinned to autograd through the oracle."""
    from oracle import potgnn_oracle as O
    g = load_golden("triclinic20")
    model, oracle = _random_model(g, 3.0, fn, fe, 2, seed=fn * 1000 + fe)
    pos = g["pos_batch"][:4]
    rng = np.random.default_rng(8)
    targets = rng.normal(size=(4, 6))
    out64, loss64, grads64 = model.train_gradients_f64(pos, targets)
    o_out, o_loss, o_grads = O.train_gradients(oracle.to(torch.float64), pos, targets)
    assert loss64 == pytest.approx(o_loss, rel=1e-9)
    for name, ref in o_grads.items():
        scale = np.abs(ref).max()
        assert np.abs(grads64[name] - ref).max() < 1e-8 * scale + 1e-12, name
    model.train()
    lat = torch.tensor(g["lattice"], dtype=torch.float32).expand(4, 3, 3)
    zs = torch.tensor(model._ref_structure.atomic_numbers).expand(4, -1)
    out = model.forward(lat, zs, torch.tensor(pos, dtype=torch.float32))
    torch.nn.MSELoss()(out, torch.tensor(targets, dtype=torch.float32)).backward()
    for name, p in model.named_parameters():
        scale = np.abs(grads64[name]).max()
        if scale < 1e-12:
            continue
        assert np.abs(p.grad.numpy() - grads64[name]).max() < 2e-4 * scale, name


@pytest.mark.parametrize("fn, fe", [(5, 14), (64, 64)])
def test_training_gradients_with_six_message_passes(fn, fe):
    """Six passes give 33 weight-gradient products per step, one more than the deferred-reduction table holds: the
    table is flushed mid-pass and the partial-sum arena reused.  float32 device gradients against the float64 step."""
    g = load_golden("triclinic20")
    model, _ = _random_model(g, 3.0, fn, fe, 6, seed=fn + 600)
    pos = g["pos_batch"][:4]
    rng = np.random.default_rng(9)
    targets = rng.normal(size=(4, 6))
    out64, loss64, grads64 = model.train_gradients_f64(pos, targets)
    model.train()
    lat = torch.tensor(g["lattice"], dtype=torch.float32).expand(4, 3, 3)
    zs = torch.tensor(model._ref_structure.atomic_numbers).expand(4, -1)
    out = model.forward(lat, zs, torch.tensor(pos, dtype=torch.float32))
    loss = torch.nn.MSELoss()(out, torch.tensor(targets, dtype=torch.float32))
    loss.backward()
    assert float(loss.detach()) == pytest.approx(loss64, rel=1e-4)
    for name, p in model.named_parameters():
        scale = np.abs(grads64[name]).max()
        if scale < 1e-12:
            continue
        assert np.abs(p.grad.numpy() - grads64[name]).max() < 5e-4 * scale, name


def _adam_run(model, optimizer, lat, zs, pos, targets, steps):
    losses = []
    model.train()
    for it in range(steps):
        sel = slice(0, pos.shape[0]) if it % 2 == 0 else slice(1, pos.shape[0])  # two batch sizes
        out = model.forward(lat[sel], zs[sel], pos[sel])
        loss = torch.nn.MSELoss()(out, targets[sel])
        loss.backward()
        losses.append(float(loss.detach()))
        optimizer.step()
        optimizer.zero_grad()
    return losses


def test_device_resident_training_step_on_cuda_tensors():
    """``train_single_epoch`` moves a batch to the device and takes the loss there (``_train.py:51-75``).  With ``DeviceAdam``
    and CUDA tensors nothing crosses PCIe (``rn_potgnn_train_forward_samples_device`` /
    ``rn_potgnn_train_backward_samples_device``): the output and the loss live on the GPU, and six steps -- two batch sizes,
    strained lattices and substituted species in half of them -- give the weights that the same steps from host tensors give."""
    from ramannoodle_amd.pmodel import DeviceAdam
    g, _, lat, zs, pos = _load_train_case()
    targets = torch.tensor(g["train/target"])
    rng = np.random.default_rng(4)
    lat2 = lat * torch.tensor(1.0 + 0.01 * rng.standard_normal((lat.shape[0], 1, 1)), dtype=lat.dtype)
    kw = dict(lr=2e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-3)
    runs = {}
    for where in ("cpu", "cuda"):
        model = product_model_from_golden(g)
        opt = DeviceAdam(model, **kw)
        model.train()
        losses = []
        for it in range(6):
            sel = slice(0, pos.shape[0]) if it % 2 == 0 else slice(1, pos.shape[0])
            la = (lat2 if it >= 3 else lat)[sel].to(where)
            out = model.forward(la, zs[sel].to(where), pos[sel].to(where))
            assert out.device.type == where and out.requires_grad
            loss = torch.nn.MSELoss()(out, targets[sel].to(where))
            loss.backward()
            losses.append(float(loss.detach()))
            opt.step()
            opt.zero_grad()
        runs[where] = (losses, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    np.testing.assert_allclose(runs["cuda"][0], runs["cpu"][0], rtol=1e-5)
    for k, v in runs["cpu"][1].items():
        # (the loss is summed on another device.  The bias of the Linear ahead of the training-mode BatchNorm has a
        #  mathematically zero gradient: what Adam integrates there is rounding noise divided by its own magnitude, so
        #  that one vector only agrees to the size of a few steps' worth of lr * noise)
        atol = 2e-5 if k == "_to_polarizability_embedding.0.bias" else 2e-6
        np.testing.assert_allclose(runs["cuda"][1][k].numpy(), v.numpy(), rtol=2e-5, atol=atol, err_msg=k)


def test_device_adam_matches_torch_adam():
    """Device-resident training (gradients, Adam moments, weights and BatchNorm buffers stay in
    HBM; ``rn_potgnn_adam_step``) against ``torch.optim.Adam`` on the host copy of the same model,
    fed by the same device gradients (``_train.py:63-76``): six steps, with weight decay."""
    from ramannoodle_amd.pmodel import DeviceAdam
    g, host, lat, zs, pos = _load_train_case()
    targets = torch.tensor(g["train/target"])
    device = product_model_from_golden(g)
    kw = dict(lr=2e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-3)
    host_losses = _adam_run(host, torch.optim.Adam(host.parameters(), **kw), lat, zs, pos, targets, 6)
    opt = DeviceAdam(device, **kw)
    dev_losses = _adam_run(device, opt, lat, zs, pos, targets, 6)
    assert all(p.grad is None for p in device._state_store.values() if isinstance(p, torch.nn.Parameter))
    np.testing.assert_allclose(dev_losses, host_losses, rtol=2e-5)
    assert host_losses[4] < host_losses[0]  # (same batch)
    # evaluation right after the steps runs on the device's weights (no upload in between) ...
    uploads = device._uploaded_version
    a_dev = device.calc_polarizabilities(g["pos_batch"][:5])
    assert device._device_ahead and device._uploaded_version == uploads
    a_host = host.calc_polarizabilities(g["pos_batch"][:5])
    np.testing.assert_allclose(a_dev, a_host, rtol=0, atol=2e-5 * np.abs(a_host).max())
    # ... and state_dict() fetches them
    sd_d, sd_h = device.state_dict(), host.state_dict()
    assert not device._device_ahead
    worst = {}
    for key, ref in sd_h.items():
        got = sd_d[key]
        if not ref.is_floating_point():
            assert int(got) == int(ref) == 6, key
            continue
        worst[key] = float((got - ref).abs().max())
        # a step moves a weight by <= lr = 2e-3; the two Adam implementations round differently and
        # the next step's gradients see that (measured: 1.6e-6 after six steps)
        assert worst[key] < 1e-5, (key, worst[key])
    print("device Adam vs torch Adam after 6 steps: worst |dw| =", max(worst.values()),
          max(worst, key=worst.get))
    # the float64 entry points see the stepped weights too
    j_dev = device.alpha_jacobian(g["pos_batch"][0], float64=True)
    j_host = host.alpha_jacobian(g["pos_batch"][0], float64=True)
    np.testing.assert_allclose(j_dev, j_host, rtol=0, atol=1e-4 * np.abs(j_host).max())
    # handing control back to a host optimiser keeps the values
    device.enable_device_training(False)
    again = device.calc_polarizabilities(g["pos_batch"][:5])
    np.testing.assert_array_equal(again, a_dev)


@pytest.mark.parametrize("batch_size", [1, 4])  # (1: the batch size of the reference's own test_train_single_epoch)
def test_device_adam_through_train_single_epoch(batch_size):
    """``train_single_epoch`` (``_train.py:20-91``) with the device-resident optimiser."""
    from ramannoodle_amd.pmodel import DeviceAdam, train_single_epoch
    g, host, lat, zs, pos = _load_train_case()
    device = product_model_from_golden(g)
    targets = torch.tensor(g["train/target"])
    data = torch.utils.data.TensorDataset(lat, zs, pos, targets)
    torch.manual_seed(3)
    ref = train_single_epoch(host, data, data, batch_size, torch.optim.Adam(host.parameters(), lr=1e-3),
                             torch.nn.MSELoss())
    torch.manual_seed(3)
    got = train_single_epoch(device, data, data, batch_size, DeviceAdam(device, lr=1e-3), torch.nn.MSELoss())
    assert np.isfinite(ref[0]) and np.isfinite(ref[1])
    assert got[0] == pytest.approx(ref[0], rel=1e-4) and got[1] == pytest.approx(ref[1], rel=1e-4)
    np.testing.assert_allclose(got[2], ref[2], rtol=1e-4, atol=1e-7)


def test_device_adam_data_parallel(tmp_path):
    """Two ranks with device-resident training: the packed gradient buffers are averaged in place
    (``parallel.average_gradients``) before ``rn_potgnn_adam_step``; after two steps every rank holds
    what one process training on the whole batch holds."""
    import socket
    import subprocess
    import sys
    from ramannoodle_amd.pmodel import DeviceAdam
    g, single, lat, zs, pos = _load_train_case()
    targets = torch.tensor(g["train/target"])
    opt = DeviceAdam(single, lr=1e-3)
    single.train()
    for _ in range(2):
        torch.nn.MSELoss()(single.forward(lat, zs, pos), targets).backward()
        opt.step()
    want = single.state_dict()
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    out = tmp_path / "dp_device.npz"
    worker = os.path.join(os.path.dirname(__file__), "dp_train_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), "2", str(port), str(out), "device"])
             for r in range(2)]
    codes = [p.wait(timeout=300) for p in procs]
    assert codes == [0, 0], codes
    got = np.load(out)
    # The bias in front of BatchNorm has no gradient in exact arithmetic (batch statistics absorb
    # it); what reaches Adam is rounding noise, which Adam normalises to +-lr per step -- torch's
    # does the same.  Its summation order differs between one and two ranks, so that vector, and the
    # running mean that carries a tenth of it per step, are compared on the scale of the steps.
    loose = {"_to_polarizability_embedding.0.bias": 2.5e-3, "_to_polarizability_embedding.1.running_mean": 5e-4}
    for key, ref in want.items():
        if ref.is_floating_point():
            np.testing.assert_allclose(got["sd/" + key], ref.numpy(), rtol=0, atol=loose.get(key, 2e-5),
                                       err_msg=key)
            np.testing.assert_array_equal(got["sd/" + key], got["sd1/" + key], err_msg=key)  # ranks agree


def test_data_parallel_training_step_matches_reference(tmp_path):
    """Two ranks (gloo, both on this GPU), half of the fixture batch each: BatchNorm statistics
    all-reduced inside the device step and gradients averaged over the ranks must reproduce the
    reference's single-process step on the whole batch."""
    import socket
    import subprocess
    import sys
    g = load_golden("triclinic20_train")
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    out = tmp_path / "dp.npz"
    worker = os.path.join(os.path.dirname(__file__), "dp_train_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), "2", str(port), str(out)]) for r in range(2)]
    codes = [p.wait(timeout=300) for p in procs]
    assert codes == [0, 0], codes
    got = np.load(out)
    np.testing.assert_allclose(got["out"], g["train/out"], rtol=0, atol=1e-5)
    assert float(got["loss"]) == pytest.approx(float(g["train/loss"]), rel=1e-5)
    for key in g.files:
        if key.startswith("train/grad/"):
            ref = g[key]
            np.testing.assert_allclose(got["grad/" + key[len("train/grad/"):]], ref, rtol=0,
                                       atol=1.5e-4 * np.abs(ref).max() + 1e-6, err_msg=key)
    np.testing.assert_allclose(got["running_mean"], g["train/running_mean"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got["running_var"], g["train/running_var"], rtol=1e-5, atol=1e-6)


def test_train_single_epoch_reduces_loss():
    """The reference's training-loop contract (_train.py:24-95) on a synthetic teacher task:
    returns (train loss, validation loss, prediction variance[6]) and learns."""
    from ramannoodle_amd.dataset import PolarizabilityDataset
    from ramannoodle_amd.pmodel import PotGNN, train_single_epoch
    from ramannoodle_amd.structure import ReferenceStructure
    g = load_golden("triclinic20")
    zs = [int(z) for z in g["atomic_numbers"]]
    ref = ReferenceStructure(zs, g["lattice"], g["positions"])
    rng = np.random.default_rng(3)
    pos = g["positions"][None] + rng.normal(0, 0.01, (48,) + g["positions"].shape)
    teacher = product_model_from_golden(g)
    alpha = teacher.calc_polarizabilities(pos)
    train = PolarizabilityDataset(g["lattice"], zs, pos[:40], alpha[:40])
    val = PolarizabilityDataset(g["lattice"], zs, pos[40:], alpha[40:])
    val.scale_polarizabilities(train.mean_polarizability, train.stddev_polarizability)
    torch.manual_seed(0)
    model = PotGNN(ref, 3.0, 8, 12, 2, 0.0, 4.0, train.mean_polarizability, train.stddev_polarizability)
    optimizer = torch.optim.Adam(model.parameters(), lr=0.01)
    losses = [train_single_epoch(model, train, val, 8, optimizer, torch.nn.MSELoss()) for _ in range(6)]
    assert losses[-1][0] < 0.9 * losses[0][0], [l[0] for l in losses]
    assert all(b[0] < a[0] for a, b in zip(losses, losses[1:])), [l[0] for l in losses]
    assert np.isfinite(losses[-1][1]) and losses[-1][2].shape == (6,)
    # evaluation after training uses the updated weights and running statistics
    a = model.calc_polarizabilities(pos[:3])
    assert a.shape == (3, 3, 3) and np.isfinite(a).all()


def test_config5_shape_epochs_learn_with_the_optimiser_on_the_device():
    """BASELINE config 5 at its shape (256-atom cell, Fn = Fe = 64, P = 4, mini-batches of 32, synthetic teacher targets) and
    a sixteenth of its size: three epochs over 768 structures through the reference's `train_single_epoch` with weights,
    gradients and Adam moments resident in HBM -- the loop's return contract holds, the loss falls from epoch to epoch, and
    the evaluation afterwards runs on the trained weights (the 50 000-structure epoch itself: profiles/r06/other_configs.txt)."""
    from bench import make_workload, rocksalt
    from ramannoodle_amd.dataset import PolarizabilityDataset
    from ramannoodle_amd.pmodel import DeviceAdam, train_single_epoch
    wl = make_workload((4, 4, 2), 768, "perf", seed=55)
    teacher = wl["model"]()
    alpha = teacher.calc_polarizabilities(wl["positions"])
    lattice, _, zs = rocksalt(4, 4, 2)
    ds = PolarizabilityDataset(lattice, zs, wl["positions"], alpha)
    val = torch.utils.data.Subset(ds, range(128))
    torch.manual_seed(1)
    student = wl["model"]()
    before = student.calc_polarizabilities(wl["positions"][:4])
    opt = DeviceAdam(student, lr=1e-3)
    losses = [train_single_epoch(student, ds, val, 32, opt, torch.nn.MSELoss()) for _ in range(3)]
    assert all(np.isfinite(l[0]) and np.isfinite(l[1]) and l[2].shape == (6,) for l in losses)
    assert losses[2][0] < losses[1][0] < losses[0][0], [l[0] for l in losses]
    after = student.calc_polarizabilities(wl["positions"][:4])
    assert np.isfinite(after).all() and np.abs(after - before).max() > 0


def test_sharded_entry_points_keep_results_on_the_device():
    """``calc_polarizabilities_sharded`` / ``calc_raman_tensors_sharded`` over RCCL (a one-rank ``nccl``
    group is what one GPU allows): the device path -- evaluation, finite differences and all-gather
    without a host bounce -- returns what the host entry points return."""
    import socket
    import torch.distributed as dist
    from ramannoodle_amd.parallel import calc_polarizabilities_sharded, calc_raman_tensors_sharded
    g = load_golden("triclinic20")
    model = product_model_from_golden(g)
    pos = g["pos_batch"][:9]
    want = model.calc_polarizabilities(pos)
    disp = np.random.default_rng(2).normal(size=(5,) + pos.shape[1:]) * 0.05
    want_rt = model.calc_raman_tensors(g["positions"], disp)
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        np.testing.assert_array_equal(calc_polarizabilities_sharded(model, pos), want)
        got_rt = calc_raman_tensors_sharded(model, g["positions"], disp)
        assert np.abs(got_rt - want_rt).max() <= 1e-9 * np.abs(want_rt).max()  # same float64 kernels; the +- cells are formed on the device
        analytic = calc_raman_tensors_sharded(model, g["positions"], disp, method="analytic")
        # (the reverse pass sums a few cotangents with float64 atomics: equal to rounding, not bit for bit)
        np.testing.assert_allclose(analytic, model.calc_raman_tensors(g["positions"], disp, method="analytic"),
                                   rtol=1e-12, atol=1e-15)
        with pytest.raises(ValueError, match="wrong shape"):
            calc_polarizabilities_sharded(model, pos[:, :-1])
    finally:
        dist.destroy_process_group()


def test_device_radius_graph_bit_exact(golden):
    """K0 on the device: same edge list as the reference (and as the host restatement)."""
    from ramannoodle_amd.pmodel import graph as G
    name, g = golden
    cutoff = float(g["hp"][0])
    edges = G.radius_graph_pbc_device(g["lattice"], g["positions"], cutoff)
    np.testing.assert_array_equal(edges, g["ref_edge_indexes"][1:])
    np.testing.assert_array_equal(edges, G.radius_graph_pbc(g["lattice"], g["positions"], cutoff))


def _bench_line(cmd, env, root):
    import json
    import subprocess
    done = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert done.returncode == 0, done.stderr[-2000:]
    lines = [ln for ln in done.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, done.stdout
    return json.loads(lines[0])


def test_bench_two_ranks_contract(tmp_path):
    """The N > 1 launch the driver uses (torch.distributed.run, one rank per GPU) on this 1-GPU
    box: both ranks share cuda:0 over gloo (RN_BENCH_SHARE_GPU).  Rank 0 prints exactly one JSON
    line with the whole-job rate; the all-gathered result is exercised by the step itself.
    Config 2 = weak scaling, 96 frames per rank."""
    import socket
    import sys
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RN_BENCH_SHARE_GPU="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"),
           "--gpus", "2", "--steps", "2", "--warmup", "1", "--config", "2", "--frames", "96", "--no-cpu", "--full"]
    result = _bench_line(cmd, env, root)
    assert result["n_gpus"] == 2 and result["steps"] == 2 and result["scaling"] == "weak"
    assert result["value"] == pytest.approx(2 * 96 * 2 / (result["ms_per_step"] * 2e-3), rel=1e-6)
    assert result["roofline"]["launches"] > 0 and result["unit"] == "structures/s"
    assert "128 atoms" in result["config"]["workload"]
    # N > 1 extra (--full): the same step from the caller's host array (every rank uploads its block through the staging entry)
    assert result["host_inclusive_structures_per_s"] > 0


def test_bench_single_gpu_line_contract():
    """``python bench.py --full`` at N = 1 (a short trajectory and a 4-frame CPU sample instead of the defaults):
    one JSON line with every key of the bench contract, the roofline object (algorithmic figure,
    committed traffic / issue records only when they match the workload) and the CPU baseline."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "1", "--frames", "60",
           "--cpu-sample", "4", "--cpu-reps", "1", "--full"]
    result = _bench_line(cmd, dict(os.environ), root)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in result, key
    assert result["n_gpus"] == 1 and result["steps"] == 2 and result["warmup"] == 1 and result["higher_is_better"]
    assert result["vs_baseline"] is None and result["dtype"] == "f32" and result["data"] == "synthetic"
    assert result["value"] == pytest.approx(60 * 2 / (result["ms_per_step"] * 2e-3), rel=1e-6)
    assert "256 atoms" in result["config"]["workload"] and result["config"]["total_frames"] == 60
    roof = result["roofline"]
    assert roof["bound"] == "hbm" and roof["unit"] == "GB/s" and roof["peak"] == 8000.0
    assert roof["frac"] == pytest.approx(roof["achieved"] / roof["peak"]) and 0 < roof["frac"] < 1
    assert roof["algorithmic_bytes_per_structure_pass"] == 4 * (256 * 64 + 2 * 4608 * 64)  # B_EB, SURVEY 8d
    # traffic / issue_frac replay committed PMC records -- but only records taken on the kernel source that is in this tree
    # (bench.committed_profile; tests/test_host_logic.py::test_committed_profile_records_are_fresh keeps them so)
    assert roof["traffic"] is not None and roof["issue_frac"] is not None and "profiles/r06" in roof["traffic_source"]
    assert result["host_boundary"]["batch_1_latency_us_per_call"] > 0 and 0 < result["host_boundary"]["host_over_resident"] < 1.5
    cpu = result["cpu_baseline"]
    assert cpu["kind"] == "port" and cpu["cores"] >= 1 and cpu["value"] > 0 and cpu["unit"] == "structures/s"
    exact = result["exact_fp32_mfma"]
    assert exact["structures_per_s"] > 0 and exact["max_rel_diff_of_alpha"] < 1e-5


def test_bench_plain_run_times_the_steps_and_dumps_them(tmp_path):
    """``python bench.py`` without ``--full``: the headline, its roofline and nothing that takes a run of its own; with
    ``--dump-outputs DIR`` the polarizabilities of the last timed step are what the host entry computes on the same
    frames, and a second run writes the same file bit for bit."""
    import sys
    from bench import make_workload
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dumps = []
    for run in range(2):
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "1", "--frames", "60",
               "--dump-outputs", str(tmp_path / str(run))]
        result = _bench_line(cmd, dict(os.environ), root)
        assert result["steps"] == 3 and result["warmup"] == 1 and result["unit"] == "structures/s"
        assert result["value"] == pytest.approx(60 * 3 / (result["ms_per_step"] * 3e-3), rel=1e-6)
        assert result["roofline"]["launches"] > 0
        assert "cpu_baseline" not in result and "documented_hparams" not in result
        assert result["host_boundary"] is None and result["exact_fp32_mfma"] is None
        dumps.append(np.load(tmp_path / str(run) / "polarizabilities.npy"))
    assert dumps[0].shape == (60, 3, 3) and dumps[0].dtype == np.float64
    np.testing.assert_array_equal(dumps[0], dumps[1])
    wl = make_workload((4, 4, 2), 60, "perf", seed=33)  # bench.CONFIGS[3]
    want = wl["model"]().calc_polarizabilities(wl["positions"])
    np.testing.assert_allclose(dumps[0], want, rtol=0, atol=1e-6 * np.abs(want).max())


def test_bench_starts_its_own_ranks(tmp_path):
    """``python bench.py --gpus 2`` with no launcher: the process starts the two ranks itself
    (before touching the GPU) and rank 0 prints the one JSON line.  Default workload = BASELINE
    config 3: the 256-atom cell, ONE trajectory sharded over the ranks (here 97 frames: blocks of
    49 and 48, so the padded all-gather is exercised), strong scaling; the dumped outputs are the
    97 frames without the padding row.  A ``--gpus`` that contradicts WORLD_SIZE is refused."""
    import subprocess
    import sys
    from bench import make_workload
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["RN_BENCH_SHARE_GPU"] = "1"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--frames", "97", "--no-cpu", "--dump-outputs", str(tmp_path)]
    result = _bench_line(cmd, env, root)
    assert result["n_gpus"] == 2 and result["scaling"] == "strong"
    assert "256 atoms" in result["config"]["workload"] and result["config"]["total_frames"] == 97
    assert result["config"]["frames_per_gpu"] == 49 and "sharded x2" in result["config"]["parallelism"]
    assert result["value"] == pytest.approx(97 * 2 / (result["ms_per_step"] * 2e-3), rel=1e-6)
    got = np.load(tmp_path / "polarizabilities.npy")
    wl = make_workload((4, 4, 2), 97, "perf", seed=33)
    want = wl["model"]().calc_polarizabilities(wl["positions"])
    assert got.shape == (97, 3, 3)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6 * np.abs(want).max())
    bad = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--no-cpu"],
                         env=dict(env, WORLD_SIZE="1", RANK="0"), cwd=root, capture_output=True, text=True,
                         timeout=300)
    assert bad.returncode != 0 and "does not match WORLD_SIZE" in bad.stderr


# ----------------------------------------------------------------------------- round 4
@pytest.mark.parametrize("case, cutoff, fn, fe, passes, frames", [
    ("rocksalt64_parity", 3.2, 64, 64, 2, 23),   # regular graph, several frames per workgroup, ragged last unit
    ("triclinic20", 3.4, 64, 64, 2, 5),          # ragged graph: tiles and rounds of unequal size
    ("triclinic20", 3.0, 40, 50, 2, 3),          # padded columns in both embeddings (PAD instantiation)
    ("triclinic20", 2.2, 64, 33, 1, 2),          # atoms with very few neighbours: rounds of a handful of destinations
])
def test_role_split_edge_block_against_oracle_and_per_frame_kernel(monkeypatch, case, cutoff, fn, fe, passes, frames):
    """The role-specialised fused EdgeBlock (producer + consumer waves, ``csrc/kernels_edge_ps.hip``) is what a 64-wide
    float32 evaluation runs on; it agrees with the pinned oracle and with what serves the passes it does not take
    (``RN_POTGNN_EDGE_PS=0``: the unfused EdgeBlock inside the fused pipeline, which replaced the retired per-frame
    kernel in round 5), and repeats bit for bit."""
    from oracle import potgnn_oracle as O
    g = load_golden(case)
    rng = np.random.default_rng(5)
    base = g["pos_batch"]
    pos = base[rng.integers(0, len(base), size=frames)] + rng.normal(scale=2e-3, size=(frames,) + base.shape[1:])
    model, oracle = _random_model(g, cutoff, fn, fe, passes, seed=fn * 13 + fe)
    got = model.calc_polarizabilities(pos)
    assert model.config_flags()["role_split_edge_block"]
    want = O.calc_polarizabilities(oracle, pos, faithful=False)
    assert _rel_err((got - oracle.mean) / oracle.std, (want - oracle.mean) / oracle.std) < REL
    np.testing.assert_array_equal(model.calc_polarizabilities(pos), got)
    monkeypatch.setenv("RN_POTGNN_EDGE_PS", "0")
    per_frame, _ = _random_model(g, cutoff, fn, fe, passes, seed=fn * 13 + fe)
    old = per_frame.calc_polarizabilities(pos)
    assert not per_frame.config_flags()["role_split_edge_block"]
    assert _rel_err((got - oracle.mean) / oracle.std, (old - oracle.mean) / oracle.std) < REL


@pytest.mark.parametrize("case,cutoff,fn,fe,passes,frames", [
    ("rocksalt64_parity", 3.2, 64, 64, 2, 23),   # regular graph: every round full, several frames per workgroup
    ("rocksalt64_parity", 3.2, 64, 64, 1, 300),  # more frames than workgroups: the next frame's rows through the LDS slots
    ("triclinic20", 3.4, 64, 64, 2, 5),          # ragged in-degrees, a last tile of 4 atoms
    ("triclinic20", 3.0, 40, 50, 2, 3),          # padded columns in both embeddings (PAD instantiation)
    ("triclinic20", 2.2, 64, 33, 1, 2),          # atoms with one or two in-edges: fewer rounds than the ring is deep
])
def test_atom_owning_node_block_against_oracle_and_row_kernel(monkeypatch, case, cutoff, fn, fe, passes, frames):
    """The atom-owning fused NodeBlock (``csrc/kernels_node_atom.hip``: tiles of 16 atoms, round r = their r-th in-edges,
    the gate on the MFMA accumulators) agrees with the pinned oracle and with the row-ordered kernel it replaces
    (``RN_POTGNN_NODE_ATOM=0``), and repeats bit for bit."""
    from oracle import potgnn_oracle as O
    g = load_golden(case)
    rng = np.random.default_rng(11)
    base = g["pos_batch"]
    pos = base[rng.integers(0, len(base), size=frames)] + rng.normal(scale=2e-3, size=(frames,) + base.shape[1:])
    monkeypatch.setenv("RN_POTGNN_NODE_ATOM", "1")
    model, oracle = _random_model(g, cutoff, fn, fe, passes, seed=fn * 7 + fe)
    got = model.calc_polarizabilities(pos)
    assert model.config_flags()["atom_owning_node_block"]
    check = pos[:: max(1, frames // 8)]
    want = O.calc_polarizabilities(oracle, check, faithful=False)
    assert _rel_err((got[:: max(1, frames // 8)] - oracle.mean) / oracle.std, (want - oracle.mean) / oracle.std) < REL
    np.testing.assert_array_equal(model.calc_polarizabilities(pos), got)
    monkeypatch.setenv("RN_POTGNN_NODE_ATOM", "0")
    rows, _ = _random_model(g, cutoff, fn, fe, passes, seed=fn * 7 + fe)
    old = rows.calc_polarizabilities(pos)
    assert not rows.config_flags()["atom_owning_node_block"]
    assert _rel_err((got - oracle.mean) / oracle.std, (old - oracle.mean) / oracle.std) < REL


@pytest.mark.parametrize("case,cutoff,fn,fe,passes,frames", [
    ("rocksalt64_parity", 3.2, 64, 64, 3, 40),
    ("triclinic20", 3.4, 64, 64, 2, 5),
    ("triclinic20", 3.0, 40, 50, 2, 3),          # padded columns (zeros in the pair rows too)
])
def test_split_f16_pair_rows_against_oracle_and_float32_rows(monkeypatch, case, cutoff, fn, fe, passes, frames):
    """Edge rows stored as the split-f16 operand pairs (written once by the geometry kernel / the EdgeBlock epilogue, read as they
    are by the NodeBlock, the next EdgeBlock and the readout) give what plain float32 rows give (``RN_POTGNN_PAIR_ROWS=0``): the
    MFMA operands are the same bits, only the residual ``tanh(edge + c2 + c3)`` sees ``hi + lo`` (2^-25 absolute) for ``edge``."""
    from oracle import potgnn_oracle as O
    g = load_golden(case)
    rng = np.random.default_rng(17)
    base = g["pos_batch"]
    pos = base[rng.integers(0, len(base), size=frames)] + rng.normal(scale=2e-3, size=(frames,) + base.shape[1:])
    monkeypatch.setenv("RN_POTGNN_NODE_ATOM", "1")
    model, oracle = _random_model(g, cutoff, fn, fe, passes, seed=fn + 3 * fe)
    got = model.calc_polarizabilities(pos)
    flags = model.config_flags()
    assert flags["role_split_edge_block"] and flags["atom_owning_node_block"] and flags["split_f16_pair_rows"]
    want = O.calc_polarizabilities(oracle, pos[:6], faithful=False)
    assert _rel_err((got[:6] - oracle.mean) / oracle.std, (want - oracle.mean) / oracle.std) < REL
    np.testing.assert_array_equal(model.calc_polarizabilities(pos), got)
    monkeypatch.setenv("RN_POTGNN_PAIR_ROWS", "0")
    plain, _ = _random_model(g, cutoff, fn, fe, passes, seed=fn + 3 * fe)
    old = plain.calc_polarizabilities(pos)
    assert not plain.config_flags()["split_f16_pair_rows"]
    assert _rel_err((got - oracle.mean) / oracle.std, (old - oracle.mean) / oracle.std) < 2e-6


def test_centred_weight_copies_follow_a_device_resident_step():
    """The role-specialised EdgeBlock multiplies with copies of c3_linear / c2_linear centred over their output columns.
    After a device-resident Adam step those copies are recomputed on the device (``refresh_derived_kernel`` kind 3):
    an evaluation right after the steps equals the one of a fresh model built from the stepped ``state_dict()``."""
    from ramannoodle_amd.pmodel import DeviceAdam
    g = load_golden("triclinic20")
    model, _ = _random_model(g, 3.0, 64, 64, 2, seed=77)
    s = 4
    pos = torch.tensor(g["pos_batch"][:s])
    lat = torch.tensor(g["lattice"]).expand(s, 3, 3)
    zs = torch.tensor(g["atomic_numbers"]).expand(s, -1)
    targets = torch.tensor(np.random.default_rng(3).normal(size=(s, 6)), dtype=torch.float32)
    _adam_run(model, DeviceAdam(model, lr=5e-3), lat, zs, pos, targets, 3)
    after = model.calc_polarizabilities(g["pos_batch"][:6])   # device weights, device-centred copies
    assert model.config_flags()["role_split_edge_block"]
    fresh, _ = _random_model(g, 3.0, 64, 64, 2, seed=77)
    fresh.load_state_dict(model.state_dict())                  # host-packed, host-centred copies
    want = fresh.calc_polarizabilities(g["pos_batch"][:6])
    np.testing.assert_allclose(after, want, rtol=0, atol=REL * np.abs(want).max())


def test_device_entry_follows_the_default_dtype():
    """``calc_polarizabilities_device(dtype=None)`` resolves the arithmetic as ``calc_polarizabilities`` does
    (``torch.get_default_dtype()``, ``_gnn.py:705-710``), so the RCCL path of ``parallel.calc_polarizabilities_sharded``
    returns what the host and gloo paths return under ``set_default_dtype(float64)``."""
    g = load_golden("rocksalt64_parity")
    model = product_model_from_golden(g)
    pos = g["pos_batch"][:6]
    dev = torch.tensor(pos, device="cuda")
    host32 = model.calc_polarizabilities(pos)
    np.testing.assert_array_equal(model.calc_polarizabilities_device(dev, synchronize=True).cpu().numpy(), host32)
    torch.set_default_dtype(torch.float64)
    try:
        host64 = model.calc_polarizabilities(pos)
        dev64 = model.calc_polarizabilities_device(dev, synchronize=True).cpu().numpy()
    finally:
        torch.set_default_dtype(torch.float32)
    np.testing.assert_array_equal(dev64, host64)
    assert np.abs(host64 - host32).max() > 0  # (the two arithmetics do differ: the test can tell them apart)
    if "f64/alpha" in g.files:
        assert _rel_err(dev64, g["f64/alpha"][:6]) < 1e-9


def test_two_threads_on_two_handles_and_on_one():
    """C-ABI threading contract (``include/rn_potgnn.h``): distinct handles run concurrently from distinct threads; calls
    on ONE handle from several threads are serialised by the handle's lock.  Either way every thread gets the
    single-threaded result."""
    import threading
    g = load_golden("rocksalt64_parity")
    a, _ = _random_model(g, 3.2, 64, 64, 2, seed=1)
    b, _ = _random_model(g, 3.2, 64, 64, 2, seed=2)
    pos = np.concatenate([g["pos_batch"]] * 8)
    want = {"a": a.calc_polarizabilities(pos), "b": b.calc_polarizabilities(pos)}
    assert np.abs(want["a"] - want["b"]).max() > 0
    results, errors = {}, []

    def run(key, model, reps):
        try:
            for r in range(reps):
                results[(key, threading.get_ident(), r)] = (key, model.calc_polarizabilities(pos))
        except BaseException as exc:  # pylint: disable=broad-except
            errors.append(exc)

    threads = [threading.Thread(target=run, args=("a", a, 3)), threading.Thread(target=run, args=("b", b, 3)),
               threading.Thread(target=run, args=("a", a, 3))]   # the third shares handle `a` with the first
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(results) == 9
    for key, got in results.values():
        np.testing.assert_array_equal(got, want[key])


def test_forward_with_cuda_tensors_stays_on_the_device():
    """``forward`` on CUDA tensors (the reference's ``test_gnn.py:130-160`` runs under ``set_default_device``; its
    ``train_single_epoch`` moves every batch to the device, ``_train.py:51-75``): the inputs are read where they are, the
    result is a CUDA tensor, and it equals the host path bit for bit -- reference lattice and species, per-sample
    lattices, per-sample species."""
    g, r2, r3 = load_golden("triclinic20"), load_golden("triclinic20_r2"), load_golden("triclinic20_r3")
    model = product_model_from_golden(g).eval()
    pos0 = g["pos_batch"][:6]
    cases = [(np.broadcast_to(g["lattice"], (len(pos0), 3, 3)).copy(),
              np.broadcast_to(g["atomic_numbers"], (len(pos0), len(g["atomic_numbers"]))).copy(), pos0),
             (r2["lat/lattices"], np.broadcast_to(g["atomic_numbers"], (len(r2["lat/positions"]), len(g["atomic_numbers"]))).copy(),
              r2["lat/positions"]),
             (r3["zs/lattices"], r3["zs/atomic_numbers"], r3["zs/positions"])]
    for lat, zs, pos in cases:
        host = model.forward(torch.tensor(lat), torch.tensor(zs), torch.tensor(pos))
        assert not host.is_cuda
        dev = model.forward(torch.tensor(lat, device="cuda"), torch.tensor(zs, device="cuda"), torch.tensor(pos, device="cuda"))
        assert dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == (len(pos), 6)
        np.testing.assert_array_equal(dev.cpu().numpy(), host.numpy())
        # float32 device tensors (what a DataLoader of the reference's dataset yields) work as well
        dev32 = model.forward(torch.tensor(lat, device="cuda", dtype=torch.float32), torch.tensor(zs, device="cuda"),
                              torch.tensor(pos, device="cuda", dtype=torch.float32))
        assert dev32.is_cuda
    unknown = r3["zs/atomic_numbers"].copy()
    unknown[1, 3] = 79
    with pytest.raises(IndexError):
        model.forward(torch.tensor(r3["zs/lattices"], device="cuda"), torch.tensor(unknown, device="cuda"),
                      torch.tensor(r3["zs/positions"], device="cuda"))
    # training mode: the loss can be taken on the device the batch lives on
    model.train()
    out = model.forward(torch.tensor(cases[0][0], device="cuda"), torch.tensor(cases[0][1], device="cuda"),
                        torch.tensor(cases[0][2], device="cuda"))
    assert out.is_cuda and out.requires_grad
    torch.nn.MSELoss()(out, torch.zeros_like(out)).backward()
    assert all(p.grad is not None for p in model.parameters())


def test_training_gradients_with_per_sample_lattices_and_species():
    """Training-mode ``forward`` takes any ``lattice[S,3,3]`` and ``atomic_numbers[S,N]`` (``_gnn.py:603-611, 541-557``):
    float64 device step against float64 autograd through the oracle (which is pinned to the reference's outputs for these
    very inputs, ``tests/test_oracle_golden.py``), and the float32 product step against the float64 one."""
    from oracle import potgnn_oracle as O
    g, r3 = load_golden("triclinic20"), load_golden("triclinic20_r3")
    model = product_model_from_golden(g)
    oracle = O.model_from_arrays(g).to(torch.float64)
    oracle.coefficient = model.gauss_coefficient  # (the device model keeps the coefficient it was created with)
    lat, zs, pos = r3["zs/lattices"], r3["zs/atomic_numbers"], r3["zs/positions"]
    targets = np.random.default_rng(11).normal(size=(len(pos), 6))
    out64, loss64, grads64 = model.train_gradients_f64(pos, targets, lattice=lat, atomic_numbers=zs)
    o_out, o_loss, o_grads = O.train_gradients(oracle, pos, targets, lattices=lat, atomic_numbers=zs)
    np.testing.assert_allclose(out64, o_out, rtol=0, atol=1e-9 * np.abs(o_out).max())
    assert loss64 == pytest.approx(o_loss, rel=1e-9)
    for name, ref in o_grads.items():
        scale = np.abs(ref).max()
        assert np.abs(grads64[name] - ref).max() < 1e-8 * scale + 1e-12, name
    # ... and they are not the gradients of the reference lattice / species
    plain = model.train_gradients_f64(pos, targets)[2]
    assert max(np.abs(plain[k] - grads64[k]).max() / (np.abs(grads64[k]).max() + 1e-30) for k in grads64) > 1e-3
    model.train()
    out = model.forward(torch.tensor(lat), torch.tensor(zs), torch.tensor(pos))
    torch.nn.MSELoss()(out, torch.tensor(targets, dtype=torch.float32)).backward()
    np.testing.assert_allclose(out.detach().numpy(), out64, rtol=0, atol=2e-5 * np.abs(out64).max())
    worst = 0.0
    for name, p in model.named_parameters():
        scale = np.abs(grads64[name]).max()
        if scale < 1e-12:
            continue
        worst = max(worst, np.abs(p.grad.numpy() - grads64[name]).max() / scale)
    assert worst < 1.5e-4, worst


def test_potgnn_is_a_torch_module():
    """``PotGNN`` is a ``torch.nn.Module`` as the reference's is (``_gnn.py:418-421``): ``model(...)``, forward hooks,
    ``modules()``, ``torch.save(model)`` and ``.to()`` are torch's own -- and wherever the parameters live, the device
    kernels see their current values."""
    import io
    g = load_golden("triclinic20")
    model = product_model_from_golden(g)
    assert isinstance(model, torch.nn.Module)
    kinds = [type(m).__name__ for m in model.modules()]
    assert kinds.count("Linear") == 3 * int(g["hp"][3]) + 5 and "Embedding" in kinds and "BatchNorm1d" in kinds
    s = 4
    lat = torch.tensor(g["lattice"]).expand(s, 3, 3)
    zs = torch.tensor(g["atomic_numbers"]).expand(s, -1)
    pos = torch.tensor(g["pos_batch"][:s])
    model.eval()
    seen = []
    handle = model.register_forward_hook(lambda m, args, out: seen.append(tuple(out.shape)))
    out = model(lat, zs, pos)           # nn.Module.__call__ -> forward
    handle.remove()
    assert seen == [(s, 6)]
    np.testing.assert_allclose(out.numpy(), g["f32/forward"][:s], rtol=0, atol=REL * np.abs(g["f32/forward"]).max())
    # torch.save / torch.load of the whole module
    buffer = io.BytesIO()
    torch.save(model, buffer)
    buffer.seek(0)
    loaded = torch.load(buffer, weights_only=False)
    np.testing.assert_array_equal(loaded.eval()(lat, zs, pos).numpy(), out.numpy())
    # parameters moved to the GPU: evaluation, a training step through torch.optim, evaluation again
    model.to("cuda")
    assert all(p.is_cuda for p in model.parameters())
    np.testing.assert_array_equal(model(lat, zs, pos).numpy(), out.numpy())
    model.train()
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    loss = torch.nn.MSELoss()(model(lat.cuda(), zs.cuda(), pos.cuda()), torch.zeros((s, 6), device="cuda"))
    loss.backward()
    assert all(p.grad is not None and p.grad.is_cuda for p in model.parameters())
    opt.step()
    after = model.eval()(lat, zs, pos).numpy()
    assert np.abs(after - out.numpy()).max() > 0   # the step reached the kernels
    assert model.state_dict()["_node_embedding.0.weight"].is_cuda


@pytest.fixture
def cuda_default_device():
    """The reference's only GPU recipe: ``torch.set_default_device(device)`` around model construction, evaluation and
    training (``test/tests/torch/test_gnn.py:130-160``, ``pmodel/torch/_gnn.py:493-494``, ``_train.py:51-58``)."""
    torch.set_default_device("cuda")
    try:
        yield
    finally:
        torch.set_default_device("cpu")


def test_reference_gpu_recipe_under_cuda_default_device(cuda_default_device):
    """Mirror of the reference's ``test_gpu`` (``test/tests/torch/test_gnn.py:130-160``): construct under a CUDA default
    device, ``eval()``, ``forward`` on default-device tensors for batch sizes 1-3, then ``calc_polarizabilities`` -- and the
    results equal the CPU-default path's bit for bit."""
    g = load_golden("tio2_gnn_test")
    model = product_model_from_golden(g)
    assert all(p.is_cuda for p in model.parameters()), "parameters follow the default device, as the reference's do"
    model.eval()
    rng = np.random.default_rng(12)
    num_atoms = len(g["atomic_numbers"])
    outs = []
    for batch_size in range(1, 4):
        lattice = torch.from_numpy(g["lattice"]).float().to("cuda")
        atomic_numbers = torch.tensor(g["atomic_numbers"])
        batch_lattices = lattice.expand(batch_size, 3, 3)
        batch_atomic_numbers = atomic_numbers.expand(batch_size, num_atoms)
        batch_positions = torch.tensor(rng.standard_normal((batch_size, num_atoms, 3)), dtype=torch.float32)
        assert batch_positions.is_cuda and batch_atomic_numbers.is_cuda
        out = model.forward(batch_lattices, batch_atomic_numbers, batch_positions)
        assert out.is_cuda and tuple(out.shape) == (batch_size, 6) and bool(torch.isfinite(out).all())
        outs.append((batch_positions.cpu(), out.cpu().numpy()))
    pos = g["pos_batch"]
    alpha = model.calc_polarizabilities(pos)
    torch.set_default_device("cpu")
    host = product_model_from_golden(g).eval()
    assert not any(p.is_cuda for p in host.parameters())
    for batch_positions, out in outs:
        s = batch_positions.shape[0]
        want = host.forward(torch.from_numpy(g["lattice"]).float().expand(s, 3, 3),
                            torch.tensor(g["atomic_numbers"]).expand(s, num_atoms), batch_positions).numpy()
        np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(alpha, host.calc_polarizabilities(pos))
    assert _rel_err(alpha, g["f32/alpha"]) < REL


@pytest.mark.parametrize("optimiser", ["torch", "device"])
def test_train_single_epoch_under_cuda_default_device(cuda_default_device, optimiser):
    """``train_single_epoch`` under ``torch.set_default_device("cuda")`` (``_train.py:51-58``: the shuffling generator
    lives on the default device, every batch is moved there).  One mini-batch per epoch holds the whole training set, so
    the CUDA generator's permutation only reorders the batch: losses and weights agree with the CPU-default run.
    ``torch``: plain SGD on ``model.parameters()`` (which live on the GPU under this recipe) -- compared tightly;
    ``device``: ``DeviceAdam`` -- Adam turns rounding-sized gradients of parameters without influence into steps of size lr
    with the rounding's sign, so two runs agree to a few lr only."""
    from ramannoodle_amd.dataset import PolarizabilityDataset
    from ramannoodle_amd.pmodel import DeviceAdam, train_single_epoch
    g = load_golden("triclinic20")
    zs = [int(z) for z in g["atomic_numbers"]]
    rng = np.random.default_rng(8)
    pos = g["positions"][None] + rng.normal(0, 0.01, (12,) + g["positions"].shape)
    alpha = rng.normal(0, 1, (12, 3, 3))
    alpha = alpha + np.swapaxes(alpha, 1, 2)
    lr = 1e-3

    def run():
        train = PolarizabilityDataset(g["lattice"], zs, pos[:8], alpha[:8])
        val = PolarizabilityDataset(g["lattice"], zs, pos[8:], alpha[8:])
        val.scale_polarizabilities(train.mean_polarizability, train.stddev_polarizability)
        model = product_model_from_golden(g, mean=train.mean_polarizability, stddev=train.stddev_polarizability)
        if torch.get_default_device().type == "cuda":
            assert all(p.is_cuda for p in model.parameters())
        opt = DeviceAdam(model, lr=lr) if optimiser == "device" else torch.optim.SGD(model.parameters(), lr=lr)
        results = [train_single_epoch(model, train, val, 8, opt, torch.nn.MSELoss()) for _ in range(3)]
        return results, {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}

    got, got_sd = run()
    torch.set_default_device("cpu")
    want, want_sd = run()
    rel = 1e-5 if optimiser == "torch" else 2e-3
    for a, b in zip(got, want):
        assert np.isfinite(a[0]) and np.isfinite(a[1]) and a[2].shape == (6,)
        assert a[0] == pytest.approx(b[0], rel=rel) and a[1] == pytest.approx(b[1], rel=rel)
        np.testing.assert_allclose(a[2], b[2], rtol=20 * rel, atol=1e-8)
    for k, v in want_sd.items():
        if optimiser == "torch":
            np.testing.assert_allclose(got_sd[k], v, rtol=1e-4, atol=2e-6, err_msg=k)
        else:
            np.testing.assert_allclose(got_sd[k], v, rtol=0, atol=6.5 * lr, err_msg=k)


def test_eight_message_passes_on_the_default_path_against_the_float64_oracle():
    """The default float32 path keeps the edge embedding between passes as split-f16 pair rows (22 significant bits): the
    rounding accumulates per pass, and the fixtures stop at four passes.  Eight passes (``_gnn.py:648-650`` runs the
    blocks ``num_message_passes`` times) on the 64-atom cell at the perf widths against the oracle in float64: the
    standardised polarizability stays within 1e-5 of it, and so does the same evaluation on plain float32 rows."""
    from oracle import potgnn_oracle as O
    g = load_golden("rocksalt64_perf")
    rng = np.random.default_rng(17)
    base = g["pos_batch"]
    pos = base[rng.integers(0, len(base), size=6)] + rng.normal(scale=2e-3, size=(6,) + base.shape[1:])
    model, oracle = _random_model(g, 3.2, 64, 64, 8, seed=88)
    got = model.calc_polarizabilities(pos)
    flags = model.config_flags()
    assert flags["role_split_edge_block"] and flags["atom_owning_node_block"] and flags["split_f16_pair_rows"]
    want = O.calc_polarizabilities(oracle.to(torch.float64), pos, faithful=False)
    std_got, std_want = (got - oracle.mean) / oracle.std, (want - oracle.mean) / oracle.std
    assert _rel_err(std_got, std_want) < REL, _rel_err(std_got, std_want)
    np.testing.assert_array_equal(model.calc_polarizabilities(pos), got)


@pytest.mark.parametrize("case,cutoff,fn,fe,passes,frames", [
    ("rocksalt64_parity", 3.2, 64, 64, 2, 23),   # regular graph: 7-tile ring, windows of two and three tiles, several units
    ("triclinic20", 3.0, 40, 50, 2, 3),          # ragged graph, padded columns
])
def test_gram_instantiation_of_the_role_split_edge_block(monkeypatch, case, cutoff, fn, fe, passes, frames):
    """The opt-in GRAM instantiation of the role-specialised EdgeBlock (``RN_POTGNN_PS_GRAM=1``: the LayerNorm cross terms
    ``p.q`` as a bf16-split Gram block on the matrix pipe, a 7-tile ring, one ``rstd`` per triplet fetched with
    ``ds_bpermute``) computes what the default instantiation computes (``_gnn.py:270-291``): within 1e-5 of the oracle, and
    of the default path, and bit for bit the same twice.  It is not the default because it is slower."""
    from oracle import potgnn_oracle as O
    g = load_golden(case)
    rng = np.random.default_rng(6)
    base = g["pos_batch"]
    pos = base[rng.integers(0, len(base), size=frames)] + rng.normal(scale=2e-3, size=(frames,) + base.shape[1:])
    plain, oracle = _random_model(g, cutoff, fn, fe, passes, seed=fn * 11 + fe)
    ref = plain.calc_polarizabilities(pos)
    monkeypatch.setenv("RN_POTGNN_PS_GRAM", "1")
    model, _ = _random_model(g, cutoff, fn, fe, passes, seed=fn * 11 + fe)
    got = model.calc_polarizabilities(pos)
    assert model.config_flags()["role_split_edge_block"]
    want = O.calc_polarizabilities(oracle, pos, faithful=False)
    assert _rel_err((got - oracle.mean) / oracle.std, (want - oracle.mean) / oracle.std) < REL
    assert _rel_err((got - oracle.mean) / oracle.std, (ref - oracle.mean) / oracle.std) < REL
    assert np.abs(got - ref).max() > 0  # (it really is another instantiation)
    np.testing.assert_array_equal(model.calc_polarizabilities(pos), got)
