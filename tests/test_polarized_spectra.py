"""Polarized and oriented Raman spectra on the host: ``measure_polarized`` of the phonon and MD spectra
against their definition, the reference's fixtures, the icosahedral rotation average and the
depolarization ratio; broadcasting and argument checks."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from ramannoodle_amd import _lib
from ramannoodle_amd.spectrum import (MDRamanSpectrum, PhononRamanSpectrum, calc_signal_spectrum,
                                      polarized_weights)
from tests.conftest import load_golden

CORRECTIONS = {"laser_correction": True, "laser_wavelength": 532, "bose_einstein_correction": True,
               "temperature": 300}


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _random_configurations(k, seed):
    """Random vectors (not orthogonal, not unit), random proper rotations."""
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(k, 3)), rng.normal(size=(k, 3)),
            Rotation.random(k, random_state=seed).as_matrix())


def _md_series(steps, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(steps)[:, None, None]
    alpha = rng.normal(size=(steps, 3, 3)) * 0.1 + np.sin(0.05 * t * (1 + np.arange(9).reshape(3, 3)))
    return alpha + np.swapaxes(alpha, 1, 2)


def _md_definition(alpha, timestep, e_i, e_s, rotations):
    """``calc_signal_spectrum(e_s . R da R^T . e_i)`` without the zero bin, one row per configuration."""
    da = np.diff(alpha, axis=0)
    rows = []
    for a, b, r in zip(_unit(e_i), _unit(e_s), rotations):
        signal = np.einsum("a,ab,tbc,dc,d->t", b, r, da, r, a)
        rows.append(calc_signal_spectrum(signal, timestep)[1][1:])
    return np.array(rows)


@pytest.mark.parametrize("steps", [48, 101, 256])
def test_md_matches_definition(steps):
    alpha = load_golden("triclinic20")["md/alpha_ts"] if steps == 48 else _md_series(steps, steps)
    e_i, e_s, rotations = _random_configurations(9, steps)
    spectrum = MDRamanSpectrum(alpha, 1.3)
    w, i = spectrum.measure_polarized(e_i, e_s, rotations)
    np.testing.assert_array_equal(w, spectrum.measure()[0])
    want = _md_definition(alpha, 1.3, e_i, e_s, rotations)
    assert i.shape == want.shape == (9, len(w))
    assert _rel(i, want) < 1e-12


def test_phonon_matches_definition():
    g = load_golden("triclinic20")
    e_i, e_s, rotations = _random_configurations(8, 3)
    spectrum = PhononRamanSpectrum(g["ph/wavenumbers"], g["ph/raman_tensors"])
    w, i = spectrum.measure_polarized(e_i, e_s, rotations)
    np.testing.assert_array_equal(w, g["ph/wavenumbers"])
    want = np.einsum("ka,kab,mbc,kdc,kd->km", _unit(e_s), rotations, g["ph/raman_tensors"], rotations,
                     _unit(e_i)) ** 2
    assert i.shape == (8, 6) and _rel(i, want) < 1e-12


def test_powder_sum_reproduces_reference_fixtures():
    """45 (parallel + perpendicular) under "polycrystalline" is the reference's unpolarized spectrum."""
    g = load_golden("triclinic20")
    e_i, e_s = np.array([[0.0, 0.0, 2.0], [1.0, 1.0, 0.0]]), np.array([[0.0, 0.0, 1.0], [1.0, -1.0, 0.0]])
    md = MDRamanSpectrum(g["md/alpha_ts"], float(g["md/timestep"]))
    ph = PhononRamanSpectrum(g["ph/wavenumbers"], g["ph/raman_tensors"])
    for kwargs, md_key, ph_key in (({}, "md/int_raw", "ph/int_raw"), (CORRECTIONS, "md/int_corr", "ph/int_corr")):
        w, i = md.measure_polarized(e_i, e_s, "polycrystalline", **kwargs)
        np.testing.assert_allclose(w, g["md/wavenumbers"], rtol=1e-14)
        assert _rel(45.0 * i.sum(axis=0), g[md_key]) < 1e-10
        w, i = ph.measure_polarized(e_i, e_s, "polycrystalline", **kwargs)
        assert _rel(45.0 * i.sum(axis=0), g[ph_key]) < 1e-13


@pytest.mark.parametrize("angle", [0.0, 0.4, 1.1, np.pi / 2, 2.5])
def test_icosahedral_average_is_polycrystalline(angle):
    """The 60-rotation icosahedral group averages a degree-4 polynomial in R exactly."""
    group = Rotation.create_group("I").as_matrix()
    e_i = _unit(np.array([0.3, -1.0, 0.7]))
    perp = _unit(np.cross(e_i, [1.0, 0.0, 0.0]))
    e_s = np.cos(angle) * e_i + np.sin(angle) * perp
    g = load_golden("triclinic20")
    for spectrum in (MDRamanSpectrum(g["md/alpha_ts"], 1.0),
                     PhononRamanSpectrum(g["ph/wavenumbers"], g["ph/raman_tensors"])):
        _, oriented = spectrum.measure_polarized(e_i, e_s, group)
        _, powder = spectrum.measure_polarized(e_i, e_s, "polycrystalline")
        assert oriented.shape == (60, powder.size)
        assert _rel(oriented.mean(axis=0), powder) < 1e-12


def test_depolarization_ratio():
    """I_perpendicular / I_parallel: 0 for an isotropic alpha(t), 3/4 for a traceless one."""
    rng = np.random.default_rng(5)
    steps = 200
    isotropic = np.cumsum(rng.normal(size=steps))[:, None, None] * np.eye(3)
    traceless = _md_series(steps, 6)
    traceless -= np.trace(traceless, axis1=1, axis2=2)[:, None, None] * np.eye(3) / 3
    e_i, e_s = [1.0, 0.0, 0.0], [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
    _, (par, perp) = MDRamanSpectrum(isotropic, 1.0).measure_polarized(e_i, e_s, "polycrystalline")
    assert np.abs(perp).max() < 1e-13 * np.abs(par).max()
    _, (par, perp) = MDRamanSpectrum(traceless, 1.0).measure_polarized(e_i, e_s, "polycrystalline")
    strong = np.abs(par) > 1e-6 * np.abs(par).max()
    np.testing.assert_allclose(perp[strong] / par[strong], 0.75, rtol=1e-10)
    tensors = rng.normal(size=(4, 3, 3))
    tensors = tensors + np.swapaxes(tensors, 1, 2)
    tensors -= np.trace(tensors, axis1=1, axis2=2)[:, None, None] * np.eye(3) / 3
    _, (par, perp) = PhononRamanSpectrum(np.arange(1.0, 5.0), tensors).measure_polarized(e_i, e_s, "polycrystalline")
    np.testing.assert_allclose(perp / par, 0.75, rtol=1e-12)


def test_broadcasting_and_squeezing():
    g = load_golden("triclinic20")
    md = MDRamanSpectrum(g["md/alpha_ts"], 1.0)
    ph = PhononRamanSpectrum(g["ph/wavenumbers"], g["ph/raman_tensors"])
    e_i, e_s, rotations = _random_configurations(5, 11)
    w, full = md.measure_polarized(e_i, e_s, rotations)
    bins = len(w)
    assert md.measure_polarized(e_i[0], e_s[0], rotations[0])[1].shape == (bins,)
    assert md.measure_polarized(e_i[0], e_s[0])[1].shape == (bins,)
    assert md.measure_polarized(e_i[:1], e_s[0])[1].shape == (1, bins)
    assert ph.measure_polarized(e_i[0], e_s[0], "polycrystalline")[1].shape == (6,)
    assert ph.measure_polarized(e_i, e_s[0], "polycrystalline")[1].shape == (5, 6)
    # a K axis on one argument broadcasts the others; rows equal the single-configuration results
    _, rows = md.measure_polarized(e_i[2], e_s[2], rotations)
    assert _rel(rows[2], full[2]) < 1e-14
    _, row = md.measure_polarized(e_i[3], e_s[3], rotations[3])
    assert _rel(row, full[3]) < 1e-14
    _, rows = ph.measure_polarized(e_i, e_s[1], None)
    _, row = ph.measure_polarized(e_i[4], e_s[1], np.eye(3))
    assert _rel(rows[4], row) < 1e-14
    # lists, integer arrays and unnormalised vectors are accepted
    _, a = md.measure_polarized([0, 0, 3], [[0, 2, 0]])
    _, b = md.measure_polarized(np.array([0.0, 0.0, 1.0]), np.array([[0.0, 1.0, 0.0]]))
    np.testing.assert_array_equal(a, b)
    # corrections apply per row
    _, raw = ph.measure_polarized(e_i, e_s, rotations)
    _, corr = ph.measure_polarized(e_i, e_s, rotations, **CORRECTIONS)
    factor = ph.measure(**CORRECTIONS)[1] / ph.measure()[1]
    np.testing.assert_allclose(corr, raw * factor, rtol=1e-14)


def test_weights_packing():
    """21 packed pairs: the powder weights of measure() (45 a^2 + 7 gamma^2) in the documented order."""
    weights, squeeze = polarized_weights([[1, 0, 0], [1, 0, 0]], [[1, 0, 0], [0, 1, 0]], "polycrystalline")
    assert weights.shape == (2, 21) and weights.flags.c_contiguous and not squeeze
    powder = 45.0 * weights.sum(axis=0)
    pairs = [(j, l) for j in range(6) for l in range(j, 6)]
    want = {(0, 0): 12, (1, 1): 12, (2, 2): 12, (3, 3): 21, (4, 4): 21, (5, 5): 21,
            (0, 1): 3, (0, 2): 3, (1, 2): 3}
    np.testing.assert_allclose(powder, [want.get(p, 0) for p in pairs], atol=1e-13)
    weights, squeeze = polarized_weights([0, 0, 1], [0, 1, 0])
    assert squeeze and np.count_nonzero(weights) == 1 and weights[0, pairs.index((4, 4))] == 1.0


def test_validation_errors():
    g = load_golden("triclinic20")
    md = MDRamanSpectrum(g["md/alpha_ts"], 1.0)
    ph = PhononRamanSpectrum(g["ph/wavenumbers"], g["ph/raman_tensors"])
    x, y = np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
    rotation = Rotation.from_euler("xyz", [0.1, 0.2, 0.3]).as_matrix()
    for spectrum in (md, ph):
        with pytest.raises(ValueError, match="number of configurations"):
            spectrum.measure_polarized(np.tile(x, (3, 1)), np.tile(y, (2, 1)))
        with pytest.raises(ValueError, match="number of configurations"):
            spectrum.measure_polarized(np.tile(x, (3, 1)), y, np.tile(rotation, (4, 1, 1)))
        with pytest.raises(ValueError, match="zero vector"):
            spectrum.measure_polarized(np.zeros(3), y)
        with pytest.raises(ValueError, match="zero vector"):
            spectrum.measure_polarized(x, np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 0.0]]))
        with pytest.raises(ValueError, match="not finite"):
            spectrum.measure_polarized(np.array([np.nan, 0.0, 1.0]), y)
        with pytest.raises(ValueError, match="not finite"):
            spectrum.measure_polarized(x, np.array([np.inf, 0.0, 1.0]))
        with pytest.raises(ValueError, match="not finite"):
            spectrum.measure_polarized(x, y, np.full((3, 3), np.nan))
        with pytest.raises(ValueError, match="wrong shape"):
            spectrum.measure_polarized(np.ones(4), y)
        with pytest.raises(ValueError, match="wrong shape"):
            spectrum.measure_polarized(x, np.ones((2, 2, 3)))
        with pytest.raises(ValueError, match="wrong shape"):
            spectrum.measure_polarized(x, y, np.eye(4))
        with pytest.raises(ValueError, match="proper rotation"):
            spectrum.measure_polarized(x, y, -rotation)  # det -1
        with pytest.raises(ValueError, match="proper rotation"):
            spectrum.measure_polarized(x, y, 1.001 * rotation)
        with pytest.raises(ValueError, match="proper rotation"):
            spectrum.measure_polarized(x, y, np.stack([rotation, np.diag([1.0, 1.0, -1.0])]))
        with pytest.raises(ValueError, match="unknown orientation"):
            spectrum.measure_polarized(x, y, "single crystal")
        with pytest.raises(TypeError, match="incident should have type"):
            spectrum.measure_polarized("x", y)
        with pytest.raises(TypeError, match="scattered should have type"):
            spectrum.measure_polarized(x, None)
        with pytest.raises(TypeError, match="scattered should have type"):
            spectrum.measure_polarized(x, np.array([1j, 0, 0]))
        with pytest.raises(TypeError, match="orientation should have type"):
            spectrum.measure_polarized(x, y, {"R": rotation})
        with pytest.raises(TypeError, match="orientation should have type"):
            spectrum.measure_polarized(x, y, np.eye(3, dtype=bool))
    # rotations within the documented tolerance pass
    md.measure_polarized(x, y, rotation + 1e-10)
    # measure() and its orientation refusal are unchanged
    with pytest.raises(NotImplementedError):
        md.measure(orientation=np.eye(3))


def test_c_abi_declares_the_polarized_entries():
    assert "rn_md_raman_polarized" in _lib.SIGNATURES and "rn_md_raman_polarized_device" in _lib.SIGNATURES
