"""Golden fixtures of the interpolation model, produced by running the REFERENCE implementation (read-only import).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_interp.py

With the identity symmetry of ``_standins`` every ``add_dof`` of the reference's ``InterpolationModel`` adds exactly one
degree of freedom, so a model is built from seeded data alone and its ``calc_polarizabilities``, ``Phonons`` and
``Trajectory`` run unmodified.

* ``interp_p1_small.npz`` -- 7 atoms, a triclinic cell, 19 of the 21 DOFs of a seeded orthonormal basis (the two left
  out leave a rest channel), orders cycling 1, 2, 3 with 2, 4, 6 amplitudes (and the reference point).  40 frames: two
  with a coordinate displaced by exactly +0.5 and -0.5 (dyadic values: the subtraction is exact) and two with an
  amplitude beyond the last knot.
* ``interp_p1_tiles.npz`` -- 23 atoms (3N = 69), 66 DOFs, 35 frames: remainders of every tile of the device kernel.

Each stores the model as data (lattice, reference positions, alpha_ref, basis vectors, every spline's t, c, k), the
frames with the reference's polarizabilities, unmasked and for one masked model, the Raman tensors and ``measure()``
output of the reference's ``Phonons.get_raman_spectrum`` for seeded modes, and the ``measure()`` output of the
reference's ``Trajectory.get_raman_spectrum``.  The script asserts that no amplitude lies within 1e-9 of a breakpoint
and that no wrapped coordinate lies within 1e-6 of 0.5 unless it is exactly 0.5.
"""
from __future__ import annotations

import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402

import _standins  # noqa: E402

_standins.install()

from ramannoodle.dynamics._phonon import Phonons  # noqa: E402
from ramannoodle.dynamics._trajectory import Trajectory  # noqa: E402
from ramannoodle.pmodel._interpolation import InterpolationModel  # noqa: E402
from ramannoodle.structure._reference import ReferenceStructure  # noqa: E402

from ramannoodle_amd.pmodel.interpolation import amplitudes_host, piecewise_tables, wrapped_displacement  # noqa: E402

ORDERS = (1, 2, 3)
AMPLITUDES = {1: (-0.1, 0.1), 2: (-0.2, -0.1, 0.1, 0.2), 3: (-0.3, -0.2, -0.1, 0.1, 0.2, 0.3)}


def symmetric(rng, scale):
    m = rng.normal(size=(3, 3)) * scale
    return (m + m.T) / 2


def build_case(seed: int, atoms: int, dofs: int, frames: int, special: bool, modes: int, masked):
    rng = np.random.default_rng(seed)
    lattice = np.diag([5.5, 6.25, 7.0]) + rng.uniform(-0.6, 0.6, size=(3, 3))
    ref_positions = np.round(rng.uniform(0.1, 0.9, size=(atoms, 3)) * 1024) / 1024  # dyadic
    if special:
        ref_positions[0, 0], ref_positions[1, 1] = 0.25, 0.75
    atomic_numbers = [int(z) for z in rng.choice([8, 22, 38], size=atoms)]
    structure = ReferenceStructure(atomic_numbers, lattice, ref_positions)
    alpha_ref = np.diag([40.0, 41.5, 39.0]) + symmetric(rng, 1.0)
    model = InterpolationModel(structure, alpha_ref)
    basis, _ = np.linalg.qr(rng.normal(size=(3 * atoms, 3 * atoms)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for j in range(dofs):
            order = ORDERS[j % 3]
            amps = np.array(AMPLITUDES[order])
            a1, a2, a3 = symmetric(rng, 4.0), symmetric(rng, 6.0), symmetric(rng, 8.0)
            pols = alpha_ref + amps[:, None, None] * a1 + amps[:, None, None] ** 2 * a2 + amps[:, None, None] ** 3 * a3
            model.add_dof(basis[:, j].reshape(atoms, 3), amps, pols, order)
    assert len(model.cart_basis_vectors) == dofs and len(model.interpolations) == dofs

    positions = ref_positions + rng.normal(size=(frames, atoms, 3)) * 0.012
    inverse = np.linalg.inv(lattice)
    if special:
        # beyond the last knot of DOF 2 (order 3) and below the first knot of DOF 3 (order 1)
        positions[5] += (0.47 * model.cart_basis_vectors[2]) @ inverse
        positions[6] += (-0.41 * model.cart_basis_vectors[3]) @ inverse
        positions[9, 0, 0] = 0.75   # exactly +0.5 from 0.25
        positions[11, 1, 1] = 0.25  # exactly -0.5 from 0.75: wraps to +0.5
    positions = positions - np.floor(positions)  # (as a Trajectory would)

    tables = piecewise_tables(model.interpolations)
    amplitudes = amplitudes_host(lattice, ref_positions, model.cart_basis_vectors, positions)
    for j in range(dofs):
        first, last = tables.piece_offsets[j] + j, tables.piece_offsets[j + 1] + j + 1
        gap = np.abs(amplitudes[:, j, None] - tables.breakpoints[None, first:last]).min()
        assert gap > 1e-9, (j, gap)
    w = wrapped_displacement(positions, ref_positions)
    near = np.abs(np.abs(w) - 0.5) < 1e-6
    assert np.all(np.abs(w[near]) == 0.5), w[near]
    if special:
        assert w[9, 0, 0] == 0.5 and w[11, 1, 1] == 0.5 and near.sum() == 2
        assert amplitudes[5, 2] > 0.3 + 0.1 and amplitudes[6, 3] < -0.1 - 0.1

    out = {
        "lattice": lattice, "ref_positions": ref_positions, "atomic_numbers": np.array(atomic_numbers, dtype=np.int32),
        "alpha_ref": alpha_ref, "basis": np.array(model.cart_basis_vectors), "positions": positions,
        "alpha": model.calc_polarizabilities(positions), "masked": np.array(masked, dtype=np.int32),
        "alpha_masked": model.get_masked_model(list(masked)).calc_polarizabilities(positions),
        "orders": np.array([s.k for s in model.interpolations], dtype=np.int32),
    }
    for j, spline in enumerate(model.interpolations):
        out[f"t{j}"], out[f"c{j}"] = np.asarray(spline.t), np.asarray(spline.c)

    displacements = rng.normal(size=(modes, atoms, 3)) * 0.05
    wavenumbers = np.sort(rng.uniform(80.0, 900.0, size=modes))
    spectrum = Phonons(ref_positions, wavenumbers, displacements).get_raman_spectrum(model)
    out["ph/displacements"], out["ph/wavenumbers"] = displacements, wavenumbers
    out["ph/raman_tensors"] = spectrum.raman_tensors
    out["ph/int_raw"] = spectrum.measure()[1]
    out["ph/int_corr"] = spectrum.measure(laser_correction=True, laser_wavelength=532, bose_einstein_correction=True,
                                          temperature=300)[1]
    timestep = 2.5
    md = Trajectory(positions, timestep).get_raman_spectrum(model)
    out["md/timestep"] = np.float64(timestep)
    out["md/wavenumbers"], out["md/int_raw"] = md.measure()
    return out


def main():
    cases = {
        "interp_p1_small": dict(seed=7101, atoms=7, dofs=19, frames=40, special=True, modes=5, masked=(1, 2, 9)),
        "interp_p1_tiles": dict(seed=7102, atoms=23, dofs=66, frames=35, special=False, modes=4, masked=(0, 64, 65)),
    }
    for name, arguments in cases.items():
        data = build_case(**arguments)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **data)
        print(f"{name}: {os.path.getsize(path)} bytes, max |alpha| {np.abs(data['alpha']).max():.3f}")


if __name__ == "__main__":
    main()
