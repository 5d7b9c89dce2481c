"""Writes ``npt.XDATCAR`` and ``expected.npz`` next to itself: a variable-cell trajectory as VASP writes it under
ISIF=3 (the header before every configuration), small enough to read by eye.

3 atoms (Ti O O), 5 configurations, scale factor 1.5; configuration 3 is ``Cartesian`` and configuration 4 sits under a
``Selective dynamics`` line.  The cell breathes and shears by about a percent, the atoms move by a few hundredths of
an Angstrom.  ``expected.npz`` holds what was drawn, before printing: ``lattices`` (5,3,3) in Angstrom with the scale
applied, ``positions`` (5,3,3) fractional, ``scale`` and ``decimals``; numbers are printed with ``decimals`` places, so a
reader agrees with the arrays to that precision.  The Cartesian rows are ``positions @ lattice`` as the reader undoes
them (``positions @ inv(lattice)`` with the scaled lattice, the reference's convention for Cartesian frames).

Run from anywhere: ``python tests/golden/xdatcar_cells/make_npt_fixture.py``."""
import os

import numpy as np

SCALE, DECIMALS, FRAMES = 1.5, 8, 5
HERE = os.path.dirname(os.path.abspath(__file__))


def main() -> None:
    rng = np.random.default_rng(2024)
    lattice0 = np.array([[6.0, 0.0, 0.0], [0.15, 7.5, 0.0], [0.0, 0.3, 9.0]])
    positions0 = np.array([[0.10, 0.20, 0.30], [0.25, 0.50, 0.10], [0.75, 0.05, 0.875]])
    lattices = np.stack([lattice0 @ (np.eye(3) + 0.01 * rng.normal(size=(3, 3))) for _ in range(FRAMES)])
    positions = positions0[None] + 0.004 * rng.normal(size=(FRAMES, 3, 3))
    fmt = f"%.{DECIMALS}f"

    def row(values, tail=""):
        return "  " + "  ".join(fmt % v for v in values) + tail + "\n"

    lines = []
    for k in range(FRAMES):
        lines += ["breathing cell\n", f"   {SCALE}\n"]
        lines += [row(vector / SCALE) for vector in lattices[k]]
        lines += ["  Ti O\n", "  1 2\n"]
        if k == 3:
            lines.append("Selective dynamics\n")
        if k == 2:
            lines.append(f"Cartesian configuration= {k + 1}\n")
            lines += [row(x) for x in positions[k] @ lattices[k]]
        else:
            lines.append(f"Direct configuration= {k + 1}\n")
            lines += [row(x, "  T T F" if k == 3 else "") for x in positions[k]]
    with open(os.path.join(HERE, "npt.XDATCAR"), "w", encoding="ascii") as file:
        file.writelines(lines)
    np.savez(os.path.join(HERE, "expected.npz"), lattices=lattices, positions=positions, scale=SCALE, decimals=DECIMALS)


if __name__ == "__main__":
    main()
