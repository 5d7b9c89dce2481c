"""Golden fixtures for the trajectory reader: the REFERENCE's XDATCAR parser
(``ramannoodle/io/vasp/xdatcar.py::read_positions_ts``) run on its own test file and on
hand-made variants / malformed inputs.  Build container only (``/root/reference`` mounted)::

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_io.py

Writes ``tests/golden/xdatcar/*.XDATCAR`` (input data: the reference's ``test/data/STO/XDATCAR``
and generated variants) and ``tests/golden/xdatcar/expected.npz`` (what the reference returned:
positions, or the exception type and message), and ``tests/golden/xdatcar/mutants.npz``: the
reference's verdict on a family of damaged files (every prefix and seeded one-byte edits of five
small files, plus a structured set; ``tests/ingest_mutants.py``, ``tests/test_ingest_mutants.py``),
reproduced bit for bit by every run.  Fixtures are data; no reference code is copied.
"""
from __future__ import annotations

import os
import shutil
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402

import _standins  # noqa: E402

_standins.install()

from ramannoodle.io.vasp.xdatcar import read_positions_ts  # noqa: E402

OUT = os.path.join(HERE, "xdatcar")
os.makedirs(OUT, exist_ok=True)

HEADER = "generated\n   1.5\n  4.0 0.0 0.0\n  0.1 5.0 0.0\n  0.0 0.2 6.0\n  Ti O\n  1 2\n"
ROWS = ["  0.1 0.2 0.3\n", " 0.25  +0.5 1e-1  T T F\n", "\t.75 5.  -0.125\n"]


def frame(label, rows=ROWS):
    return label + "".join(rows)


CASES = {
    "sto": None,  # the reference's own test file
    "variants": HEADER + frame("Direct configuration=     1\n") + frame("direct\n") +
                frame("Cartesian configuration= 3\n", ["  0.4 0.5 0.6\n", " 1.0 2.0 3.0\n", "0 0 0\n"]) +
                frame("Selective dynamics\nDirect\n") + frame("D\r\n", [r.replace("\n", "\r\n") for r in ROWS]),
    "ends_on_blank_label": HEADER + frame("Direct\n") + "\n" + frame("Direct\n"),
    "ends_on_indented_label": HEADER + frame("Direct\n") + frame(" Direct\n"),
    "no_trailing_newline": HEADER + frame("Direct\n") + "Direct\n" + "".join(ROWS)[:-1],
    "underscores_inf": HEADER + frame("Direct\n", ["1_0.5 inf -Infinity\n", "nan 1E2 2e-3\n", "1 2 3\n"]),
    "no_frames": HEADER,
    "negative_count": HEADER.replace("  1 2\n", "  -1 3\n") + frame("Direct\n"),
    # malformed
    "bad_scale": HEADER.replace("   1.5\n", "   1.5 2\n") + frame("Direct\n"),
    "bad_lattice_token": HEADER.replace("0.1 5.0 0.0", "0.1 five 0.0") + frame("Direct\n"),
    "short_lattice": HEADER.replace("  0.0 0.2 6.0\n", "  0.0 0.2\n") + frame("Direct\n"),
    "no_symbols": HEADER.replace("  Ti O\n", "\n") + frame("Direct\n"),
    "bad_symbol": HEADER.replace("Ti O", "Ti Xx") + frame("Direct\n"),
    "count_mismatch": HEADER.replace("  1 2\n", "  1 2 3\n") + frame("Direct\n"),
    "bad_count": HEADER.replace("  1 2\n", "  1 two\n") + frame("Direct\n"),
    "bad_label": HEADER + frame("Direct\n") + frame("Fractional\n"),
    "bad_row_token": HEADER + frame("Direct\n", ["0.1 0.2 0.3\n", "0.1 0.2 zero\n", "1 2 3\n"]),
    "short_row": HEADER + frame("Direct\n", ["0.1 0.2 0.3\n", "0.1 0.2\n", "1 2 3\n"]),
    "truncated_frame": HEADER + frame("Direct\n") + frame("Direct\n", ROWS[:2]),
    "underscore_misuse": HEADER + frame("Direct\n", ["_1 0.2 0.3\n", "0.1 0.2 0.3\n", "1 2 3\n"]),
}

expected = {}
for name, text in CASES.items():
    path = os.path.join(OUT, f"{name}.XDATCAR")
    if text is None:
        shutil.copyfile("/root/reference/test/data/STO/XDATCAR", path)
    else:
        with open(path, "w", encoding="utf-8", newline="") as f:
            f.write(text)
    os.chmod(path, 0o644)
    try:
        result = read_positions_ts(path)
        expected[f"{name}/positions"] = np.asarray(result, dtype=np.float64)
        print(f"{name}: positions {np.asarray(result).shape}")
    except Exception as exc:  # pylint: disable=broad-except
        expected[f"{name}/error_type"] = np.array(type(exc).__name__)
        expected[f"{name}/error_message"] = np.array(str(exc))
        print(f"{name}: {type(exc).__name__}: {exc!r}")
np.savez(os.path.join(OUT, "expected.npz"), **expected)


# ----------------------------------------------------------------------------- damaged files (tests/test_ingest_mutants.py)
# The reference's verdict on every prefix and on seeded one-byte edits of a few small files, plus a
# structured set that holds each known damage class on purpose.  -> xdatcar/mutants.npz
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import tempfile  # noqa: E402

from tests import ingest_mutants as M  # noqa: E402

# A variable-cell layout (the header before every configuration) whose repeated comment line starts
# with a blank, as VASP writes it for an unnamed system: there the reference and the package both
# stop reading (the end-of-trajectory signal comes before the header is tried).  A repeated header
# with any other comment is the package's one addition to the reference, which refuses every such
# file; those cases are counted and left out by the test, and only a few may be.
REPEATED = " unnamed system\n   1.5\n  4.0 0.0 0.0\n  0.1 5.0 0.0\n  0.0 0.2 6.0\n  Ti O\n  1 2\n"
VARIABLE_CELL = REPEATED + frame("Direct configuration=     1\n") + REPEATED.replace("4.0", "4.1") + \
    frame("Direct configuration=     2\n") + REPEATED.replace("4.0", "4.2") + frame("Cartesian configuration= 3\n")
with open(os.path.join(OUT, "repeated_header.XDATCAR"), "w", encoding="utf-8", newline="") as f:
    f.write(VARIABLE_CELL)
os.chmod(os.path.join(OUT, "repeated_header.XDATCAR"), 0o644)

MUTANT_BASES = ["variants", "no_trailing_newline", "underscores_inf", "ends_on_blank_label", "repeated_header"]


def judge(data, scratch):
    with open(scratch, "wb") as f:
        f.write(data)
    try:
        return {"read": ("ok", np.asarray(read_positions_ts(scratch), dtype=np.float64), None)}
    except Exception as exc:  # pylint: disable=broad-except
        return {"read": ("err", type(exc).__name__, str(exc))}


def structured_xdatcar(base):
    """(offset, deleted, inserted) splices of `base` (variants.XDATCAR): line endings, labels, selective dynamics."""
    out = []
    ends = [k for k, c in enumerate(base) if c == 0x0A]
    starts = [0] + [k + 1 for k in ends]
    for k in ends:  # a lone \r or \r\n in place of every \n: header lines, labels and rows
        out.append((k, 1, b"\r"))
        if base[k - 1] != 0x0D:
            out.append((k, 1, b"\r\n"))
    for old, new in ((b"\n", b"\r"), (b"\n", b"\r\n"), (b"\r\n", b"\n")):  # the whole file in one convention
        out.append((0, len(base), base.replace(b"\r\n", b"\n").replace(old, new) if old != b"\r\n" else base.replace(old, new)))
    mixed = base.replace(b"\r\n", b"\n").split(b"\n")
    out.append((0, len(base), b"".join(line + (b"\n", b"\r", b"\r\n")[k % 3] for k, line in enumerate(mixed[:-1]))))
    out.append((0, len(base), b"".join(line + (b"\r", b"\r\n")[k % 2] for k, line in enumerate(mixed[:-1]))[:-1]))
    for s in starts[1:12]:  # a \r inside a line: after the first token of header lines and of the first frame's rows
        line = base[s:base.index(b"\n", s)]
        body = line.lstrip()
        cut = s + (len(line) - len(body)) + len(body.split()[0]) if body.split() else s
        out.append((cut, 0, b"\r"))
        out.append((s, 0, b"\r"))
    labels = [s for s in starts[7:] if s < len(base) and base[s:s + 1].lower() in (b"d", b"c", b"s")]
    for s in labels:
        for blanks in (b" ", b"   ", b"\t", b"\r", b"\x1c"):  # a label with leading blanks ends the trajectory
            out.append((s, 0, blanks))
        for line in (b"Selective dynamics\n", b"s\n", b"S\r", b"Selective\r\n", b"Selective dynamics\nSelective dynamics\n",
                     b"Selective\n\n", b"Selective\n \n", b"selective\nFractional\n"):
            out.append((s, 0, line))
    out.append((len(base), 0, b"Selective dynamics"))  # the file ends after the selective-dynamics line
    out.append((len(base), 0, b"Selective dynamics\n"))
    out.append((len(base), 0, b"S"))
    # a header repeated where a label is expected (variable cell): the deliberate difference, left out by the test
    header = base[:starts[7]]
    out.append((len(base), 0, header + b"Direct\n" + b"".join(r.encode() for r in ROWS)))
    out.append((starts[7], 0, header))
    out.append((len(base), 0, header.replace(b"generated", b"Direct run") + b"Cartesian\n" + b"".join(r.encode() for r in ROWS)))
    # no atoms at all: the reference returns (S, 0) for direct frames, and its conversion of a Cartesian
    # frame fails inside numpy with a ValueError that it lets through
    for counts in (b"0 0", b"-1 0", b"0 -3", b"-0 +0", b"0_0 0", b"00 0", b" 0\t0 ", b"+0 -0"):
        for tail in (b"Cartesian\n", b"Direct\nCartesian\n", b"Selective\nCartesian\n", b"Direct\nDirect\nc\n", b"cart",
                     b"C\r", b"D\nC\r\nD\n", b"Direct\nFractional\n", b"Direct\nDirect", b"Direct\n\nCartesian\n"):
            out.append((starts[6], len(base) - starts[6], counts + b"\n" + tail))
    return out


def record_mutants():
    rec = M.Recorder(["read"])
    scratch = os.path.join(tempfile.mkdtemp(), "XDATCAR")
    bases = {}
    for seed, name in enumerate(MUTANT_BASES):
        with open(os.path.join(OUT, f"{name}.XDATCAR"), "rb") as f:
            bases[name] = f.read()
        for op, offset, arg in M.family(bases[name], M.XDATCAR_ALPHABET, seed + 1):
            data = M.apply(bases[name], op, offset, arg)
            rec.add(rec.base(name), op, offset, arg, data, judge(data, scratch))
    structured = structured_xdatcar(bases["variants"])
    for offset, deleted, inserted in structured:
        data = bases["variants"][:offset] + inserted + bases["variants"][offset + deleted:]
        rec.add(rec.base("variants"), M.SPLICE, offset, rec.splice(deleted, inserted), data, judge(data, scratch))
    rec.save(os.path.join(OUT, "mutants.npz"))
    counts = rec.counts("read")
    print(f"mutants: {len(rec.rows)} cases ({len(structured)} structured): {counts}")
    left_out = 0
    for b, op, offset, arg in rec.rows:
        left_out += M.has_repeated_header(M.apply(bases[rec.base_names[b]], op, offset, arg, rec.splices))
    print(f"mutants: {left_out} cases hold a repeated header (left out by the test); the cap is {len(rec.rows) // 100}")
    assert left_out <= len(rec.rows) // 100, "too many variable-cell cases: the test's cap is 1 %"
    assert min(counts[k] for k in ("returned", "InvalidFileException", "ValueError")) >= 50, "lopsided family: widen it"
    largest = max(os.path.getsize(os.path.join(OUT, n)) for n in os.listdir(OUT) if n != "mutants.npz")
    assert os.path.getsize(os.path.join(OUT, "mutants.npz")) < largest, "mutants.npz must stay below the largest fixture"


record_mutants()
