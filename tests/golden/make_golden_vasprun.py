"""Golden fixtures for the vasprun.xml reader: the REFERENCE's parser
(``ramannoodle/io/vasp/vasprun.py``: ``read_trajectory``, ``read_positions``, ``read_ref_structure``)
run on its own test files and on generated variants / malformed documents.  Build container only::

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vasprun.py

Writes ``tests/golden/vasprun/*.xml`` (input data: the reference's ``test/data/TiO2/md_run_vasprun.xml``
cut to its first 6 MD frames, ``test/data/STO/vasprun.xml`` as is, generated variants) and
``tests/golden/vasprun/expected.npz`` (what the reference returned: arrays, or the exception type
and message, per function), and ``tests/golden/vasprun/mutants.npz``: the reference's verdict
(``read_trajectory``, ``read_positions``) on a family of damaged documents (every prefix and seeded
one-byte edits of five small documents, plus a structured set; ``tests/ingest_mutants.py``,
``tests/test_ingest_mutants.py``), reproduced bit for bit by every run.  Fixtures are data; no
reference code is copied.
"""
from __future__ import annotations

import os
import re
import shutil
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402

import _standins  # noqa: E402

_standins.install()

from ramannoodle.io.vasp import vasprun as ref  # noqa: E402

OUT = os.path.join(HERE, "vasprun")
os.makedirs(OUT, exist_ok=True)


def small(frames, atoms=("Ti", "O", "O"), potim="  0.50000000", rows=None, extra="", initial=True,
          unnamed_attr="", row_tag="v"):
    """A minimal vasprun-like document (same element layout as VASP writes)."""
    n = len(atoms)
    rng = np.random.default_rng(7)
    doc = ['<?xml version="1.0" encoding="ISO-8859-1"?>', "<modeling>", ' <generator><i name="program">vasp</i></generator>',
           " <incar>", f'  <i name="POTIM">{potim}</i>', " </incar>",
           ' <parameters><separator name="electronic"><i name="POTIM">9.0</i></separator>'
           f'<separator name="ionic" ><i type="int" name="NSW">5</i><i name="POTIM">{potim}</i></separator></parameters>',
           " <atominfo><atoms>%d</atoms><array name=\"atoms\" ><dimension dim=\"1\">ion</dimension>"
           "<field type=\"string\">element</field><field type=\"int\">atomtype</field><set>" % n
           + "".join(f"<rc><c>{a:2s}</c><c>{i + 1:4d}</c></rc>" for i, a in enumerate(atoms))
           + "</set></array></atominfo>"]

    def structure(name, k):
        pos = rows[k] if rows is not None else [" ".join(f"{v:16.8f}" for v in rng.uniform(size=3)) for _ in range(n)]
        body = "".join(f"   <{row_tag}> {r} </{row_tag}>\n" for r in pos)
        return (f' <structure{name}>\n  <crystal>\n   <varray name="basis" >\n    <v> 4.0 0.0 0.0 </v>\n'
                "    <v> 0.1 5.0 0.0 </v>\n    <v> 0.0 0.2 6.0 </v>\n   </varray>\n  </crystal>\n"
                f'  <varray name="positions" >\n{body}  </varray>\n </structure>')

    if initial:
        doc.append(structure(' name="initialpos" ', 0))
    for k in range(frames):
        doc.append(structure(unnamed_attr, k))
    doc.append(extra)
    doc.append(' <structure name="finalpos" ><varray name="positions" ><v> 0 0 0 </v></varray></structure>')
    doc.append("</modeling>")
    return "\n".join(doc) + "\n"


def cut_md(text, frames):
    """Keep the first `frames` un-named <structure> elements (and what lies between them)."""
    starts = [m.start() for m in re.finditer(r"<structure>", text)]
    if len(starts) <= frames:
        return text
    return text[: starts[frames]] + "</modeling>\n"


good = small(4)
ROWS3 = [["0.1 0.2 0.3", "0.25 +0.5 1e-1", ".75 5. -0.125"]] * 2
CASES = {
    "tio2_md": ("file", "/root/reference/test/data/TiO2/md_run_vasprun.xml", 6),
    "sto": ("file", "/root/reference/test/data/STO/vasprun.xml", None),
    # the two inputs of the reference's own exception test (test/tests/test_vasprun.py:154-200):
    # an empty <modeling> root, and a POSCAR handed over as a vasprun.xml
    "ref_malformed": ("file", "/root/reference/test/data/malformed/vasprun.xml", None),
    "ref_poscar_as_xml": ("file", "/root/reference/test/data/TiO2/POSCAR", None),
    "small": good,
    "number_forms": small(2, rows=[["1_0.5 inf -Infinity", "nan 1E2 2e-3", "1 2 3"], ["1 2 3", "4 5 6", "7 8 9"]]),
    "comments_cdata_entities": small(2, rows=[["0.1 <!-- c --> 0.2 0.3", "<![CDATA[0.4 0.5]]> 0.6", "&#48;.7 0.8 0.9"],
                                              ["1 2 3", "4 5 6", "7 8 9"]]),
    "one_frame": small(1),
    "no_frames": small(0),
    "no_initial": small(2, initial=False),
    "named_frames_only": small(2, unnamed_attr=' name="step" '),
    "self_closing_row": small(2, rows=ROWS3).replace("<v> 0.25 +0.5 1e-1 </v>", "<v/>", 1),
    "empty_row_text": small(2, rows=ROWS3).replace("<v> 0.25 +0.5 1e-1 </v>", "<v></v>", 1),
    "bad_token": small(2, rows=[["0.1 0.2 0.3", "0.1 zero 0.3", "1 2 3"], ["1 2 3", "4 5 6", "7 8 9"]]),
    "potim_missing": good.replace('<i name="POTIM">  0.50000000</i></separator></parameters>', "</separator></parameters>"),
    "potim_empty": good.replace('<i name="POTIM">  0.50000000</i></separator></parameters>',
                                '<i name="POTIM"></i></separator></parameters>'),
    "potim_bad": small(2, potim="fast"),
    "structure_without_varray": small(2, extra=" <structure><crystal></crystal></structure>"),
    "no_atominfo": good.replace("<atominfo>", "<atominfox>").replace("</atominfo>", "</atominfox>"),
    "no_lattice": good.replace('<varray name="basis" >', '<varray name="bases" >', 1),
    # ill-formed XML
    "truncated": good[: len(good) // 2],
    "mismatched_tag": good.replace("</incar>", "</incarx>"),
    "junk_after_root": good + "trailing\n",
    "not_xml": "hello\n",
    "empty": "",
    "unclosed_comment": good.replace("<incar>", "<!-- <incar>", 1),
}


def attempt(fn, path):
    try:
        return ("ok", fn(path))
    except Exception as exc:  # pylint: disable=broad-except
        return ("err", type(exc).__name__, str(exc))


expected = {}
for name, spec in CASES.items():
    path = os.path.join(OUT, f"{name}.xml")
    if isinstance(spec, tuple):
        text = open(spec[1], encoding="utf-8").read()
        if spec[2] is not None:
            text = cut_md(text, spec[2])
    else:
        text = spec
    with open(path, "w", encoding="utf-8", newline="") as f:
        f.write(text)
    os.chmod(path, 0o644)

    res = attempt(ref.read_trajectory, path)
    if res[0] == "ok":
        expected[f"{name}/traj/positions"] = res[1].positions_ts
        expected[f"{name}/traj/timestep"] = np.float64(res[1].timestep)
    else:
        expected[f"{name}/traj/error_type"], expected[f"{name}/traj/error_message"] = np.array(res[1]), np.array(res[2])
    res_p = attempt(ref.read_positions, path)
    if res_p[0] == "ok":
        expected[f"{name}/pos/positions"] = np.asarray(res_p[1], dtype=np.float64)
    else:
        expected[f"{name}/pos/error_type"], expected[f"{name}/pos/error_message"] = np.array(res_p[1]), np.array(res_p[2])
    res_s = attempt(ref.read_ref_structure, path)
    if res_s[0] == "ok":
        expected[f"{name}/ref/lattice"] = res_s[1].lattice
        expected[f"{name}/ref/positions"] = res_s[1].positions
        expected[f"{name}/ref/atomic_numbers"] = np.array(res_s[1].atomic_numbers)
    else:
        expected[f"{name}/ref/error_type"], expected[f"{name}/ref/error_message"] = np.array(res_s[1]), np.array(res_s[2])
    print(name, res[:2] if res[0] == "err" else res[1].positions_ts.shape, "|",
          res_p[:3] if res_p[0] == "err" else np.asarray(res_p[1]).shape, "|", res_s[:3] if res_s[0] == "err" else "ref ok")
np.savez_compressed(os.path.join(OUT, "expected.npz"), **expected)


# ----------------------------------------------------------------------------- damaged files (tests/test_ingest_mutants.py)
# The reference's verdict (read_trajectory and read_positions) on every prefix and on seeded one-byte
# edits of a few small documents, plus a structured set that holds each known damage class on
# purpose.  -> vasprun/mutants.npz
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import tempfile  # noqa: E402

from tests import ingest_mutants as M  # noqa: E402

MUTANT_BASES = ["small", "comments_cdata_entities", "number_forms", "self_closing_row", "one_frame"]


def judge(data, scratch):
    with open(scratch, "wb") as f:
        f.write(data)
    out = {}
    res = attempt(ref.read_trajectory, scratch)
    out["traj"] = ("ok", res[1].positions_ts, res[1].timestep) if res[0] == "ok" else res
    res = attempt(ref.read_positions, scratch)
    out["pos"] = ("ok", np.asarray(res[1], dtype=np.float64), None) if res[0] == "ok" else res
    return out


def structured_xml(base):
    """(offset, deleted, inserted) splices of `base` (small.xml), one damage class after the other."""
    out = []

    def at(needle, nth=0, after=False):
        k = -1
        for _ in range(nth + 1):
            k = base.index(needle, k + 1)
        return k + (len(needle) if after else 0)

    row = at(b"0.46793495")              # a number in a row of the first MD frame (character data)
    initial = at(b"0.62509547")          # ... and of the initial structure
    potim = at(b"0.50000000", 1)         # the text of the POTIM element that is read
    attr = at(b'name="POTIM">  0.5', 1) + len(b'name="P')  # inside that element's attribute value, before "OTIM"
    gap = at(b" <structure>")            # between two children of the root
    decl_end = at(b"?>\n", after=True)   # after the XML declaration
    enc = at(b"ISO-8859-1")
    end = len(base)

    # references: the five predefined entities, decimal and hexadecimal character references, well and ill formed
    good_refs = [b"&lt;", b"&gt;", b"&amp;", b"&quot;", b"&apos;", b"&#48;", b"&#x30;", b"&#048;", b"&#x0030;", b"&#x4f;",
                 b"&#79;", b"&#233;", b"&#x20AC;", b"&#9;", b"&#x10FFFF;"]
    bad_refs = [b"&", b"& ", b"&;", b"&lt", b"&amp ", b"&AMP;", b"&foo;", b"&#;", b"&#x;", b"&#X30;", b"&#4;", b"&#0;",
                b"&#x110000;", b"&#xD800;", b"&#xFFFE;", b"&#48", b"&#4 8;", b"&#x3G;", b"&1;", b"&#-48;", b"&lt;;&", b"&&amp;"]
    for ref_ in good_refs + bad_refs:
        out.append((row, 1, ref_))        # in place of the leading 0 of a number
        out.append((attr, 1, ref_))       # in place of the O of name="POTIM"
        out.append((potim, 1, ref_))
    for ref_ in (b"&#48;", b"&amp;", b"&", b"&#4;"):
        out.append((initial, 1, ref_))
        out.append((gap, 0, ref_))        # between elements, inside the root
        out.append((end, 0, ref_))        # after the root
        out.append((decl_end, 0, ref_))   # before the root
    # comments
    for text in (b"<!-- a -- b -->", b"<!-- a --->", b"<!---->", b"<!--->", b"<!-- - -->", b"<!-- <v> & -->", b"<!- a -->",
                 b"<!-- a --", b"<! -- a -->"):
        for where in (row, gap, decl_end, end):
            out.append((where, 0, text))
    # "]]>" in character data, CDATA sections
    for text in (b"]]>", b"]]", b"]>", b"]]&gt;", b"] ]>", b"<![CDATA[]]>", b"<![CDATA[ 0.5 ]]>", b"<![CDATA[<v>&amp;]]>",
                 b"<![CDATA[]]]]>", b"<![CDATA[ ]]", b"<![cdata[ ]]>", b"<![CDATA [ ]]>", b"<![CDATA[ ]]><![CDATA[ ]]>"):
        for where in (row, potim, gap):
            out.append((where, 0, text))
    out.append((decl_end, 0, b"<![CDATA[ ]]>"))
    out.append((end, 0, b"<![CDATA[ ]]>"))
    # attributes
    tag = at(b'<i name="POTIM">  0.5', 1)
    for text in (b'<i name="POTIM" name="POTIM">', b'<i type="x" type="y" name="POTIM">', b'<i name="POTIM" nam="x">',
                 b'<i name="PO<TIM">', b'<i name="PO>TIM">', b'<i name="PO&lt;TIM">', b"<i name='POTIM'>", b"<i name='PO\"TIM'>",
                 b'<i name="POTIM\'>', b"<i name=POTIM>", b'<i name ="POTIM">', b'<i name= "POTIM">', b'<i name\n=\n"POTIM">',
                 b'<i type="x"name="POTIM">', b'<i name="POTIM"type="x">', b'<i name="POTIM" >', b'<i name="POTIM"/>',
                 b'<i name="POTIM" / >', b'<i name=" POTIM">', b'<i name="POTIM\n">', b'<i name="PO\tTIM">', b'<i 0name="POTIM">',
                 b'<i -name="POTIM">', b'<i .name="POTIM">', b'<i _name="POTIM">', b'<i na.me-0="POTIM">', b'<i name>',
                 b'<i name="POTIM" x>', b'<i a:b="1" name="POTIM">', b'<i xml:lang="en" name="POTIM">', b'<i name="POTIM"',
                 b'<i\nname="POTIM"\n>', b'< i name="POTIM">', b'<0i name="POTIM">', b'<i name="">', b'<i name="POTIM" name2="POTIM">'):
        out.append((tag, len(b'<i name="POTIM">'), text))
    out.append((at(b"<v> 4.0", 1), 3, b'<v a="1" a="2">'))
    out.append((at(b"<v> 4.0", 1), 3, b"<a:v>"))
    out.append((at(b"</incar>"), len(b"</incar>"), b"</incar >"))
    out.append((at(b"</incar>"), len(b"</incar>"), b"</ incar>"))
    out.append((at(b"</incar>"), len(b"</incar>"), b'</incar a="1">'))
    # processing instructions
    for text in (b"<?x?>", b"<?x y?>", b"<?x y ?> ?>", b"<? x?>", b"<?0x?>", b"<?x", b"<?x y>", b"<?xml version=\"1.0\"?>",
                 b"<?XML y?>", b"<?xmlx y?>", b"<?x?y?>"):
        for where in (decl_end, row, gap, end):
            out.append((where, 0, text))
    # DOCTYPE
    for text in (b"<!DOCTYPE modeling>", b"<!DOCTYPE modeling SYSTEM \"m.dtd\">", b"<!DOCTYPE modeling [ <!ELEMENT modeling ANY> ]>",
                 b"<!doctype modeling>", b"<!DOCTYPE>", b"<!DOCTYPE modeling", b"<!DOCTYPE modeling><!DOCTYPE modeling>",
                 b"<!ELEMENT modeling ANY>"):
        for where in (decl_end, gap, end):
            out.append((where, 0, text))
    # byte-order mark, what may precede the declaration
    for text in (b"\xef\xbb\xbf", b"\xef\xbb\xbf\xef\xbb\xbf", b"\xef\xbb\xbf ", b" ", b"\n", b"<!-- c -->", b"\xef\xbb"):
        out.append((0, 0, text))
    out.append((0, decl_end, b""))                      # no declaration at all
    out.append((0, decl_end, b"\xef\xbb\xbf"))          # a mark and no declaration
    # the declaration: encoding names, known, unknown and misspelt; its other parts
    for name in (b"ISO-859-1", b"klingon", b"latin1", b"latin-1", b"iso-8859-1", b"ISO-8859-15", b"ISO-8859-12", b"UTF-8", b"utf-8",
                 b"utf8", b"US-ASCII", b"ascii", b"UTF-16", b"utf-16", b"cp1252", b"", b"8859", b"ISO 8859-1", b"ISO-8859-1 "):
        out.append((enc, len(b"ISO-8859-1"), name))
    for text in (b'<?xml version="1.0"?>', b'<?xml version="1.1" encoding="ISO-8859-1"?>', b"<?xml version='1.0' encoding='ISO-8859-1'?>",
                 b'<?xml encoding="ISO-8859-1"?>', b'<?xml encoding="ISO-8859-1" version="1.0"?>', b'<?xml version="1.0" standalone="yes"?>',
                 b'<?xml version="1.0" standalone="maybe"?>', b'<?xml version="1.0" standalone="no" encoding="UTF-8"?>',
                 b'<?xml version="1.0" encoding="UTF-8" standalone="no" ?>', b'<?xml version = "1.0" ?>', b'<?xml version="1.0"encoding="UTF-8"?>',
                 b'<?xml version="1.0" encoding="UTF-8"', b'<?xml?>', b'<?xml ?>', b'<?xml version=1.0?>', b'<?xml version="1.0" x="y"?>',
                 b'<?xml version="">', b'<?xml version=""?>', b'<?XML version="1.0"?>', b'<?xml\nversion="1.0"\n?>'):
        out.append((0, decl_end - 1, text))
    return out


def record_mutants():
    rec = M.Recorder(["traj", "pos"])
    scratch = os.path.join(tempfile.mkdtemp(), "vasprun.xml")
    bases = {}
    for seed, name in enumerate(MUTANT_BASES):
        with open(os.path.join(OUT, f"{name}.xml"), "rb") as f:
            bases[name] = f.read()
        for op, offset, arg in M.family(bases[name], M.XML_ALPHABET, seed + 101):
            data = M.apply(bases[name], op, offset, arg)
            rec.add(rec.base(name), op, offset, arg, data, judge(data, scratch))
    structured = structured_xml(bases["small"])
    for offset, deleted, inserted in structured:
        data = bases["small"][:offset] + inserted + bases["small"][offset + deleted:]
        rec.add(rec.base("small"), M.SPLICE, offset, rec.splice(deleted, inserted), data, judge(data, scratch))
    rec.save(os.path.join(OUT, "mutants.npz"))
    print(f"mutants: {len(rec.rows)} cases ({len(structured)} structured)")
    for kind in rec.kinds:
        counts = rec.counts(kind)
        print(f"mutants: {kind}: {counts}")
        assert min(counts[k] for k in ("returned", "InvalidFileException", "ValueError")) >= 50, "lopsided family: widen it"
    largest = max(os.path.getsize(os.path.join(OUT, n)) for n in os.listdir(OUT) if n != "mutants.npz")
    assert os.path.getsize(os.path.join(OUT, "mutants.npz")) < largest, "mutants.npz must stay below the largest fixture"


record_mutants()
