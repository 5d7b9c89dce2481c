"""Damaged trajectory files for the ingest readers, shared by the fixture makers
(``tests/golden/make_golden_io.py``, ``make_golden_vasprun.py``) and ``tests/test_ingest_mutants.py``.

A case is a base file plus a tuple ``(operation, offset, argument)``: cut the file at ``offset``,
replace / delete / insert one byte there, or splice (delete ``n`` bytes and insert a string; the
structured cases the makers build on purpose).  The makers draw the tuples once, from the small
generator below, and store them beside the reference's verdict in ``mutants.npz``; the test only
replays what is stored, so no random-number library can move the family.
"""
from __future__ import annotations

import hashlib
import io
import re
import zipfile

import numpy as np

CUT, REPLACE, DELETE, INSERT, SPLICE = range(5)
OP_NAMES = ("cut", "replace", "delete", "insert", "splice")

XML_ALPHABET = b"<>&;/\"'= \n!-[]?x0"
XDATCAR_ALPHABET = b" \n\t\r0.-+eEdDcCsSx_1"
EDITS_PER_BASE = 1200

# verdict codes
RETURNED, INVALID_FILE, VALUE_ERROR, OTHER = range(4)
VERDICT_NAMES = ("returned", "InvalidFileException", "ValueError", "other")


def apply(base: bytes, op: int, offset: int, arg: int, splices=None) -> bytes:
    """The bytes of one case.  ``splices[arg] = (deleted_length, inserted_bytes)`` for SPLICE."""
    if op == CUT:
        return base[:offset]
    if op == REPLACE:
        return base[:offset] + bytes([arg]) + base[offset + 1:]
    if op == DELETE:
        return base[:offset] + base[offset + 1:]
    if op == INSERT:
        return base[:offset] + bytes([arg]) + base[offset:]
    if op == SPLICE:
        deleted, inserted = splices[arg]
        return base[:offset] + inserted + base[offset + deleted:]
    raise ValueError(f"unknown operation {op}")


class Lcg:
    """Knuth's 64-bit linear congruential generator (upper 32 bits): the same numbers everywhere."""

    def __init__(self, seed: int) -> None:
        self.state = (seed * 2 + 1) & 0xFFFFFFFFFFFFFFFF

    def below(self, n: int) -> int:
        self.state = (self.state * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return (self.state >> 32) % n


def family(base: bytes, alphabet: bytes, seed: int) -> list[tuple[int, int, int]]:
    """Every prefix of ``base`` (the whole file included), then EDITS_PER_BASE seeded one-byte edits."""
    cases = [(CUT, k, 0) for k in range(len(base) + 1)]
    rng = Lcg(seed)
    edits = []
    for _ in range(EDITS_PER_BASE):
        op = (REPLACE, DELETE, INSERT)[rng.below(3)]
        offset = rng.below(len(base) + 1 if op == INSERT else len(base))
        edits.append((op, offset, alphabet[rng.below(len(alphabet))]))
    # (in the order of their offsets: neighbours share verdicts, which keeps the recorded fixture small)
    return cases + sorted(edits, key=lambda e: (e[1], e[0], e[2]))


def python_lines(data: bytes) -> list[str]:
    """The lines ``readline`` gives for a file opened in text mode (universal newlines)."""
    return io.TextIOWrapper(io.BytesIO(data), encoding="latin-1", newline=None).readlines()


def digest(array) -> int:
    """First 8 bytes of the SHA-256 of the array's float64 bytes (C order), as an unsigned integer."""
    data = np.ascontiguousarray(np.asarray(array, dtype=np.float64)).tobytes()
    return int.from_bytes(hashlib.sha256(data).digest()[:8], "little")


def shape3(array) -> tuple[int, int, int]:
    """The shape padded with -1 to three entries (``np.array([])`` has one)."""
    shape = tuple(np.asarray(array).shape)[:3]
    return shape + (-1,) * (3 - len(shape))


def context(data: bytes, op: int, offset: int, width: int = 24) -> str:
    """The bytes around an edit, for failure reports."""
    lo = max(0, offset - width)
    return repr(data[lo:offset + width])


# ----------------------------------------------------------------------------- fixture files
def save_npz(path: str, arrays: dict) -> None:
    """``np.savez_compressed`` with fixed member dates and order, so that a maker run reproduces the file bit for bit."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as archive:
        for name in sorted(arrays):
            buffer = io.BytesIO()
            np.lib.format.write_array(buffer, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            archive.writestr(info, buffer.getvalue(), compresslevel=9)


def pack_strings(strings) -> dict:
    """A list of byte strings as one blob plus end offsets (npz members hold no Python objects)."""
    blob = b"".join(strings)
    ends = np.cumsum([len(s) for s in strings], dtype=np.int64) if strings else np.zeros(0, np.int64)
    return {"blob": np.frombuffer(blob, dtype=np.uint8), "ends": ends}


def unpack_strings(blob, ends) -> list[bytes]:
    data, out, start = bytes(bytearray(blob)), [], 0
    for end in ends:
        out.append(data[start:int(end)])
        start = int(end)
    return out


def _quoted_line(message: str, lines: list[str]):
    """``(text before the quoted line, line number)`` when the message ends in one of the file's
    lines as ``readline`` gives it (most of the XDATCAR parser's messages do), else None."""
    cut = message.find(": ")
    if cut < 0:
        return None
    head, tail = message[:cut + 2], message[cut + 2:]
    for k, line in enumerate(lines):
        if line == tail:
            return head, k
    return (head, len(lines)) if tail == "" else None  # readline at the end of the file: ''


class Recorder:
    """Collects cases and verdicts of one format and writes ``mutants.npz``.  ``kinds`` names the
    readers judged per case (XDATCAR: one; vasprun: ``traj`` and ``pos``).

    Kept small: offsets as differences, returned results as an index into a table of distinct
    (shape, digest, time step), a message that quotes a line of the file as (text, line number)."""

    def __init__(self, kinds) -> None:
        self.kinds = tuple(kinds)
        self.base_names: list[str] = []
        self.splices: list[tuple[int, bytes]] = []
        self.messages: list[str] = [""]
        self.type_names: list[str] = []
        self.results: list[tuple] = []
        self.rows: list[tuple] = []
        self.verdicts = {kind: [] for kind in self.kinds}

    def base(self, name: str) -> int:
        if name not in self.base_names:
            self.base_names.append(name)
        return self.base_names.index(name)

    def splice(self, deleted: int, inserted: bytes) -> int:
        self.splices.append((deleted, inserted))
        return len(self.splices) - 1

    @staticmethod
    def _index(table: list, value) -> int:
        if value not in table:
            table.append(value)
        return table.index(value)

    def add(self, base: int, op: int, offset: int, arg: int, data: bytes, outcomes: dict) -> None:
        """``outcomes[kind]`` = ("ok", array, timestep or None) or ("err", type name, message); ``data``: the case's bytes."""
        self.rows.append((base, op, offset, arg))
        lines = None
        for kind in self.kinds:
            res = outcomes[kind]
            if res[0] == "ok":
                step = -1.0 if res[2] is None else float(res[2])
                result = shape3(res[1]) + (digest(res[1]), step)
                self.verdicts[kind].append((RETURNED, self._index(self.results, result), -1))
                continue
            code = {"InvalidFileException": INVALID_FILE, "ValueError": VALUE_ERROR}.get(res[1], OTHER)
            lines = python_lines(data) if lines is None else lines
            quoted = _quoted_line(res[2], lines)
            text, line = quoted if quoted else (res[2], -1)
            if code == OTHER:  # another exception type: OTHER + its index in type_names
                code = OTHER + self._index(self.type_names, res[1])
            self.verdicts[kind].append((code, self._index(self.messages, text), line))

    def counts(self, kind: str) -> dict:
        out = {name: 0 for name in VERDICT_NAMES}
        for row in self.verdicts[kind]:
            out[VERDICT_NAMES[min(row[0], OTHER)]] += 1
        return out

    def save(self, path: str) -> None:
        rows = np.array(self.rows, dtype=np.int64).reshape(-1, 4)
        arrays = {
            "base_names": np.array(self.base_names),
            "base": rows[:, 0].astype(np.uint8), "op": rows[:, 1].astype(np.uint8),
            "offset_step": np.diff(rows[:, 2], prepend=0).astype(np.int32), "arg": rows[:, 3].astype(np.uint16),
            "splice_deleted": np.array([s[0] for s in self.splices], dtype=np.int32),
            "type_names": np.array(self.type_names),
            "result_shape": np.array([r[:3] for r in self.results], dtype=np.int32).reshape(-1, 3),
            "result_digest": np.array([r[3] for r in self.results], dtype=np.uint64),
            "result_timestep": np.array([r[4] for r in self.results], dtype=np.float64),
        }
        packed = pack_strings([s[1] for s in self.splices])
        arrays["splice_blob"], arrays["splice_ends"] = packed["blob"], packed["ends"].astype(np.int32)
        packed = pack_strings([m.encode("utf-8") for m in self.messages])
        arrays["message_blob"], arrays["message_ends"] = packed["blob"], packed["ends"].astype(np.int32)
        for kind in self.kinds:
            v = np.array(self.verdicts[kind], dtype=np.int64).reshape(-1, 3)
            arrays[f"{kind}_verdict"] = v[:, 0].astype(np.uint8)
            arrays[f"{kind}_index"] = v[:, 1].astype(np.uint16)  # RETURNED: into result_*, else into the messages
            arrays[f"{kind}_line"] = v[:, 2].astype(np.int16)
        save_npz(path, arrays)


class Family:
    """A loaded ``mutants.npz``: ``bytes_of(i)`` rebuilds case ``i``, ``expected(kind, i, data)`` is the record."""

    def __init__(self, path: str, base_dir: str, suffix: str) -> None:
        z = np.load(path)
        self.z = {name: z[name] for name in z.files}
        self.base_names = [str(n) for n in z["base_names"]]
        self.bases = []
        for name in self.base_names:
            with open(f"{base_dir}/{name}{suffix}", "rb") as f:
                self.bases.append(f.read())
        inserted = unpack_strings(z["splice_blob"], z["splice_ends"])
        self.splices = list(zip((int(d) for d in z["splice_deleted"]), inserted))
        self.messages = [m.decode("utf-8") for m in unpack_strings(z["message_blob"], z["message_ends"])]
        self.type_names = [str(n) for n in z["type_names"]]
        self.base, self.op, self.arg = z["base"], z["op"], z["arg"]
        self.offset = np.cumsum(z["offset_step"].astype(np.int64))

    def __len__(self) -> int:
        return len(self.op)

    def bytes_of(self, i: int) -> bytes:
        return apply(self.bases[self.base[i]], int(self.op[i]), int(self.offset[i]), int(self.arg[i]), self.splices)

    def expected(self, kind: str, i: int, data: bytes) -> tuple:
        """(RETURNED, shape, digest, time step or None) or (verdict code, exception type name, message)."""
        z = self.z
        verdict, index = int(z[f"{kind}_verdict"][i]), int(z[f"{kind}_index"][i])
        if verdict == RETURNED:
            shape = tuple(int(n) for n in z["result_shape"][index] if n >= 0)
            step = float(z["result_timestep"][index])
            return RETURNED, shape, int(z["result_digest"][index]), (None if step < 0 else step)
        message, line = self.messages[index], int(z[f"{kind}_line"][i])
        if line >= 0:
            lines = python_lines(data)
            message += lines[line] if line < len(lines) else ""
        name = VERDICT_NAMES[verdict] if verdict < OTHER else self.type_names[verdict - OTHER]
        return min(verdict, OTHER), name, message

    def describe(self, i: int) -> str:
        arg = self.splices[self.arg[i]] if self.op[i] == SPLICE else bytes([int(self.arg[i]) & 0xFF])
        return f"{self.base_names[self.base[i]]} {OP_NAMES[self.op[i]]}@{int(self.offset[i])} {arg!r}"


# ----------------------------------------------------------------------------- the variable-cell predicate
_SYMBOLS = frozenset(
    "H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br "
    "Kr Rb Sr Y Zr Nb Mo Tc Ru Rh Pd Ag Cd In Sn Sb Te I Xe Cs Ba La Ce Pr Nd Pm Sm Eu Gd Tb Dy Ho Er "
    "Tm Yb Lu Hf Ta W Re Os Ir Pt Au Hg Tl Pb Bi Po At Rn Fr Ra Ac Th Pa U Np Pu Am Cm Bk Cf Es Fm Md "
    "No Lr Rf Db Sg Bh Hs Mt Ds Rg Cn Nh Fl Mc Lv Ts Og".split())


def _is_float(token: str) -> bool:
    try:
        float(token)
        return True
    except ValueError:
        return False


def _header_at(lines: list[str], i: int):
    """A complete header (comment, one-token scale, three vectors, symbols, counts) at ``lines[i]``:
    (number of atoms, index of the line after it), else None."""
    if i + 7 > len(lines):
        return None
    scale = lines[i + 1].split()
    if len(scale) != 1 or not _is_float(scale[0]):
        return None
    for row in lines[i + 2:i + 5]:
        tokens = row.split()[:3]
        if len(tokens) != 3 or not all(_is_float(t) for t in tokens):
            return None
    symbols, counts = lines[i + 5].split(), lines[i + 6].split()
    if not symbols or len(counts) != len(symbols) or any(s not in _SYMBOLS for s in symbols):
        return None
    try:
        total = sum(max(int(c), 0) for c in counts)
    except ValueError:
        return None
    return total, i + 7


def _label_at(lines: list[str], i: int):
    """(first letter in lower case, index after the label) of the coordinate label at ``lines[i]``."""
    label = lines[i] if i < len(lines) else ""
    if label[:1].lower() == "s":
        i += 1
        label = lines[i] if i < len(lines) else ""
    return label[:1].lower(), i + 1


def has_repeated_header(data: bytes) -> bool:
    """True when, reading the file as an XDATCAR, a complete header followed by a label stands where
    a label is expected and is not the end-of-trajectory signal (an empty line or one that starts
    with white space).  The package reads such a file as a variable-cell run, which the reference
    does not know: the one deliberate difference.  Looks at the bytes only, never at an outcome."""
    lines = re.split("\r\n|\r|\n", data.decode("latin-1"))
    first = _header_at(lines, 0)
    if first is None:
        return False
    atoms, i = first
    while i < len(lines):
        label = lines[i]
        if not label or label[0].isspace():
            return False
        header = _header_at(lines, i)
        if header is not None and _label_at(lines, header[1])[0] in ("c", "d"):
            return True
        letter, after = _label_at(lines, i)
        if letter not in ("c", "d"):
            return False
        i = after + atoms
    return False
