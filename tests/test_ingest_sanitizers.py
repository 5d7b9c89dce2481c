"""The trajectory readers under AddressSanitizer + UBSan and under ThreadSanitizer, from a stand-alone
program (``tests/native/ingest_sweep.cpp``): compiled here together with ``csrc/ingest.cpp`` and
``csrc/ingest_vasprun.cpp``, run as a child process, exit status 0 and no sanitizer report required.
Nothing is loaded into Python under a sanitizer.

The readers map their files; a read past the end of a mapping shows in no Python test unless the
file happens to end on a page boundary.  So the sweep hands every input over twice: as a heap copy
of exactly its size (one byte too far is a report) and as a file padded to a whole number of pages
(one byte too far is a fault).  Inputs: every prefix of every committed fixture, and the recorded
family of damaged files of ``tests/test_ingest_mutants.py``.  Host-only; skipped on a machine with
a GPU (sanitizer runs belong on a CPU machine) and where the compiler cannot link with those flags.
"""
import os
import shutil
import struct
import subprocess

import pytest

from tests import ingest_mutants as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ramannoodle_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
SOURCES = [os.path.join(ROOT, "tests", "native", "ingest_sweep.cpp"), os.path.join(CSRC, "ingest.cpp"),
           os.path.join(CSRC, "ingest_vasprun.cpp")]
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
TSAN = ["-fsanitize=thread"]
REPORTS = ("Sanitizer", "runtime error:")


def _compile(flags, output, sources):
    return subprocess.Popen(["g++", "-std=c++17", "-pthread", "-O1", "-g", *flags, *sources, "-o", str(output)],
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _probe(tmp, name, flags):
    """None when a one-line program links with `flags`, else the reason to skip."""
    if os.path.exists("/dev/kfd"):
        return "a GPU machine: sanitizer runs belong on the CPU machine"
    if shutil.which("g++") is None:
        return "no g++"
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    build = _compile(flags, tmp / f"probe_{name}", [str(probe)])
    output, _ = build.communicate(timeout=120)
    if build.returncode != 0:
        return f"g++ cannot link a one-line program with {' '.join(flags)}: {output.strip()[-200:]}"
    return None


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    """Both sanitizer builds of the sweep, compiled side by side: name -> (executable, reason to skip or None)."""
    tmp = tmp_path_factory.mktemp("ingest_sanitizers")
    variants = {"asan": ASAN, "tsan": TSAN}
    skip = {name: _probe(tmp, name, flags) for name, flags in variants.items()}
    running = {name: _compile(flags, tmp / f"ingest_sweep_{name}", SOURCES) for name, flags in variants.items() if not skip[name]}
    for name, build in running.items():
        output, _ = build.communicate(timeout=300)
        assert build.returncode == 0, output[-3000:]
    return {name: (tmp / f"ingest_sweep_{name}", skip[name]) for name in variants}


def _export(family, path):
    """The family's tuples as the plain binary file ``ingest_sweep.cpp`` reads (format: there)."""
    with open(path, "wb") as f:
        f.write(b"RNMUT1\0\0" + struct.pack("<I", len(family.bases)))
        for base in family.bases:
            f.write(struct.pack("<I", len(base)) + base)
        f.write(struct.pack("<I", len(family.splices)))
        for deleted, inserted in family.splices:
            f.write(struct.pack("<II", deleted, len(inserted)) + inserted)
        f.write(struct.pack("<I", len(family)))
        for i in range(len(family)):
            f.write(struct.pack("<IIII", int(family.base[i]), int(family.op[i]), int(family.offset[i]), int(family.arg[i])))


def _run(command, timeout):
    done = subprocess.run(command, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, check=False)
    print(done.stdout.strip())
    assert done.returncode == 0, f"exit status {done.returncode}\n{done.stderr[-3000:]}"
    assert not any(word in done.stderr for word in REPORTS), done.stderr[-3000:]
    return done.stdout


def test_address_and_undefined_behaviour_sweep(builds, tmp_path):
    program, skip = builds["asan"]
    if skip:
        pytest.skip(skip)
    cases = {}
    for name, suffix in (("xdatcar", ".XDATCAR"), ("vasprun", ".xml")):
        directory = os.path.join(GOLDEN, name)
        cases[name] = program.parent / f"{name}_mutants.bin"  # beside the executable
        _export(M.Family(os.path.join(directory, "mutants.npz"), directory, suffix), cases[name])
    out = _run([str(program), "sweep", os.path.join(GOLDEN, "xdatcar"), os.path.join(GOLDEN, "vasprun"),
                str(cases["xdatcar"]), str(cases["vasprun"]), str(tmp_path)], timeout=300)
    assert "inputs from" in out


def test_threaded_reads_under_thread_sanitizer(builds, tmp_path):
    program, skip = builds["tsan"]
    if skip:
        pytest.skip(skip)
    out = _run([str(program), "threads", str(tmp_path)], timeout=120)
    assert "threaded reads" in out
