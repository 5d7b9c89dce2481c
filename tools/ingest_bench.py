#!/usr/bin/env python3
"""Parse rate of the native XDATCAR and vasprun.xml readers on a synthetic trajectory (config-3 shape:
256 atoms): open + read of the whole file, median of five runs per thread count.
usage: ingest_bench.py [frames] [--reference]   (--reference also times the reference's Python
parser; build container only, needs /root/reference)"""
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ramannoodle_amd.io.vasp import vasprun, xdatcar  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 2000
atoms = 256
rng = np.random.default_rng(0)
with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "XDATCAR")
    with open(path, "w", encoding="utf-8") as f:
        f.write(f"synthetic\n 1.0\n 16.8 0 0\n 0 16.8 0\n 0 0 8.4\n Mg O\n {atoms // 2} {atoms // 2}\n")
        for k in range(frames):
            f.write(f"Direct configuration= {k + 1:5d}\n")
            np.savetxt(f, rng.uniform(size=(atoms, 3)), fmt="  %.8f")
    xml_path = os.path.join(tmp, "vasprun.xml")
    with open(xml_path, "w", encoding="utf-8") as f:
        f.write('<?xml version="1.0" encoding="ISO-8859-1"?>\n<modeling>\n <parameters><separator name="ionic">'
                '<i name="POTIM">  1.00000000</i></separator></parameters>\n')
        for k in range(frames):
            f.write(' <structure>\n  <crystal>\n   <varray name="basis" >\n    <v> 16.8 0.0 0.0 </v>\n    <v> 0.0 16.8 0.0 </v>\n'
                    '    <v> 0.0 0.0 8.4 </v>\n   </varray>\n  </crystal>\n  <varray name="positions" >\n')
            np.savetxt(f, rng.uniform(size=(atoms, 3)), fmt="   <v> %16.8f %16.8f %16.8f </v>")
            f.write("  </varray>\n </structure>\n")
        f.write("</modeling>\n")
    for what, file, opener in (("XDATCAR", path, xdatcar.XdatcarReader), ("vasprun.xml", xml_path, vasprun.VasprunReader)):
        size = os.path.getsize(file) / 1e6
        for threads in (1, 8, 0):  # (auto: at most 16)
            times = []
            for _ in range(5):
                t = time.perf_counter()
                with opener(file) as reader:
                    pos = reader.read(num_threads=threads)
                times.append(time.perf_counter() - t)
                if what == "XDATCAR":
                    xdatcar_pos = pos
            dt = float(np.median(times))
            print(f"native {what} reader, threads={threads or 'auto'}: {frames} frames x {atoms} atoms, {size:.1f} MB in "
                  f"{dt * 1e3:.1f} ms (median of 5; {min(times) * 1e3:.1f}..{max(times) * 1e3:.1f}) = {size / dt:.0f} MB/s = "
                  f"{frames / dt:.0f} frames/s")
    pos, size = xdatcar_pos, os.path.getsize(path) / 1e6
    if "--reference" in sys.argv:
        sys.dont_write_bytecode = True
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"))
        sys.path.insert(0, "/root/reference")
        import _standins
        _standins.install()
        from ramannoodle.io.vasp.xdatcar import read_positions_ts
        t = time.perf_counter()
        ref = read_positions_ts(path)
        dt = time.perf_counter() - t
        print(f"reference Python parser: {dt * 1e3:.0f} ms = {size / dt:.1f} MB/s = {frames / dt:.0f} frames/s; "
              f"bit-identical: {np.array_equal(ref, pos)}")
