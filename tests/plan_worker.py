"""Child process of the graph-plan tests (tests/test_host_logic.py): the plans of one knob group's cases through the
host-only ``rn_potgnn_debug_plan``, saved as ``<case name> -> flat int32 array``.  A process of its own because some
``RN_POTGNN_*`` knobs are read once per process: the parent passes the group's knobs in the environment.

usage: python -m tests.plan_worker <group index> <num_cus> <out.npz>"""
import ctypes as C
import sys

import numpy as np

from ramannoodle_amd import _lib
from tests.helpers import PLAN_KNOBS, plan_cases


def debug_plan(lib, shape, ea, eb, types, num_cus):
    n, e, k, fn, fe = shape
    cfg = _lib.Config(n, e, k, fn, fe, 2, -1.0, 0, 0)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    count = C.c_size_t(0)
    lib.rn_potgnn_debug_plan(C.byref(cfg), p(ea), p(eb), p(types), num_cus, None, 0, C.byref(count))  # asks for the size
    out = np.empty(count.value, dtype=np.int32)
    rc = lib.rn_potgnn_debug_plan(C.byref(cfg), p(ea), p(eb), p(types), num_cus, p(out), out.size, C.byref(count))
    assert rc == _lib.RN_OK and count.value == out.size, (rc, lib.rn_potgnn_last_error(None))
    return out


if __name__ == "__main__":
    lib = _lib.load()
    plans = {name: debug_plan(lib, shape, ea, eb, types, int(sys.argv[2]))
             for name, shape, ea, eb, types in plan_cases(PLAN_KNOBS[int(sys.argv[1])])}
    np.savez(sys.argv[3], **plans)
