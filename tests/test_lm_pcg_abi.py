"""sgo_optimize_lm_pcg and sgo_lm_pcg_trace (include/sgo.h) are declared, bound and exported, and refuse a null context without a device."""
import ctypes as C
import os
import re

from sparse_gslam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sgo_optimize_lm_pcg", "sgo_lm_pcg_trace")


def test_the_two_symbols_are_declared_bound_and_exported(sgo_lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgo.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in capi.SYMBOLS and hasattr(sgo_lib, name), name
    assert re.search(r"#define\s+SGO_LM_SOLVE_CONVERGED\s+%d\b" % capi.LM_SOLVE_CONVERGED, src)
    assert re.search(r"#define\s+SGO_LM_SOLVE_FLOOR\s+%d\b" % capi.LM_SOLVE_FLOOR, src)
    assert sgo_lib.sgo_version() == 107
    assert callable(capi.Optimizer.optimize_lm_pcg) and callable(capi.Optimizer.lm_pcg_trace)


def test_a_null_context_is_einval():
    L = capi.lib()
    st = capi.LmStats()
    C.memset(C.byref(st), 0x5A, C.sizeof(st))
    before = bytes(st)
    assert L.sgo_optimize_lm_pcg(None, 3, 0.0, C.byref(st)) == -2 and bytes(st) == before
    assert L.sgo_optimize_lm_pcg(None, 3, 0.0, None) == -2
    its = (C.c_int32 * 4)(7, 7, 7, 7)
    assert L.sgo_lm_pcg_trace(None, 4, its, None) == -2 and list(its) == [7, 7, 7, 7]
    assert L.sgo_lm_pcg_trace(None, 0, None, None) == -2
