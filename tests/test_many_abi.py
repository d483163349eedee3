"""sgo_optimize_gn_many at the boundary, without a device: the symbols, sgo_many_result's layout, the binding, and the refusals
that are decided before anything touches a GPU."""
import ctypes as C
import os
import re

from sparse_gslam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_struct_and_binding(sgo_lib):
    for name in ("sgo_optimize_gn_many", "sgo_many_workspace_bytes"):
        assert name in capi.SYMBOLS and hasattr(sgo_lib, name), name
    src = open(os.path.join(ROOT, "include", "sgo.h")).read()
    body = re.search(r"typedef struct sgo_many_result \{(.*?)\} sgo_many_result;", src, re.S).group(1)
    fields = re.findall(r"int32_t\s+(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == ["rc", "stop_reason", "in_launch"] == [f for f, _ in capi.ManyResult._fields_]
    assert C.sizeof(capi.ManyResult) == 12 and all(t is C.c_int32 for _, t in capi.ManyResult._fields_)
    assert callable(capi.optimize_many) and callable(capi.Optimizer.many_workspace_bytes)
    assert sgo_lib.sgo_many_workspace_bytes(None) == -2


def test_no_contexts_is_no_work(sgo_lib):
    launches = C.c_int32(-7)
    assert sgo_lib.sgo_optimize_gn_many(None, 0, 20, 0.0, None, None, C.byref(launches)) == 0 and launches.value == 0
    assert capi.optimize_many([]) == ([], 0)


def test_null_arguments_are_refused_without_a_device(sgo_lib):
    res = (capi.ManyResult * 2)()
    for r in res:
        r.rc = r.stop_reason = r.in_launch = -7
    launches = C.c_int32(-7)
    none = (C.c_void_p * 2)(None, None)
    for what, args in (("NULL ctxs", (None, 2, 20, 0.0, None, res, C.byref(launches))),
                       ("NULL res", (none, 2, 20, 0.0, None, None, C.byref(launches))),
                       ("NULL contexts", (none, 2, 20, 0.0, None, res, C.byref(launches))),
                       ("n < 0", (None, -1, 20, 0.0, None, res, C.byref(launches))),
                       ("max_iters", (None, 0, capi.SGO_MAX_ITERS + 1, 0.0, None, res, C.byref(launches))),
                       ("gain_tol", (None, 0, 20, float("nan"), None, res, C.byref(launches)))):
        assert sgo_lib.sgo_optimize_gn_many(*args) == -2, what
        assert b"sgo_optimize_gn_many" in sgo_lib.sgo_last_error(None), what
        assert launches.value == -7 and all((r.rc, r.stop_reason, r.in_launch) == (-7, -7, -7) for r in res), what
