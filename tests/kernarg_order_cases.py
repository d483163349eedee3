"""The cases of tests/test_gpu_kernarg_order.py and of scripts/make_golden_kernarg_order.py, which records their results.

The kernels of the solve take their pointers as plain leading parameters and two of these often have the
same type: a swapped pair compiles.  Every case is a small graph that sends optimize(4) through one group of those kernels;
what it returns (chi2 of every iterate, PCG iteration counts, final poses) was recorded before the parameters were reordered
and has to come back bit for bit.  All cases run with direct_rows=0, so that the PCG path is taken whatever the size."""
from __future__ import annotations

import contextlib
import os

import numpy as np

from sparse_gslam_amd import capi, synth

ITERS = 4
MODES = (("graph", dict(use_graph=1)), ("plain", dict(use_graph=0)), ("profile", dict(profile=1)))


def _closed(V, E, seed, **kw):
    g = synth.manhattan(V, E, seed, **kw)
    return dict(graph=g.arrays())


def _append():
    base, steps, gg = synth.append_session(600, 2400, 1, 16, seed=5)
    st = steps[0]
    arrs = [np.concatenate([getattr(base, k), st[k]]) for k in ("ei", "ej", "meas", "info", "phi")]
    fixed = np.zeros(st["V"], dtype=bool)
    fixed[0] = True
    return dict(graph=base.arrays(), append=dict(V=st["V"], fixed=fixed, arrs=arrs, n_resident=base.E, odom=gg.meas[: gg.V - 1]))


# name -> (environment, builder): the kernels the case is there for are named in the comment
CASES = {
    # k_spmv0t (all three tile passes), the folded level-0 transfers, k_spmv / k_up_fold on the coarse levels
    "tile": (dict(SGO_SPMV0="tile"), lambda: _closed(2000, 8000, 1, info_mode="full")),
    # k_spmv0 / k_jacobi0_restrict, k_prolong_fold: the wave-group kernel a graph of this size takes by itself
    "wave_group": (dict(), lambda: _closed(2000, 8000, 1, info_mode="full")),
    # the unfolded cycle: explicit sweeps, k_restrict_p / k_prolong_p on their own
    "no_fold_tile": (dict(SGO_SPMV0="tile", SGO_AMG_FOLD="0"), lambda: _closed(2000, 8000, 1, info_mode="full")),
    "no_fold_wave_group": (dict(SGO_AMG_FOLD="0"), lambda: _closed(2000, 8000, 1, info_mode="full")),
    # random closures: tentative levels and the K-cycle (k_spmv's dot modes, k_restrict, k_prolong_add)
    "tentative_kcycle": (dict(), lambda: _closed(2000, 12000, 2, p_random=0.05)),
    # a dense single level: k_dense_fill, k_gj_pivot / k_gj_step, k_dense_apply
    "dense_level": (dict(), lambda: _closed(300, 1200, 3, info_mode="full")),
    # the block-Jacobi recurrence: k_precond_bj, k_update_xr, k_update_p, k_dot without a cycle between them
    "block_jacobi": (dict(SGO_SOLVER="pcg"), lambda: _closed(255, 1000, 4, info_mode="full")),
    # one incremental append: the overlay's launches around the reordered ones
    "append": (dict(), _append),
}


# The four runs of the first graph end within a few units of the last place of each other: the fixture keeps the poses of
# XOR_BASE as they are and, of the other three, the bit patterns XORed with XOR_BASE's -- the same bits, a quarter of the file.
XOR_BASE = "wave_group"
XOR_CASES = ("tile", "no_fold_tile", "no_fold_wave_group")


def save(path, results):
    """results: name -> run()'s dict"""
    rec = {}
    for name, r in results.items():
        for k, v in r.items():
            if k == "poses" and name in XOR_CASES:
                rec[f"{name}.poses_xor"] = v.view(np.uint64) ^ results[XOR_BASE]["poses"].view(np.uint64)
            else:
                rec[f"{name}.{k}"] = v
    np.savez_compressed(path, **rec)


def load(path):
    """name -> dict(chi2, robust_chi2, pcg_iters, poses), as save() was given them"""
    out = {}
    with np.load(path) as z:
        for key in z.files:
            name, k = key.split(".")
            out.setdefault(name, {})[k] = z[key]
    for name in XOR_CASES:
        out[name]["poses"] = (out[name].pop("poses_xor") ^ out[XOR_BASE]["poses"].view(np.uint64)).view(np.float64)
    return out


@contextlib.contextmanager
def environment(env):
    keys = ("SGO_SPMV0", "SGO_AMG_FOLD", "SGO_SOLVER")
    old = {k: os.environ.get(k) for k in keys}
    try:
        for k in keys:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run(name, mode_opts):
    """optimize(ITERS) of the case in one execution mode -> dict(chi2, robust_chi2, pcg_iters, poses)"""
    env, builder = CASES[name]
    c = builder()
    with environment(env), capi.Optimizer(0, direct_rows=0, **mode_opts) as opt:
        opt.set_graph(*c["graph"])
        if "append" in c:
            a = c["append"]
            opt.optimize(ITERS)
            P = opt.get_poses()
            P0 = np.empty((a["V"], 3))
            P0[: P.shape[0]] = P
            synth.chain_init(P0, a["odom"], P.shape[0], a["V"] - 1)
            opt.update_graph(P0, a["fixed"], *a["arrs"], a["n_resident"])
            assert "incremental overlay" in opt.solver_description()
        done, st = opt.optimize(ITERS)
        assert done == ITERS, (name, done)
        return dict(chi2=np.array(st["chi2"]), robust_chi2=np.array(st["robust_chi2"]),
                    pcg_iters=np.array(st["pcg_iters"], dtype=np.int32), poses=opt.get_poses())
