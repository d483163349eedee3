"""The resident multigrid hierarchy and its cycle against tests/amg_reference.py, stage by stage.

Every case linearises, exports the hierarchy through sgo_debug_amg_array (exactly what the next sgo_precondition and the next
refresh read), runs every applicable stage of the reference and compares sgo_precondition on three vectors -- two random, one with rows scaled
by 10^+-6 -- with stage 9; where a level runs the K-cycle's flexible CG (a tentative level always does), also with stage 10 on the
exported work vectors (test_gpu_kcycle_reference.py has the K-cycle's own cases).  A case asserts the shape it exists for, read from the
export and sgo_solver_description, and a failing case reports every stage's worst ratio and where it was.  Each case prints its
figures before it asserts (run with -s to see them).

Measured on the MI355X, worst error / (U abs) per stage over the case classes (constants in amg_reference.C_STAGE / K_CYCLE):
the table above amg_reference.MEASURED.  The file adds about 75 s of GPU-machine time (C4: 15 s;
C4r with its K-cycle stages: 7 s).
"""
import json

import numpy as np
import pytest

import amg_reference as ar
from sparse_gslam_amd import capi, synth
from test_gpu_kcycle_reference import kcycle_vectors
from test_gpu_kernel_reference import _hubs, _vectors
from test_gpu_setup_pipeline import _graph as _fixed_and_duplicates

pytestmark = pytest.mark.gpu


def check(case, o, fixed, cycle=True, check_mask=True, seed=0):
    """Linearise, export, run every stage; returns (levels, description, report)."""
    o.linearize()
    lv = ar.export_hierarchy(o)
    desc = o.solver_description()
    assert len(lv) >= 2, desc
    n = lv[0]["n"]
    order = lv[0]["row_order"].astype(np.int64)          # hessian row -> internal row
    xy = np.empty((n, 2))
    xy[order] = o.get_poses()[np.flatnonzero(~np.asarray(fixed, dtype=bool))][:, :2]
    res = ar.check_hierarchy(lv, poses_xy=xy, check_mask=check_mask)
    worst = {k: (round(v[0], 3), v[1], v[2], v[3]) for k, v in ar.worst_by_stage(res).items()}
    tentative = [l for l, L in enumerate(lv[:-1]) if not L["smoothed"]]
    # cycle=True: a V-cycle hierarchy is expected (stage 9 against K_CYCLE); False: a tentative level is expected, whose cycle is
    # the K-cycle (stage 9 with the flexible-CG driver against K_KCYCLE, and stage 10 on the exported work vectors)
    assert bool(tentative) != bool(cycle) and ar.has_kcycle(lv) != bool(cycle), (case, "tentative levels", tentative, desc)
    cyc, kstep, kbad = [], {}, {}
    if cycle:
        for r in _vectors(n, seed):
            z = o.precondition(r)
            ri, zi = np.empty((n, 3)), np.empty((n, 3))
            ri[order], zi[order] = r, z
            zr, eps = ar.cycle_scale(lv, ri)
            cyc.append((ar.cycle_ratio(zi, zr, eps), eps))
    else:
        kstep, kc, kbad, _ = kcycle_vectors(o, lv, list(zip(("random", "uniform", "scaled"), _vectors(n, seed))))
        cyc = [(c[1], c[2]) for c in kc]
    shape = [dict(l=l, n=L["n"], nslot=L["nslot"], smoothed=L["smoothed"], filtered=L["filtered"], kind=L["kind"], nu=L["nu"],
                  t_nlong=L["t_nlong"], ps_t_nlong=L["ps_t_nlong"], f32=L["f32"], max_row=int(np.diff(L["rowptr"]).max()),
                  max_aggregate=int(np.diff(L["mem_ptr"]).max()) if "mem_ptr" in L else 0,
                  max_p_column=int(np.bincount(L["p_col"]).max()) if "p_col" in L else 0,
                  folded_worst=L.get("_folded_worst")) for l, L in enumerate(lv)]
    report = dict(case=case, desc=desc, worst=worst, cycle=cyc, kcycle_steps=kstep, kappa_coarsest=lv[-1].get("_kappa"), shape=shape)
    print("AMGREF " + json.dumps(report, default=str))
    bad = ar.failures(res)
    assert not bad, (case, bad, worst)
    assert not kbad, (case, kbad, kstep)
    assert len(cyc) == 3 and all(r <= (ar.K_CYCLE if cycle else ar.K_KCYCLE) for r, _ in cyc), (case, cyc, worst)
    return lv, desc, report


def _run(case, g, **kw):
    arrs = g.arrays() if hasattr(g, "arrays") else g
    with capi.Optimizer(0, direct_rows=0) as o:
        o.set_graph(*arrs)
        return check(case, o, arrs[1], **kw)


def _all_smoothed(lv):
    return all(L["smoothed"] for L in lv[:-1])


def _coarse_folded(lv):
    return all(L["kind"] in (ar.FOLDED, ar.FOLDED2) for L in lv[1:-1])


# ------------------------------------------------------------------ smoothed hierarchies, level 0 folded
@pytest.mark.parametrize("name", ["C1", "C2"])
def test_smoothed_levels_and_a_folded_level0(name):
    lv, desc, _ = _run(f"{name}_full", synth.config(name, info_mode="full"))
    assert _all_smoothed(lv) and not any(L["filtered"] for L in lv[:-1]), desc
    assert lv[0]["folded"] and lv[0]["kind"] == ar.FOLDED, desc


def _c2_odom():
    return synth.config("C2", info_mode="full", init="odom")


def _c2_odom_heavy():
    """C2 from the dead-reckoned start plus six closures of 10^8 times the usual weight, on both odometry neighbours of three
    poses: next to such neighbours a pose's own connections all fall below theta_filter sqrt(w_ii w_jj), the first of the two
    documented reasons for a zeroed dinvF row (k_filtered_diag: "both neighbours heavy hubs")."""
    from oracle import np_oracle as npo
    g = _c2_odom()
    a = np.array([1000, 4000, 7000])
    hi, hj = np.r_[a - 1, a + 1], np.r_[a + 300, a + 400]
    meas = npo.se2_mul(npo.se2_inv(g.poses[hi]), g.poses[hj])
    info = np.tile(np.array([1e10, 0.0, 0.0, 1e10, 0.0, 1e10]), (hi.size, 1))
    return synth.Graph(g.poses, g.fixed, np.r_[g.ei, hi].astype(np.int32), np.r_[g.ej, hj].astype(np.int32), np.r_[g.meas, meas],
                       np.r_[g.info, info], np.r_[g.phi, np.full(hi.size, -1.0)])


def test_filtered_smoothing_from_the_dead_reckoned_start():
    """Filtered smoothing on level 0.  C2 from the dead-reckoned start itself zeroes none of its 9 999 rows of dinvF (measured on
    the MI355X and recomputed from the formulas on the CPU, with diagonal and with full information: every row keeps a connection
    and trace(D^-1 L) stays below 0.05), so it asserts the non-zero rows; the zeroed ones: the next case."""
    lv, desc, _ = _run("C2_odom", _c2_odom())
    assert lv[0]["smoothed"] and lv[0]["filtered"] and "filtered" in desc, desc
    assert lv[0]["_zero_rows"] == 0 and lv[0]["_nonzero_rows"] == lv[0]["n"], (lv[0]["_zero_rows"], lv[0]["_nonzero_rows"])


def test_filtered_smoothing_with_zeroed_and_nonzero_rows():
    """The same start with three poses between heavy neighbours: at least one zeroed row of dinvF and at least one non-zero one,
    every zeroed row explained by the reference (stage 3) and turned into the tentative row T(d_i) (stage 4)."""
    lv, desc, _ = _run("C2_odom_heavy_neighbours", _c2_odom_heavy())
    assert lv[0]["smoothed"] and lv[0]["filtered"] and "filtered" in desc, desc
    assert lv[0]["_zero_rows"] >= 1 and lv[0]["_nonzero_rows"] >= 1, (lv[0]["_zero_rows"], lv[0]["_nonzero_rows"])


def test_30k_300k_folded_level0_with_long_columns_of_the_folded_transfer():
    """30 k poses are below the size from which level 0 stays unfolded (AmgConfig::fold0_rows = 60 000): level 0 is folded here, the
    coarse levels run one explicit sweep around the folded form (nu = 2), and P~ has columns longer than 512 entries (the
    workgroup-per-column path of the restriction).  The unfolded level 0 over folded coarse levels: the next two cases."""
    lv, desc, _ = _run("manhattan_30k_300k", synth.manhattan(30000, 300000, seed=12, info_mode="full"))
    assert _all_smoothed(lv) and len(lv) >= 3, desc
    assert lv[0]["kind"] == ar.FOLDED and _coarse_folded(lv) and lv[0]["f32"] == 1, desc
    assert lv[0]["ps_t_nlong"] > 0 and int(np.bincount(lv[0]["ap_col"]).max()) > 512, desc


def test_unfolded_level0_over_folded_coarse_levels():
    lv, desc, _ = _run("manhattan_70k_250k", synth.manhattan(70000, 250000, seed=13, info_mode="full"))
    assert _all_smoothed(lv) and len(lv) >= 3, desc
    assert lv[0]["kind"] == ar.UNFOLDED and not lv[0]["folded"] and _coarse_folded(lv), desc


def test_c4_two_sweeps_around_the_folded_cycle_and_long_columns_of_p():
    """C4: level 0 unfolded, nu = 2 as one explicit sweep around the folded cycle on the coarse levels, 13 M products of A P (the
    reference runs in chunks), and columns of P longer than 512 entries: k_restrict_p_long's workgroup-per-column path."""
    lv, desc, _ = _run("C4", synth.config("C4"))
    assert _all_smoothed(lv) and "nu=2" in desc, desc
    assert lv[0]["kind"] == ar.UNFOLDED and any(L["nu"] == 2 and L["kind"] == ar.FOLDED2 for L in lv[1:-1]), desc
    assert lv[0]["f32"] == 1, desc
    assert lv[0]["t_nlong"] > 0 and int(np.bincount(lv[0]["p_col"]).max()) > 512, desc


def test_tentative_levels_of_a_graph_with_random_closures():
    """Stages 1, 2, 6 and 8, and the K-cycle of its tentative levels: stages 9 and 10."""
    lv, desc, rep = _run("manhattan_20k_random_closures", synth.manhattan(20000, 120000, seed=21, p_random=0.05, info_mode="full"),
                         cycle=False)
    assert any(not L["smoothed"] for L in lv[:-1]), desc
    assert len(rep["cycle"]) == 3 and rep["kcycle_steps"]


def test_c4r_stalled_hierarchy_with_a_large_aggregate():
    """C4 with 5 % random closures: tentative levels whose coarsening stalls, the last one collapsing into aggregates of more than
    64 members (k_centres' wave-per-aggregate sums, k_restrict's long groups).  Stages 1, 2, 6 and 8, and the K-cycle: stages 9 and 10
    (three vectors: the reference takes about as long as C4's)."""
    lv, desc, rep = _run("C4r", synth.config("C4r"), cycle=False)
    assert any(not L["smoothed"] for L in lv[:-1]), desc
    assert max(int(np.diff(L["mem_ptr"]).max()) for L in lv[:-1]) > 64, desc
    assert len(rep["cycle"]) == 3 and rep["kcycle_steps"]


def test_hubs_rows_longer_than_a_wave():
    """Hubs of 65, 130 and 1000 edges: rows longer than 64 slots on level 0 and above (a tentative hierarchy: stages 1, 2, 6, 8, and 9, 10 for its K-cycle).
    Its largest aggregate has 19 members (measured on the MI355X; asserted, so that a change of it is seen): the aggregate of
    more than 64 members is asserted where one occurs, on C4r's stalled last level (627 members)."""
    lv, desc, _ = _run("hubs_65_130_1000", _hubs(), cycle=False)
    assert int(np.diff(lv[0]["rowptr"]).max()) > 1000 and max(int(np.diff(L["rowptr"]).max()) for L in lv[1:]) > 64, desc
    assert max(int(np.diff(L["mem_ptr"]).max()) for L in lv[:-1]) <= 64, desc


def test_fixed_vertices_mid_graph_and_duplicate_edges():
    arrs = _fixed_and_duplicates(0.0)
    lv, desc, _ = _run("fixed_mid_graph_and_duplicates", arrs)
    row = ar.slot_rows(lv[0])
    keys = row * lv[0]["n"] + lv[0]["col"]
    assert np.unique(keys).size < keys.size, "no duplicate logical slot"
    assert lv[0]["n"] == int((~arrs[1]).sum())


def test_refresh_path_after_optimize(monkeypatch):
    """After optimize(3) with the coarse operators refreshed before every solve: every stage holds again at the GPU's own poses
    (amg_update, not only the set-up's level_values)."""
    monkeypatch.setenv("SGO_AMG_LAG", "0")
    g = synth.config("C2", info_mode="full")
    with capi.Optimizer(0, direct_rows=0) as o:
        o.set_graph(*g.arrays())
        done, _ = o.optimize(3)
        assert done == 3
        assert np.abs(o.get_poses() - g.poses).max() > 1e-6
        check("C2_after_optimize3", o, g.fixed, check_mask=False, seed=1)


# ------------------------------------------------------------------ every producer, absolutely
PRODUCERS = {"setup_host": dict(SGO_AMG_SETUP="host"), "lists_host": dict(SGO_AMG_LISTS="host"), "agg_device": dict(SGO_AMG_AGG="device"),
             "kept_aggregates_rebuild": dict(SGO_AMG_FORCE_REBUILD="1", SGO_AMG_KEEP_AGG="1")}


@pytest.mark.parametrize("producer", list(PRODUCERS))
@pytest.mark.parametrize("base", ["C2_full", "C2_odom"])
def test_each_producer_is_checked_on_its_own(base, producer, monkeypatch):
    for k, v in PRODUCERS[producer].items():
        monkeypatch.setenv(k, v)
    g = synth.config("C2", info_mode="full") if base == "C2_full" else _c2_odom()
    with capi.Optimizer(0, direct_rows=0) as o:
        o.set_graph(*g.arrays())
        rebuilt = producer == "kept_aggregates_rebuild"
        if rebuilt:   # the rebuild happens before the call's first solve; the poses then move: the mask is the rebuild's
            done, _ = o.optimize(1)
            assert done == 1
        lv, desc, _ = check(f"{base}_{producer}", o, g.fixed, check_mask=not rebuilt)
    assert lv[0]["smoothed"], desc
    if base == "C2_odom":   # (the device's own aggregation ends up filtering level 1 instead of level 0)
        assert any(L["filtered"] for L in lv[:-1]), desc


@pytest.mark.parametrize("base", ["C2_full", "C2_odom"])
@pytest.mark.parametrize("env,f32,folded", [(dict(SGO_SPMV0="tile"), 1, True), (dict(SGO_SPMV0="tile", SGO_PRECOND_F32="0"), 0, True),
                                            (dict(SGO_AMG_FOLD="0"), 0, False)], ids=["tile_f32", "tile_f64", "fold_off"])
def test_fp32_level0_copy_and_unfolded_cycle(base, env, f32, folded, monkeypatch):
    """C2 and the filtered case with the level-0 passes on the tile kernel's fp32 copy, on its fp64 blocks, and with the sweeps
    as launches of their own."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g = synth.config("C2", info_mode="full") if base == "C2_full" else _c2_odom()
    lv, desc, _ = _run(base + "_" + "_".join(f"{k}={v}" for k, v in env.items()), g)
    assert lv[0]["f32"] == f32 and ("blk32" in lv[0]) == bool(f32), desc
    assert any(L["folded"] for L in lv[:-1]) == folded, desc
    if base == "C2_odom":
        assert any(L["filtered"] for L in lv[:-1]), desc
