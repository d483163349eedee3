"""The multi-GPU modes of libsgo run for real with world_size > 1 on ONE GPU.

RCCL refuses two ranks on one device, and the GPU box has one: the ranks here are separate processes that
share the card and exchange through libsgo's caller-supplied transport (sgo_comm_init_host) with gloo
underneath.  Everything else is the product's multi-rank path as bench.py --gpus N drives it: every rank
marshals the same graph and
  * row-owner mode (graphs whose closures are spatially local: thin boundaries in Hilbert order): linearises, multiplies,
    smooths, restricts, prolongates and updates its own rows only, exchanges boundary rows and partial dot products,
    all-reduces the coarse right-hand sides, the level-1 Galerkin blocks and chi2;
  * all-reduce mode (random long-range closures: every row is a boundary row): evaluates its own range of tiles in every
    level-0 pass and all-reduces the product vectors;
set-up, multigrid hierarchy, optimize(), stopping and rebuild decisions included.  Checked: no rank hangs or diverges
(all ranks bit-identical, same number of collectives), and the result equals the 1-rank path through the same
transport and the single-GPU path to rounding."""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _graph(name):
    from sparse_gslam_amd import synth
    if name == "C2":
        return synth.config("C2", info_mode="full")
    if name == "random":     # long-range closures: the tentative-prolongator fallback levels
        return synth.manhattan(8000, 32000, seed=11, info_mode="full", p_random=0.05)
    if name == "rebuild":    # robust-kernel re-weighting from a dead-reckoned start: the hierarchy is rebuilt inside optimize()
        return synth.manhattan(V=3000, E=4500, seed=1, p_random=0.3, info_mode="diag", phi=1.0, init="odom")
    if name == "bj":         # the block-Jacobi solver BASELINE.json names (thousands of PCG iterations: a small graph, one GN iteration)
        return synth.manhattan(3000, 12000, seed=5, info_mode="full")
    if name == "C4":         # configs[3] at full size (100k poses / 1M edges): the bench workload of bench.py --gpus N
        return synth.config("C4")
    if name == "tiny":       # fewer level-0 tiles than ranks (a rank's range would be empty): runs replicated on every rank
        return synth.manhattan(700, 760, seed=9, info_mode="full")
    if name == "pipelined":  # >= 20 000 free poses: the set-up's helper thread is active on every rank (bench.py's C4 at N > 1)
        return synth.manhattan(24000, 150000, seed=77, info_mode="full")
    raise KeyError(name)


def _opts(name):
    from sparse_gslam_amd import capi
    return dict(solver=capi.SOLVER_PCG_BJ, pcg_maxit=100000) if name == "bj" else {}


def _worker(rank, world, port, name, iters, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from sparse_gslam_amd import capi
        g = _graph(name)
        calls = [0]

        def allreduce(a):
            t = torch.from_numpy(a)
            dist.all_reduce(t)
            calls[0] += 1

        def allgather(send, recv):     # the optional companion transport of the row-owner mode's packets
            out = [torch.empty(send.size, dtype=torch.float64) for _ in range(world)]
            dist.all_gather(out, torch.from_numpy(send.copy()))
            for r, t in enumerate(out):
                recv[r * send.size:(r + 1) * send.size] = t.numpy()
            calls[0] += 1

        with capi.Optimizer(0, **_opts(name)) as o:
            # (one case brings a real all-gather; the others let libsgo perform it as an all-reduce of zero-padded slots)
            o.comm_init_host(world, rank, allreduce, allgather if name == "pipelined" else None)
            o.set_graph(*g.arrays())
            done, st = o.optimize(iters)
            P = o.get_poses()
            c, rc = o.chi2()
            desc = o.solver_description() + f" level0_bytes={o.level0_bytes()}"
        q.put((rank, done, st["chi2"], st["pcg_iters"], P.tobytes(), c, rc, calls[0], desc))
    except Exception as e:   # report instead of leaving the parent waiting on the queue
        q.put((rank, -1, repr(e), [], b"", 0.0, 0.0, 0, ""))
        raise
    finally:
        dist.destroy_process_group()


def _run(world, name, iters):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, name, iters, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return res


@pytest.mark.parametrize("world,name,mode", [(2, "C2", "owner"), (3, "C2", "owner"), (2, "random", "owner"), (2, "random", "allreduce"),
                                             (3, "C2", "allreduce"), (2, "pipelined", "owner"), (2, "bj", "owner")])
def test_ranks_agree_bitwise_and_match_one_rank(world, name, mode, monkeypatch):
    from sparse_gslam_amd import capi
    iters = 1 if name == "bj" else 5
    # the library picks the mode by the share of boundary rows (C2, pipelined: 2-5 %; random: 20 %: still row-owner; beyond
    # a quarter of the rows: all-reduce); the all-reduce cases force it so that both modes run on the same graphs
    if mode == "allreduce":
        monkeypatch.setenv("SGO_COMM_MODE", "allreduce")     # (inherited by the spawned rank processes)
    res = _run(world, name, iters)
    assert all(r[1] == iters for r in res), [r[:3] for r in res]
    _, _, chi2_0, its_0, P0, c0, rc0, calls0, desc0 = res[0]
    assert ("all-reduce mode" if mode == "allreduce" else "row-owner mode") in desc0, desc0
    for r in res[1:]:        # every rank holds the same iterates, bit for bit, and took the same decisions
        assert r[2] == chi2_0 and r[3] == its_0 and r[4] == P0 and r[7] == calls0
    assert calls0 >= 3 * sum(its_0)     # two product vectors + one coarse right-hand side per PCG iteration
    g = _graph(name)
    rank_bytes = [int(r[8].rsplit("level0_bytes=", 1)[1]) for r in res]
    # one rank through the same transport
    with capi.Optimizer(0, **_opts(name)) as o:
        o.comm_init_host(1, 0, lambda a: None)
        o.set_graph(*g.arrays())
        d1, s1 = o.optimize(iters)
        P1 = o.get_poses()
        bytes1 = o.level0_bytes()
    if mode == "owner":
        # a rank holds the level-0 blocks, edge operands, transfer blocks and product lists of ITS rows: 1 / world of the
        # one-rank bytes each, up to the pairs the 256-per-rank tile cut stores twice and the entries kept for the boundary
        assert max(rank_bytes) <= 1.25 * bytes1 / world + (4 << 20), (rank_bytes, bytes1)
        assert sum(rank_bytes) <= 1.25 * bytes1 + world * (4 << 20), (rank_bytes, bytes1)
    else:
        assert min(rank_bytes) >= 0.9 * bytes1      # all-reduce mode: every rank holds the whole graph
    assert d1 == iters and max(abs(a - b) for a, b in zip(s1["pcg_iters"], its_0)) <= (1 if name != "bj" else 0.02 * max(its_0))
    # (two PCG solves to 1e-8 with differently rounded coarse right-hand sides: poses agree to the solves' accuracy)
    assert np.abs(np.frombuffer(P0, dtype=np.float64).reshape(-1, 3) - P1).max() <= 1e-6
    for a, b in zip(chi2_0, s1["chi2"]):
        assert abs(a - b) <= 1e-7 * b   # (the solves' tolerance: a tenth of BASELINE.json's bound)
    # and the single-GPU path (fused dot products, hipGraph replay): agreement to rounding
    with capi.Optimizer(0, **_opts(name)) as o:
        o.set_graph(*g.arrays())
        ds, ss = o.optimize(iters)
        Ps = o.get_poses()
    assert ds == iters
    assert np.abs(Ps - P1).max() <= 1e-6
    for a, b in zip(chi2_0, ss["chi2"]):
        assert abs(a - b) <= 1e-7 * b   # (the solves' tolerance: a tenth of BASELINE.json's bound)


def test_c4_full_size_two_ranks_row_owner_mode_matches_the_direct_solver_golden():
    """configs[3] (100k poses / 1M edges) with two rank processes in row-owner mode: every iterate's chi2 within BASELINE.json's
    1e-6 of the sparse-direct-solver oracle's fixture (tests/golden/C4_direct.npz), ranks bit-identical, and each rank holds
    about half of the level-0 structure."""
    import os as _os
    f = np.load(_os.path.join(_os.path.dirname(__file__), "golden", "C4_direct.npz"))
    iters = 4
    res = _run(2, "C4", iters)
    assert all(r[1] == iters for r in res), [r[:3] for r in res]
    assert "row-owner mode" in res[0][8], res[0][8]
    assert res[0][2] == res[1][2] and res[0][3] == res[1][3] and res[0][4] == res[1][4]
    for k in range(iters + 1):
        assert abs(res[0][2][k] - f["chi2"][k]) <= 1e-6 * f["chi2"][k], k
    b = [int(r[8].rsplit("level0_bytes=", 1)[1]) for r in res]
    assert 0.8 <= b[0] / b[1] <= 1.25, b        # (tiles hold equal numbers of blocks: the ranks' shares are even)


def _api_worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from sparse_gslam_amd import capi
        g = _graph("C2")
        with capi.Optimizer(0, pcg_tol=1e-10) as o:
            o.comm_init_host(world, rank, lambda a: dist.all_reduce(torch.from_numpy(a)))
            o.set_graph(*g.arrays())
            b, diag, c2, rc2 = o.linearize()
            x = np.random.default_rng(3).standard_normal(b.shape)
            y = o.hessian_apply(x)
            z = o.precondition(x)
            sol, its, relres = o.solve()
            e2 = o.edge_chi2()
            desc = o.solver_description()
        q.put((rank, b.tobytes(), diag.tobytes(), c2, rc2, y.tobytes(), z.tobytes(), sol.tobytes(), its, e2.tobytes(), desc))
    except Exception as e:
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


def test_single_step_entry_points_in_row_owner_mode():
    """sgo_linearize / sgo_hessian_apply / sgo_precondition / sgo_solve / sgo_edge_chi2 with two rank processes in row-owner
    mode: every rank reports the FULL vectors (the ranks' slices are gathered at the boundary), identical on both ranks, and
    equal to the single-GPU results to rounding (1e-9 for the solve: two PCG runs to 1e-10)."""
    import torch.multiprocessing as mp
    from sparse_gslam_amd import capi
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_api_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert all(len(r) == 11 for r in res), res
    assert "row-owner mode" in res[0][10]
    for k in (1, 2, 5, 6, 7, 9):
        assert res[0][k] == res[1][k], k          # bit-identical on the two ranks
    g = _graph("C2")
    with capi.Optimizer(0, pcg_tol=1e-10) as o:
        o.set_graph(*g.arrays())
        b, diag, c2, rc2 = o.linearize()
        x = np.random.default_rng(3).standard_normal(b.shape)
        y = o.hessian_apply(x)
        z = o.precondition(x)
        sol, its, relres = o.solve()
        e2 = o.edge_chi2()
    f = lambda k, shape: np.frombuffer(res[0][k], dtype=np.float64).reshape(shape)   # noqa: E731
    assert np.abs(f(1, b.shape) - b).max() <= 1e-12 * np.abs(b).max()
    assert np.abs(f(2, diag.shape) - diag).max() <= 1e-12 * np.abs(diag).max()
    assert abs(res[0][3] - c2) <= 1e-12 * c2 and abs(res[0][4] - rc2) <= 1e-12 * rc2
    assert np.abs(f(5, y.shape) - y).max() <= 1e-12 * np.abs(y).max()     # (another tile cut: rounding)
    assert np.abs(f(6, z.shape) - z).max() <= 1e-6 * np.abs(z).max()      # (fp32 blocks inside the preconditioner, other tiles)
    assert np.abs(f(7, sol.shape) - sol).max() <= 1e-8 * np.abs(sol).max()
    assert np.array_equal(f(9, e2.shape), e2)


def test_hierarchy_rebuild_inside_optimize_in_row_owner_mode(monkeypatch):
    """The stale-aggregation rule (counts only: every rank decides alike) redoes the multigrid set-up inside optimize() with
    two rank processes in row-owner mode (forced: the graph's random closures would pick the all-reduce mode): ranks
    bit-identical, iterates within the parity bound of the single-GPU run, which rebuilds at the same iterations."""
    from sparse_gslam_amd import capi
    monkeypatch.setenv("SGO_COMM_MODE", "owner")
    res = _run(2, "rebuild", 20)
    assert all(r[1] == 20 for r in res), [r[:3] for r in res]
    assert "row-owner mode" in res[0][8]
    assert res[0][2] == res[1][2] and res[0][3] == res[1][3] and res[0][4] == res[1][4]
    monkeypatch.delenv("SGO_COMM_MODE")
    g = _graph("rebuild")
    with capi.Optimizer(0, direct_rows=0) as o:
        o.set_graph(*g.arrays())
        d, st = o.optimize(20)
    assert d == 20
    for a, b in zip(res[0][2], st["chi2"]):
        assert abs(a - b) <= 1e-6 * b
    assert max(res[0][3]) < 400        # no solve ground on with a stale hierarchy


def test_fewer_tiles_than_ranks_runs_replicated():
    """A graph whose level-0 plan has fewer tiles than ranks would leave a rank an empty range, which the level-0 kernels and
    the transfers read as "everything" (u1 == 0 / row1 == 0): out-of-bounds reads in row-owner mode, double-counted coarse
    right-hand sides in all-reduce mode.  Such graphs run replicated -- every rank the whole single-GPU computation, no
    collective inside the solve: ranks bit-identical, and equal to the single-GPU path to rounding (that one multiplies through
    the wave-group kernel, the ranks through the tile kernel)."""
    from sparse_gslam_amd import capi
    g = _graph("tiny")
    plan = capi.plan_rows(g.poses, g.fixed, g.ei, g.ej, nranks=3)
    assert len(plan["tile_row_begin"]) - 1 < 3          # the premise: fewer tiles than ranks
    res = _run(3, "tiny", 5)
    assert all(r[1] == 5 for r in res), [r[:3] for r in res]
    assert "replicated" in res[0][8], res[0][8]
    for r in res[1:]:
        assert r[2] == res[0][2] and r[3] == res[0][3] and r[4] == res[0][4]
    with capi.Optimizer(0, direct_rows=0) as o:        # the multigrid-PCG path the ranks ran (a communicator rules the direct path out)
        o.set_graph(*g.arrays())
        d, st = o.optimize(5)
        P = o.get_poses()
    assert d == 5
    assert np.abs(np.frombuffer(res[0][4], dtype=np.float64).reshape(-1, 3) - P).max() <= 1e-9
    for a, b in zip(res[0][2], st["chi2"]):
        assert abs(a - b) <= 1e-9 * b


def test_bench_gpus_2_runs_end_to_end_over_the_host_transport():
    """`bench.py --gpus N` as the driver launches it (python -m torch.distributed.run, one process per rank, rendezvous on
    127.0.0.1), with --transport host: the rank processes share this box's one GPU and libsgo's collectives go through
    sgo_comm_init_host + gloo.  The whole launcher path runs -- rendezvous, every rank marshalling the graph, the library's
    choice of the sharding mode, barrier + MAX-reduce of the time, ONE JSON line from rank 0 -- and the final chi2 is within
    BASELINE.json's 1e-6 of the direct-solver golden.  (A functional run: the line's `transport` says it is no scaling figure.)"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1",
           "--config", "C2", "--transport", "host", "--full", "--no-cpu-baseline", "--no-roofline"]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout          # rank 0 alone prints
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 1 and out["scaling"] == "strong"
    assert out["metric"].startswith("edge-Jacobians/sec per GN iter")
    assert "row-owner mode" in out["config"]["parallelism"] or "all-reduce mode" in out["config"]["parallelism"], out["config"]
    assert out["config"]["transport"].startswith("host")
    assert out["value"] > 0 and out["ms_per_step"] > 0
    err = out["final_chi2_rel_err_vs_oracle"]
    assert err is not None and err["value"] <= 1e-6, err
