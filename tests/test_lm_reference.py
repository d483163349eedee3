"""tests/lm_reference.py, the numpy statement of sgo_optimize_lm's schedule, against oracle/np_lm_oracle.py::levenberg -- the
statement the landmark path is tested with -- on a pose-only graph: 12 poses, the odometry chain and 3 closures, seven iterations
from a start perturbed far enough that the first and the third iteration reject trials ([3, 1, 2, 1, 1, 1, 1]).  The oracle
linearises with g2o's numeric Jacobians (central differences, delta = 1e-9), the reference with the analytic ones: the lambda
traces agree within the 1e-6 (relative) that file's docstring states.  The information is scaled by 1e-4 so that the 1e-3 of the
gain ratio's denominator is not negligible beside x . (lambda x + b).  A reference with one constant changed misses the same
comparison: the comparison, and so the GPU test built on the reference, notices each of them."""
import numpy as np
import pytest

import lm_reference as lr
from oracle import np_lm_oracle, np_oracle
from sparse_gslam_amd import synth

ITERS = 7
LAMBDA_RTOL = 1e-6


@pytest.fixture(scope="module")
def case():
    g = synth.manhattan(12, 14, seed=21, info_mode="full", init="odom")
    g.phi[:] = -1.0
    g.info = g.info * 1e-4
    start = lr.perturbed(g, 4.0)
    G = np_lm_oracle.Graph()
    for v in range(g.V):
        G.v[v] = dict(kind="pose", est=start[v].copy(), fixed=bool(g.fixed[v]))
    O = np_oracle.info_full(g.info)
    for k in range(g.E):
        G.e.append(dict(kind="odom", vi=int(g.ei[k]), vj=int(g.ej[k]), z=g.meas[k].copy(), info=O[k]))
    done, trace = np_lm_oracle.levenberg(G, ITERS)
    assert done == ITERS
    return g, start, trace


def run(case, **constants):
    g, start, _ = case
    return lr.levenberg(start, g.fixed, g.ei, g.ej, g.meas, g.info, g.phi, ITERS, **constants)


def agrees(ref, trace):
    if ref["iters_done"] != len(trace) or ref["trials"] != [t[2] for t in trace]:
        return False
    return all(abs(a - t[0]) <= LAMBDA_RTOL * t[0] for a, t in zip(ref["lam"], trace))


def test_reference_reproduces_the_landmark_oracle(case):
    ref = run(case)
    trace = case[2]
    assert ref["trials"] == [3, 1, 2, 1, 1, 1, 1] and ref["stop_reason"] == lr.STOP_MAX_ITERS
    assert ref["trials"] == [t[2] for t in trace]
    dev = max(abs(a - t[0]) / t[0] for a, t in zip(ref["lam"], trace))
    print("worst relative lambda deviation", dev)
    assert agrees(ref, trace), dev
    # chi2: the oracle's numeric Jacobians move the iterates by 1e-6 or so
    assert np.allclose(ref["robust_chi2"][1:], [t[1] for t in trace], rtol=1e-4, atol=0.0)
    # the trace's own bookkeeping
    assert len(ref["records"]) == sum(ref["trials"]) and ref["lambda0"] == ref["records"][0]["lam"]
    assert all(a >= b for a, b in zip(ref["robust_chi2"], ref["robust_chi2"][1:]))
    assert ref["chi2"] == ref["robust_chi2"]   # no kernel


@pytest.mark.parametrize("constants", [dict(upper=0.5), dict(eps=0.0), dict(reset_nu=False)], ids=["two_thirds_to_half", "no_1e-3", "nu_not_reset"])
def test_a_mutated_constant_is_noticed(case, constants):
    assert not agrees(run(case, **constants), case[2])
