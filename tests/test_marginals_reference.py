"""The reference of the marginal-covariance tests (tests/marginals_reference.py) against numpy.linalg.inv of the dense Hessian on
tests/golden/tiny_full.npz: 1e-9 on the natural scale of every block, the zero-block rule for the fixed vertex, the
symmetrisation of diagonal blocks, and the unit columns' own residuals."""
import os

import numpy as np

import marginals_reference as mr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_full.npz")


def _tiny():
    z = np.load(GOLDEN)
    g = tuple(z[k] for k in ("fixed", "ei", "ej", "meas", "info", "phi"))
    return z["poses_iter1"], g


def test_blocks_agree_with_the_dense_inverse():
    P, g = _tiny()
    fixed = g[0]
    H = mr.hessian(P, *g)
    ref = mr.Reference(H, fixed)
    inv = np.linalg.inv(H.toarray())
    V = fixed.size
    vs = [1, V // 2, V - 1, 17]
    vi = np.array([a for a in vs for _ in vs])
    vj = np.array([b for _ in vs for b in vs])
    got = ref.blocks(vi, vj)
    worst = 0.0
    for t, (i, j) in enumerate(zip(vi, vj)):
        hi, hj = int(ref.hidx[i]), int(ref.hidx[j])
        D = inv[3 * hi:3 * hi + 3, 3 * hj:3 * hj + 3]
        scale = np.sqrt(np.abs(inv[3 * hi:3 * hi + 3, 3 * hi:3 * hi + 3]).max() * np.abs(inv[3 * hj:3 * hj + 3, 3 * hj:3 * hj + 3]).max())
        assert abs(ref.scale(i, j) - scale) <= 1e-9 * scale
        worst = max(worst, np.abs(got[t] - D).max() / scale)
        if i == j:
            assert np.array_equal(got[t], got[t].T) and np.all(np.linalg.eigvalsh(got[t]) > 0)
    print("worst |ref - inv| / natural scale", worst, "worst unit-column residual", ref.worst_residual)
    assert worst <= 1e-9
    assert ref.worst_residual <= 1e-9
    # H^-1 is symmetric: blocks from different solves are each other's transposes to the same bar
    a, b = ref.block(1, V - 1), ref.block(V - 1, 1)
    assert np.abs(a - b.T).max() <= 1e-9 * ref.scale(1, V - 1)


def test_a_fixed_vertex_gives_zero_blocks_and_costs_no_column():
    P, g = _tiny()
    fixed = g[0]
    assert fixed[0] and not fixed[1:].any()
    ref = mr.Reference(mr.hessian(P, *g), fixed)
    for i, j in ((0, 5), (5, 0), (0, 0)):
        assert np.array_equal(ref.block(i, j), np.zeros((3, 3)))
    assert not ref._cols and ref.scale(0, 5) == 0.0
    assert mr.worst_ratio(np.zeros((1, 3, 3)), ref, [0], [5]) == 0.0


def test_weights_are_in_the_hessian():
    """Another kind on the closures, and a zero information row, change H as the pre-scaled information says."""
    P, g = _tiny()
    fixed, ei, ej, meas, info, phi = g
    w = mr.weights(P, ei, ej, meas, info, phi)
    assert np.all(w[phi < 0] == 1.0) and (w[phi >= 0] < 1.0).any()
    kind = np.where(phi >= 0, mr.rr.HUBER, mr.rr.NONE)
    wh = mr.weights(P, ei, ej, meas, info, phi, kind, np.full(phi.size, 1.5))
    assert not np.array_equal(w, wh)
    dead = info.copy()
    k = int(np.flatnonzero(phi >= 0)[0])
    dead[k] = 0.0
    H0, H1 = mr.hessian(P, *g), mr.hessian(P, fixed, ei, ej, meas, dead, phi)
    assert abs(H0 - H1).max() > 0
    assert mr.weights(P, ei, ej, meas, dead, phi)[k] == 1.0
