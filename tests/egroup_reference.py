"""The leave-group-out statistic of sgo_edge_joint / sgo_edge_groups in numpy, by two routes that share
nothing but the edge arithmetic of loo_reference.Edges (e, A, B, Omega, w and the robustified H they make):

  closed form   N = 1/2 (Q + Q^T), Q = J H^-1 J^T from sparse solves with the FULL graph's H, then, in fp64 numpy,
                K = I + Nt - D Nt - Nt D - Nt D (I - D) Nt with Nt = G^T N G, d2 = c^T K^-1 c, pivot = the smallest squared diagonal
                entry of chol(I - T Nt T);
  explicit      the group is taken out, in np.longdouble: H_ = H - J^T (D Omega) J is factorised (SuperLU in fp64, refined with
                long-double residuals until the correction vanishes), e~ = e + J H_^-1 J^T D Omega e, P_ = J H_^-1 J^T,
                d2 = e~^T (Omega^-1 + P_)^-1 e~ by a long-double Cholesky.  The same refinement against the full H gives N, and from
                it pivot and K's condition number, in long double.

As in loo_reference the linear step is the one the removal CAUSES (the statistic is defined at b = 0)."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import loo_reference as lr
import mfront_cases as mc

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
MIN_PIVOT = 1e-3
CLUSTER = [306, 360, 361, 362]          # the four closures of cluster_graph that are wrong together
CHI2_99_DOF3, CHI2_99_DOF12 = 11.345, 26.22


def cluster_graph(shift=0.25, dcs=False):
    """loo_reference.motivating_graph's graph (300 poses, 360 edges) with closure 306 (poses 23 to 35) and three added closures
    (22 to 34, 24 to 36, 25 to 37) all shifted by `shift` in x and y -> (Case, CLUSTER).  dcs: the graph's own DCS on its closures, phi = 10 on the three added ones."""
    from sparse_gslam_amd import synth
    g = synth.manhattan(300, 360, seed=4, info_mode="full", init="incremental", tail=20)
    rng = np.random.default_rng(9)
    extra = [(22, 34), (24, 36), (25, 37)]
    ei = np.r_[g.ei, [a for a, _ in extra]].astype(np.int32)
    ej = np.r_[g.ej, [b for _, b in extra]].astype(np.int32)
    sig = np.array([synth.SIGMA_XY, synth.SIGMA_XY, synth.SIGMA_TH])
    m = synth._rel(g.truth[ei[360:]], g.truth[ej[360:]]) + rng.standard_normal((3, 3)) * sig
    meas = np.r_[g.meas, m]
    info = np.r_[g.info, np.tile([1 / sig[0]**2, 0, 0, 1 / sig[1]**2, 0, 1 / sig[2]**2], (3, 1))]
    meas[CLUSTER, :2] += shift
    phi = np.r_[g.phi, [10.0] * 3] if dcs else np.full(ei.size, -1.0)
    return mc.Case("cluster", g.poses.copy(), g.fixed.copy(), ei, ej, meas, info, phi), list(CLUSTER)


def info6(O):
    O = np.asarray(O)
    return np.stack([O[..., 0, 0], O[..., 0, 1], O[..., 0, 2], O[..., 1, 1], O[..., 1, 2], O[..., 2, 2]], axis=-1)


# ------------------------------------------------------------------ the table (fp64) and the closed form
def table(S: lr.Edges, edges):
    """-> dict(N (3 n, 3 n), e (n, 3), w (n,), O (n, 3, 3)) of the listed edges, as sgo_edge_joint exports them"""
    edges = np.asarray(edges, dtype=np.int64)
    n = edges.size
    N = np.zeros((3 * n, 3 * n))
    if S.n > 0 and n > 0:
        J = np.concatenate([S.J(k) for k in edges], axis=0)
        Q = J @ S.lu().solve(J.T)
        N = 0.5 * (Q + Q.T)
    return dict(N=N, e=S.e[edges].copy(), w=S.w[edges].copy(), O=S.O[edges].copy())


MUTATIONS = ("third_term_dropped", "no_transpose", "zero_information_kept", "w_ignored")


def closed_form(O, N, e, w, mutation=None):
    """One group from its rows of the table: O (k, 3, 3), N (3 k, 3 k), e (k, 3), w (k,) -> dict(d2, pivot, dof, and where they exist
    K's condition number condK and ||Nt||_2 normN).  A member with all-zero information is dropped; an information that is not positive definite gives NaN.  `mutation`: one of MUTATIONS, a
    wrong formula the tests must tell from the right one."""
    O, e, w = np.asarray(O, dtype=np.float64), np.asarray(e, dtype=np.float64), np.asarray(w, dtype=np.float64)
    keep = np.array([bool(o.any()) for o in O], dtype=bool)
    if mutation == "zero_information_kept":
        O = np.where(keep[:, None, None], O, 1e-300 * np.eye(3))
        keep[:] = True
    rows = np.repeat(keep, 3)
    O, e, w, N = O[keep], e[keep], w[keep], np.asarray(N)[np.ix_(rows, rows)]
    k = O.shape[0]
    if k == 0:
        return dict(d2=0.0, pivot=1.0, dof=0)
    if mutation == "w_ignored":
        w = np.ones(k)
    G = np.zeros((3 * k, 3 * k))
    try:
        for t in range(k):
            G[3 * t:3 * t + 3, 3 * t:3 * t + 3] = np.linalg.cholesky(O[t])
    except np.linalg.LinAlgError:
        return dict(d2=np.nan, pivot=np.nan, dof=3 * k)
    Nt = G.T @ (0.5 * (N + N.T)) @ G
    c = G.T @ e.reshape(-1)
    D = np.repeat(w, 3)
    I = np.eye(3 * k)
    T = np.sqrt(D)
    try:
        pivot = float((np.diag(np.linalg.cholesky(I - T[:, None] * Nt * T[None, :]))**2).min())
    except np.linalg.LinAlgError:
        return dict(d2=np.nan, pivot=0.0, dof=3 * k)
    K = I + Nt - D[:, None] * Nt - (0.0 if mutation == "no_transpose" else 1.0) * Nt * D[None, :]
    if mutation != "third_term_dropped":
        K = K - (Nt * (D * (1.0 - D))[None, :]) @ Nt
    if mutation == "no_transpose":
        d2 = float(c @ np.linalg.solve(K, c))
    else:
        try:
            z = np.linalg.solve(np.linalg.cholesky(0.5 * (K + K.T)), c)
            d2 = float(z @ z)
        except np.linalg.LinAlgError:
            d2 = np.nan
    ev = np.linalg.eigvalsh(0.5 * (K + K.T))
    return dict(d2=d2, pivot=pivot, dof=3 * k, condK=float(ev.max() / ev.min()) if ev.min() > 0 else np.inf,
                normN=float(np.abs(np.linalg.eigvalsh(0.5 * (Nt + Nt.T))).max()))


# ------------------------------------------------------------------ explicit removal in long double
def chol_ld(A):
    """lower Cholesky factor in long double; LinAlgError where a pivot is not above zero"""
    A = np.asarray(A, dtype=LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError(f"pivot {j} is {float(d):.3g}")
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def forward_ld(L, b):
    x = np.array(b, dtype=LD)
    for j in range(L.shape[0]):
        x[j] = (x[j] - L[j, :j] @ x[:j]) / L[j, j]
    return x


class Refined:
    """Solves with M = H - Jc^T W Jc in long double: H a sparse fp64 matrix (taken as exact), Jc (r, |cols|) and W (r, r) dense long
    double on the columns `cols` (None: M = H).  SuperLU factorises M rounded to fp64; every solve is refined with long-double
    residuals."""

    def __init__(self, H, Jc=None, W=None, cols=None):
        Hc = sp.coo_matrix(H)
        order = np.argsort(Hc.row, kind="stable")
        self.n = H.shape[0]
        self.row, self.col, self.val = Hc.row[order], Hc.col[order], Hc.data[order].astype(LD)
        self.start = np.flatnonzero(np.r_[True, self.row[1:] != self.row[:-1]])
        self.rows_present = self.row[self.start]
        self.Jc, self.W, self.cols = Jc, W, cols
        M = sp.csc_matrix(H)
        if Jc is not None:
            low = sp.coo_matrix(np.asarray(Jc.T @ W @ Jc, dtype=np.float64))
            M = (M - sp.coo_matrix((low.data, (cols[low.row], cols[low.col])), shape=H.shape)).tocsc()
        self.lu = spla.splu(M)

    def apply(self, X):
        Y = np.zeros((self.n, X.shape[1]), dtype=LD)
        if self.val.size:
            Y[self.rows_present] = np.add.reduceat(self.val[:, None] * X[self.col], self.start, axis=0)
        if self.Jc is not None:
            Y[self.cols] -= self.Jc.T @ (self.W @ (self.Jc @ X[self.cols]))
        return Y

    def solve(self, R, sweeps=6):
        R = np.asarray(R, dtype=LD)
        X = self.lu.solve(np.asarray(R, dtype=np.float64)).astype(LD)
        for _ in range(sweeps):
            dX = self.lu.solve(np.asarray(R - self.apply(X), dtype=np.float64)).astype(LD)
            X = X + dX
            if not np.abs(dX).max() > 1e-30 * np.abs(X).max():
                break
        self.last_correction = float(np.abs(dX).max() / max(float(np.abs(X).max()), 1e-300))
        return X


def _stack(S, ks):
    """the members with non-zero information: J restricted to its non-zero columns (long double), the columns, Omega, w, e"""
    ks = [k for k in ks if S.O[k].any()]
    J = np.concatenate([S.J(k) for k in ks], axis=0) if ks else np.zeros((0, 3 * S.n))
    cols = np.flatnonzero(np.abs(J).sum(axis=0) > 0) if ks else np.zeros(0, dtype=np.int64)
    r = 3 * len(ks)
    Om, D = np.zeros((r, r), dtype=LD), np.zeros(r, dtype=LD)
    for q, k in enumerate(ks):
        Om[3 * q:3 * q + 3, 3 * q:3 * q + 3] = S.O[k]
        D[3 * q:3 * q + 3] = S.w[k]
    e = np.concatenate([S.e[k] for k in ks]).astype(LD) if ks else np.zeros(0, dtype=LD)
    return ks, J[:, cols].astype(LD), cols, Om, D, e


def explicit(S: lr.Edges, ks):
    """The group taken out of the system, in long double -> dict(d2, dof).  LinAlgError where Omega^-1 + P_ is not positive
    definite; meant for groups whose removal leaves H_ well away from singular (the tests' usable groups)."""
    ks, Jc, cols, Om, D, e = _stack(S, ks)
    r = 3 * len(ks)
    if r == 0:
        return dict(d2=0.0, dof=0)
    W = D[:, None] * Om
    if S.n == 0 or cols.size == 0:
        Pm, et = np.zeros((r, r), dtype=LD), e
    else:
        R = np.zeros((3 * S.n, r + 1), dtype=LD)
        R[cols, :r] = Jc.T
        R[cols, r] = Jc.T @ (W @ e)
        X = Refined(S.H, Jc, W, cols).solve(R)
        Pm = Jc @ X[cols, :r]
        Pm = (Pm + Pm.T) / 2
        et = e + Jc @ X[cols, r]
    Oi = np.zeros((r, r), dtype=LD)
    for q in range(r // 3):
        Lq = chol_ld(Om[3 * q:3 * q + 3, 3 * q:3 * q + 3])
        Y = np.stack([forward_ld(Lq, col) for col in np.eye(3, dtype=LD)], axis=1)   # L^-1
        Oi[3 * q:3 * q + 3, 3 * q:3 * q + 3] = Y.T @ Y
    z = forward_ld(chol_ld(Oi + Pm), et)
    return dict(d2=float(z @ z), dof=r)


def reference_conditions(S: lr.Edges, ks, full=None):
    """pivot, ||Nt||_2 and the condition number of K from a long-double N -> dict(pivot, normN, condK, dof).  full: a Refined of the
    full H to share between groups."""
    ks, Jc, cols, Om, D, e = _stack(S, ks)
    r = 3 * len(ks)
    if r == 0:
        return dict(pivot=1.0, normN=0.0, condK=1.0, dof=0)
    N = np.zeros((r, r), dtype=LD)
    if S.n > 0 and cols.size:
        R = np.zeros((3 * S.n, r), dtype=LD)
        R[cols] = Jc.T
        X = (full or Refined(S.H)).solve(R)
        N = Jc @ X[cols]
        N = (N + N.T) / 2
    G = np.zeros((r, r), dtype=LD)
    for q in range(r // 3):
        G[3 * q:3 * q + 3, 3 * q:3 * q + 3] = chol_ld(Om[3 * q:3 * q + 3, 3 * q:3 * q + 3])
    Nt = G.T @ N @ G
    T = np.sqrt(D)
    I = np.eye(r, dtype=LD)
    try:
        pivot = float((np.diag(chol_ld(I - T[:, None] * Nt * T[None, :]))**2).min())
    except np.linalg.LinAlgError:
        pivot = 0.0
    K = I + Nt - D[:, None] * Nt - Nt * D[None, :] - (Nt * (D * (1 - D))[None, :]) @ Nt
    ev = np.linalg.eigvalsh(np.asarray(0.5 * (K + K.T), dtype=np.float64))
    return dict(pivot=pivot, normN=float(np.abs(np.linalg.eigvalsh(np.asarray(Nt, dtype=np.float64))).max()),
                condK=float(ev.max() / ev.min()) if ev.min() > 0 else np.inf, dof=r)


# ------------------------------------------------------------------ the groups the tests draw
SIZES = (1, 2, 5, 6, 11, 40)


def pool(S: lr.Edges):
    """the edges groups are drawn from: closures and in-loop odometry -- every edge with non-zero, positive definite information
    whose own leave-one-out redundancy is at least 1e-2 (a bridge's is 0)"""
    F = lr.by_formulas(S, np.arange(S.ei.size))
    return np.flatnonzero(np.nan_to_num(F["redundancy"], nan=0.0) >= 1e-2)


def loops(S: lr.Edges):
    """the cycle rank of the live graph with the fixed poses merged into one ground vertex: no more edges than this can leave
    together without disconnecting it"""
    live = np.array([bool(S.O[k].any()) and S.w[k] >= 1e-3 for k in range(S.ei.size)])
    verts = np.unique(np.r_[S.ei[live], S.ej[live]])
    free = int((~S.fixed[verts]).sum())
    return int(live.sum()) - free


def _stays_connected(S, live, removed):
    """every free pose still reaches a fixed one through live edges outside `removed` (union-find; structure only)"""
    parent = np.arange(S.fixed.size + 1)
    ground = S.fixed.size

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for v in np.flatnonzero(S.fixed):
        parent[find(v)] = find(ground)
    gone = set(int(k) for k in removed)
    for k in np.flatnonzero(live):
        if int(k) not in gone:
            parent[find(S.ei[k])] = find(S.ej[k])
    g = find(ground)
    return all(find(v) == g for k in removed for v in (S.ei[k], S.ej[k]))


def draw_groups(S: lr.Edges, seed, per_size=12, sizes=SIZES, tries=400):
    """-> list of sorted edge-id arrays, up to per_size of every size, drawn with a fixed seed from closures and in-loop odometry
    (pool): seven members in ten are closures where there are any (a group of 40 holds closures alone where the graph has that many:
    with a quarter of odometry it is a bridge nearly always); below 40 every other group comes from a window of neighbouring pool
    edges (clusters share poses: the cross blocks matter), the rest from the whole pool.  A member is taken only if the graph
    stays connected without the group so far (structure alone; whether a group is far enough from a bridge is the reference
    pivot's to say)."""
    rng = np.random.default_rng(seed)
    P = pool(S)
    live = np.array([bool(S.O[k].any()) and S.w[k] >= 1e-3 for k in range(S.ei.size)])
    closure = np.abs(S.ei - S.ej) != 1
    out = []
    for k in sizes:
        if P.size < k:
            continue
        for q in range(per_size):
            cand = P
            if q % 2 == 0 and P.size > 3 * k and k < 40:
                a = int(rng.integers(0, P.size - 3 * k + 1))
                cand = P[a:a + 3 * k]
            cl, od = cand[closure[cand]], cand[~closure[cand]]
            grp = []
            for _ in range(tries):
                if len(grp) == k:
                    break
                src = cl if (cl.size and (od.size == 0 or rng.random() < (1.0 if k >= 40 and cl.size >= k else 0.7))) else od
                e = int(src[rng.integers(0, src.size)])
                if e in grp or (live[e] and not _stays_connected(S, live, grp + [e])):
                    continue
                grp.append(e)
            if len(grp) == k:
                out.append(np.sort(np.array(grp, dtype=np.int64)))
    return out
