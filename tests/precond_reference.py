"""The eigensolver's preconditioner B (mh_eigs.hip: Precond) restated on the host in float64 (numpy + scipy).

Built from data the device did not compute where that is possible: the shifted operator A2 = K - sigma M, the element node lists, the
mesh points and the aggregates.  What only the device knows -- the P1 operator it assembled, the patch node lists and weights, the
spectral bounds -- comes in from the lab export and is judged on its own before it is used (tests/test_preconditioner_gpu.py).

Panels are dense (n x w) arrays in the reference's DOF order: node q owns rows 3 q .. 3 q + 2; mesh points are the first P2 nodes."""
import numpy as np
import scipy.sparse as sp

EDGE_CORNERS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))  # oracle/analysis.cpp: midside node 4 + e between these corners


def shifted_operator(K, M, sigma):
    """A = K - sigma M (CSR)."""
    return (K - sigma * M).tocsr()


def _node_rows(nodes):
    """DOF rows of a node list, node-major (3 a + k): the local order of the device's patch blocks."""
    nodes = np.asarray(nodes, np.int64)
    return (3 * nodes[:, None] + np.arange(3)[None, :]).ravel()


# ---- P2 <-> P1 transfers ---------------------------------------------------------------------------------------------------
def midside_parents(element_nodes, n_nodes):
    """(parent_a, parent_b) of every P2 node: a corner is its own parent (both), midside node 4 + e has the two corners of edge e."""
    en = np.asarray(element_nodes, np.int64)
    pa, pb = np.full(n_nodes, -1, np.int64), np.full(n_nodes, -1, np.int64)
    for c in range(4):
        pa[en[:, c]] = en[:, c]
        pb[en[:, c]] = en[:, c]
    for e, (i, j) in enumerate(EDGE_CORNERS):
        pa[en[:, 4 + e]] = en[:, i]
        pb[en[:, 4 + e]] = en[:, j]
    assert (pa >= 0).all(), "a P2 node in no element"
    return pa, pb


def prolongation(element_nodes, n_nodes, n_points):
    """P (3 n_nodes x 3 n_points, CSR): a corner takes its point's value, a midside node half of each parent's."""
    pa, pb = midside_parents(element_nodes, n_nodes)
    rows = np.concatenate([np.arange(n_nodes), np.arange(n_nodes)])
    cols = np.concatenate([pa, pb])
    vals = np.full(2 * n_nodes, 0.5)  # (a corner: 0.5 + 0.5 on its own point)
    Pn = sp.coo_matrix((vals, (rows, cols)), shape=(n_nodes, n_points)).tocsr()
    return sp.kron(Pn, sp.identity(3), format="csr")


def prolong_p1(x1, pa, pb):
    """x2 = P x1 as k_prolong_p1 forms it: corner rows copy, midside rows average their parents."""
    x1 = x1.reshape(-1, 3, x1.shape[-1])
    out = np.where((pa == pb)[:, None, None], x1[pa], 0.5 * (x1[pa] + x1[pb]))
    return out.reshape(-1, out.shape[-1])


def restrict_p1(r2, pa, pb, n_points):
    """r1 = P^T r2 as k_restrict_p1 forms it: a point's own value plus half of every midside node on one of its edges."""
    r = r2.reshape(-1, 3, r2.shape[-1])
    out = np.zeros((n_points, 3, r2.shape[-1]))
    corner = pa == pb
    np.add.at(out, pa[corner], r[corner])
    mid = ~corner
    np.add.at(out, pa[mid], 0.5 * r[mid])
    np.add.at(out, pb[mid], 0.5 * r[mid])
    return out.reshape(-1, r2.shape[-1])


# ---- level 0 ----------------------------------------------------------------------------------------------------------------
def point_graph(element_nodes, n_points):
    """CSR (row_ptr, col) of the mesh points' graph with the diagonal: the P1 operator's node-block pattern."""
    en = np.asarray(element_nodes, np.int64)[:, :4]
    r = np.repeat(en, 4, axis=1).ravel()
    c = np.tile(en, (1, 4)).ravel()
    g = sp.coo_matrix((np.ones(len(r)), (r, c)), shape=(n_points, n_points)).tocsr()
    g.sum_duplicates()
    g.sort_indices()
    return g.indptr.astype(np.uint32), g.indices.astype(np.uint32)


def rigid_body_blocks(points, agg_of, n_agg):
    """Per point its 3 x 6 block of T, as k_aggregate_t forms it: translations scaled by 1 / sqrt(aggregate size), rotations e_q x (x - c)
    about the aggregate's centroid, each column scaled to unit norm over the aggregate (0 where it vanishes)."""
    pts = np.asarray(points, np.float64)
    agg_of = np.asarray(agg_of, np.int64)
    cnt = np.bincount(agg_of, minlength=n_agg).astype(np.float64)
    cen = np.stack([np.bincount(agg_of, pts[:, d], minlength=n_agg) for d in range(3)], 1) / cnt[:, None]
    rel = pts - cen[agg_of]
    rx, ry, rz = rel[:, 0], rel[:, 1], rel[:, 2]
    rn = np.stack([np.bincount(agg_of, ry * ry + rz * rz, minlength=n_agg), np.bincount(agg_of, rx * rx + rz * rz, minlength=n_agg),
                   np.bincount(agg_of, rx * rx + ry * ry, minlength=n_agg)], 1)
    sr = np.where(rn > 1e-300, 1.0 / np.sqrt(np.where(rn > 1e-300, rn, 1.0)), 0.0)[agg_of]
    st = 1.0 / np.sqrt(cnt[agg_of])
    t = np.zeros((len(pts), 3, 6))
    for p in range(3):
        t[:, p, p] = st
    t[:, 1, 3], t[:, 2, 3] = -rz * sr[:, 0], ry * sr[:, 0]
    t[:, 0, 4], t[:, 2, 4] = rz * sr[:, 1], -rx * sr[:, 1]
    t[:, 0, 5], t[:, 1, 5] = -ry * sr[:, 2], rx * sr[:, 2]
    return t


def rigid_body_t(blocks, agg_of, n_agg):
    """T (3 n_points x 6 n_agg, CSR) from the per-point blocks."""
    npts = len(agg_of)
    rows = np.repeat(3 * np.arange(npts)[:, None] + np.arange(3)[None, :], 6, axis=1).reshape(npts, 3, 6)
    cols = 6 * np.asarray(agg_of, np.int64)[:, None, None] + np.arange(6)[None, None, :] + 0 * rows
    return sp.coo_matrix((blocks.ravel(), (rows.ravel(), cols.ravel())), shape=(3 * npts, 6 * n_agg)).tocsr()


def p1_operator(l1_row, l1_col, l1_val, n_points):
    """The P1 operator from node blocks (reference point ids, 3 x 3 row-major values), CSR."""
    rows = 3 * l1_row[:, None, None] + np.arange(3)[None, :, None] + 0 * np.arange(3)[None, None, :]
    cols = 3 * l1_col[:, None, None] + np.arange(3)[None, None, :] + 0 * np.arange(3)[None, :, None]
    return sp.coo_matrix((l1_val.ravel(), (rows.ravel(), cols.ravel())), shape=(3 * n_points, 3 * n_points)).tocsr()


def coarse_operator(A1, T, lift):
    """A0 = T^T A1 T (dense) with k_fix_coarse_diag's lift: a positive diagonal entry times (1 + lift), an empty one set to 1."""
    a0 = np.asarray((T.T @ (A1 @ T)).todense())
    d = np.diag(a0).copy()
    np.fill_diagonal(a0, np.where(d > 0, d * (1.0 + lift), 1.0))
    return a0


# ---- smoothers --------------------------------------------------------------------------------------------------------------
def patch_inverses(A, patches):
    """w_e inv(A[e, e]) for every (dof rows, weight) of `patches`."""
    out = []
    for rows, w in patches:
        out.append(w * np.linalg.inv(A[rows][:, rows].toarray()))
    return out


def smoother_scaling(A, patches=(), clusters=(), inverses=None):
    """M^-1 = D^-1 + sum_e w_e R_e^T inv(A_ee) R_e + sum_c R_c^T inv(A_cc) R_c (CSR), the smoothers' scaling (mh_patch.hip).  patches:
    (dof rows, weight); clusters: dof rows; inverses: the weighted patch inverses, then the cluster inverses, when given (else formed here)."""
    n = A.shape[0]
    parts = [sp.diags(1.0 / A.diagonal())]
    blocks = list(patches) + [(rows, 1.0) for rows in clusters]
    if blocks:
        r, c, v = [], [], []
        for (rows, _), inv in zip(blocks, patch_inverses(A, blocks) if inverses is None else inverses):
            r.append(np.repeat(rows, len(rows)))
            c.append(np.tile(rows, len(rows)))
            v.append(inv.ravel())
        parts.append(sp.coo_matrix((np.concatenate(v), (np.concatenate(r), np.concatenate(c))), shape=(n, n)))
    return sum(parts[1:], parts[0]).tocsr()


def chebyshev(A, Minv, b, x, deg, lmax, ratio):
    """deg Chebyshev steps for A x = b scaled by Minv over [lmax / ratio, lmax], from x (None: zero), as Precond::cheb runs them."""
    lmin = lmax / ratio
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    sig = theta / delta
    rho = 1.0 / sig
    r = b.copy() if x is None else b - A @ x
    d = (Minv @ r) / theta
    x = d.copy() if x is None else x + d
    for _ in range(1, deg):
        rho_new = 1.0 / (2 * sig - rho)
        r = r - A @ d
        d = rho_new * rho * d + (2 * rho_new / delta) * (Minv @ r)
        x = x + d
        rho = rho_new
    return x


def chebyshev_error_polynomial(lam, deg, lmax, ratio):
    """1 - lam q(lam) of `chebyshev` from zero: T_deg((theta - lam) / delta) / T_deg(theta / delta) (numpy.polynomial.chebyshev)."""
    from numpy.polynomial import chebyshev as ch
    lmin = lmax / ratio
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    c = np.zeros(deg + 1)
    c[deg] = 1.0
    return ch.chebval((theta - np.asarray(lam)) / delta, c) / ch.chebval(theta / delta, c)


class Cycle:
    """B restated as Precond::apply runs it: pre-smoothing on L2; r1 = P^T (r - A2 z); gamma times (smoothing on L1 -- from zero the first
    time --, coarse correction x1 += T a0inv T^T (r1 - A1 x1), smoothing on L1); z += P x1; post-smoothing on L2.  shape: deg2, ratio,
    deg1, gamma, ratio1 (0: the L1 level takes `ratio` too)."""

    def __init__(self, A2, M2inv, lmax2, P, A1, M1inv, lmax1, T, a0inv, shape):
        self.A2, self.M2inv, self.lmax2, self.P, self.A1, self.M1inv, self.lmax1, self.T, self.a0inv = A2, M2inv, lmax2, P, A1, M1inv, lmax1, T, a0inv
        self.deg2, self.ratio, self.deg1, self.gamma = shape["deg2"], shape["ratio"], shape["deg1"], shape["gamma"]
        self.ratio1 = shape["ratio1"] if shape["ratio1"] > 0 else shape["ratio"]

    def apply(self, r):
        r = np.asarray(r, np.float64)
        vec = r.ndim == 1
        if vec:
            r = r[:, None]
        z = chebyshev(self.A2, self.M2inv, r, None, self.deg2, self.lmax2, self.ratio)
        r1 = self.P.T @ (r - self.A2 @ z)
        x1 = None
        for _ in range(self.gamma):
            x1 = chebyshev(self.A1, self.M1inv, r1, x1, self.deg1, self.lmax1, self.ratio1)
            r0 = self.T.T @ (r1 - self.A1 @ x1)
            x1 = x1 + self.T @ (self.a0inv @ r0)
            x1 = chebyshev(self.A1, self.M1inv, r1, x1, self.deg1, self.lmax1, self.ratio1)
        z = z + self.P @ x1
        z = chebyshev(self.A2, self.M2inv, r, z, self.deg2, self.lmax2, self.ratio)
        return z[:, 0] if vec else z


def spectral_radius(A, Minv, tol=1e-10):
    """lambda_max(M^-1 A) for SPD A and M^-1 (the generalised problem A x = lambda M x, M = (M^-1)^-1, by ARPACK)."""
    from scipy.sparse.linalg import LinearOperator, eigsh, splu
    n = A.shape[0]
    lu = splu(Minv.tocsc())
    Mop = LinearOperator((n, n), matvec=lambda v: lu.solve(np.asarray(v, np.float64).ravel()), dtype=np.float64)
    Mi = LinearOperator((n, n), matvec=lambda v: Minv @ np.asarray(v, np.float64).ravel(), dtype=np.float64)
    w = eigsh(A, k=1, M=Mop, Minv=Mi, which="LA", tol=tol, return_eigenvectors=False, v0=np.ones(n))
    return float(w[0])
