"""The host restatement of the preconditioner (tests/precond_reference.py), judged before it judges the device: its Chebyshev recurrence is
the shifted and scaled Chebyshev polynomial, its restriction is its prolongation transposed, and the whole cycle it restates is
symmetric and positive definite -- on a small Kuhn box from the CPU oracle, aggregated by the product's own host aggregation."""
import numpy as np
import pytest
import scipy.linalg as sla

from mesheditor_amd import meshes
from tests import precond_reference as ref

SIGMA = -(2 * np.pi * 20.0) ** 2
SHAPES = {  # the product's three cycle shapes (mh_eigs.hip: mh_cycle_shape)
    "bulk": {"deg2": 2, "ratio": 8.0, "deg1": 12, "gamma": 1, "ratio1": 100.0},
    "surface": {"deg2": 5, "ratio": 60.0, "deg1": 16, "gamma": 1, "ratio1": 250.0},
    "patches": {"deg2": 5, "ratio": 60.0, "deg1": 5, "gamma": 3, "ratio1": 0.0},
}


@pytest.fixture(scope="module")
def box(oracle):
    from tools import lab
    pts, tets = meshes.kuhn_box(3, 3, 2, 0.1, 0.1, 0.06)
    s = oracle.System(pts, tets, oracle.material(*meshes.MATERIALS["Ceramic"]))
    en = s.element_nodes().astype(np.int64)
    A2 = ref.shifted_operator(s.full(0), s.full(1), SIGMA)
    npts, nn = len(pts), s.node_count
    P = ref.prolongation(en, nn, npts)
    A1 = (P.T @ A2 @ P).tocsr()
    rp, cl = ref.point_graph(en, npts)
    agg_of, nagg = lab.graph_aggregates(rp, cl, target=8)
    agg_of = agg_of.astype(np.int64)
    T = ref.rigid_body_t(ref.rigid_body_blocks(pts, agg_of, nagg), agg_of, nagg)
    # patches as the device forms them: two elements sharing nodes (weight 2^-0.35 each), one apart (weight 1); one cluster of two elements
    rows = lambda nodes: ref._node_rows(nodes)  # noqa: E731
    share = [e for e in range(1, len(en)) if len(set(en[0, :4]) & set(en[e, :4])) == 3][0]
    apart = [e for e in range(len(en)) if not set(en[e]) & (set(en[0]) | set(en[share]))][-1]
    w = 2.0 ** -0.35
    patches2 = [(rows(en[0]), w), (rows(en[share]), w), (rows(en[apart]), 1.0)]
    patches1 = [(rows(en[0, :4]), w), (rows(en[share, :4]), w), (rows(en[apart, :4]), 1.0)]
    return {"pts": pts, "en": en, "A2": A2, "A1": A1, "P": P, "T": T, "nagg": nagg, "agg_of": agg_of, "patches2": patches2, "patches1": patches1,
            "n_points": npts, "n_nodes": nn}


def _cycle(box, shape, patched):
    A2, A1, T = box["A2"], box["A1"], box["T"]
    M2inv = ref.smoother_scaling(A2, box["patches2"] if patched else ())
    M1inv = ref.smoother_scaling(A1, box["patches1"] if patched else ())
    lmax2, lmax1 = 1.1 * ref.spectral_radius(A2, M2inv), 1.1 * ref.spectral_radius(A1, M1inv)
    a0inv = np.linalg.inv(ref.coarse_operator(A1, T, 1e-12))
    return ref.Cycle(A2, M2inv, lmax2, box["P"], A1, M1inv, lmax1, T, 0.5 * (a0inv + a0inv.T), shape)


@pytest.mark.parametrize("deg,ratio", [(1, 8.0), (2, 8.0), (5, 60.0), (12, 100.0), (16, 250.0), (28, 800.0)])
def test_chebyshev_recurrence_is_the_shifted_chebyshev_polynomial(deg, ratio):
    """On a diagonal operator, 1 - lam q(lam) of the recurrence from zero equals T_deg((theta - lam) / delta) / T_deg(theta / delta) on and
    below the interval, and a start from x0 adds exactly the recurrence's answer for the residual b - A x0."""
    import scipy.sparse as sp
    lmax = 3.7
    lam = np.concatenate([np.linspace(0.0, lmax, 401), lmax * np.logspace(-6, 0, 61)])
    A, Id = sp.diags(lam), sp.identity(len(lam), format="csr")
    b = np.ones((len(lam), 1))
    x = ref.chebyshev(A, Id, b, None, deg, lmax, ratio)[:, 0]
    want = ref.chebyshev_error_polynomial(lam, deg, lmax, ratio)
    assert np.abs((1 - lam * x) - want).max() < 1e-12, np.abs((1 - lam * x) - want).max()
    assert np.abs(want[lam >= lmax / ratio]).max() <= 1.0 / np.cosh(deg * np.arccosh((ratio + 1) / (ratio - 1))) * (1 + 1e-9)
    rng = np.random.default_rng(deg)
    x0 = rng.standard_normal((len(lam), 1))
    got = ref.chebyshev(A, Id, b, x0, deg, lmax, ratio)
    assert np.allclose(got, x0 + ref.chebyshev(A, Id, b - A @ x0, None, deg, lmax, ratio), rtol=0, atol=1e-12)


def test_chebyshev_recurrence_with_the_patched_scaling(box):
    """The same identity through the generalised eigenvectors of (A2, M): the error e - x of the recurrence for b = A2 e from zero is
    V diag(T_deg(...) / T_deg(...)) V^T M e, with the overlapping, weighted patches in M^-1."""
    A2 = box["A2"]
    Minv = ref.smoother_scaling(A2, box["patches2"])
    Md = np.linalg.inv(Minv.toarray())
    lam, V = sla.eigh(A2.toarray(), 0.5 * (Md + Md.T))
    lmax = 1.05 * lam[-1]
    e = np.random.default_rng(3).standard_normal((A2.shape[0], 2))
    for deg, ratio in ((2, 8.0), (5, 60.0)):
        x = ref.chebyshev(A2, Minv, A2 @ e, None, deg, lmax, ratio)
        want = V @ (ref.chebyshev_error_polynomial(lam, deg, lmax, ratio)[:, None] * (V.T @ (Md @ e)))
        assert np.abs((e - x) - want).max() < 1e-9 * np.abs(e).max(), (deg, np.abs((e - x) - want).max())


def test_restriction_is_prolongation_transposed(box):
    """k_restrict_p1's form (corner plus half of every incident midside node) is P^T of k_prolong_p1's form, entry for entry; P carries a
    linear field on the points to the same field on the quadratic nodes; the rigid-body columns of T are unit columns of aggregates."""
    en, nn, npts, P = box["en"], box["n_nodes"], box["n_points"], box["P"]
    pa, pb = ref.midside_parents(en, nn)
    Pd = P.toarray()
    assert np.array_equal(ref.prolong_p1(np.eye(3 * npts), pa, pb), Pd)
    assert np.array_equal(ref.restrict_p1(np.eye(3 * nn), pa, pb, npts), Pd.T)
    xyz = 0.5 * (box["pts"][pa] + box["pts"][pb])  # quadratic node positions: corners, and edge midpoints
    g = np.array([[1.0, -2.0, 0.5], [0.25, 3.0, -1.0], [2.0, 0.0, 1.5]])
    u1 = (box["pts"] @ g.T + np.array([0.1, -0.2, 0.3])).reshape(-1, 1)
    u2 = (xyz @ g.T + np.array([0.1, -0.2, 0.3])).reshape(-1, 1)
    assert np.abs(P @ u1 - u2).max() < 1e-15 * np.abs(u2).max() * 10
    T = box["T"]
    tt = (T.T @ T).toarray()
    assert np.allclose(np.diag(tt), 1.0, rtol=0, atol=1e-14)
    assert np.allclose(tt[np.arange(0, tt.shape[0], 6)][:, np.arange(0, tt.shape[0], 6)], np.eye(box["nagg"]), atol=1e-15)


@pytest.mark.parametrize("shape,patched", [("bulk", False), ("surface", False), ("patches", True)])
def test_restated_cycle_is_symmetric_positive_definite(box, shape, patched):
    """B formed densely from the restated cycle: symmetric to rounding, positive definite, and B A well conditioned."""
    cyc = _cycle(box, SHAPES[shape], patched)
    n = box["A2"].shape[0]
    B = cyc.apply(np.eye(n))
    asym = np.abs(B - B.T).max() / np.abs(B).max()
    # (exactly symmetric; three P1 cycles form r1 - A1 x1 three times, and cond(A1) = 5e7 here carries that rounding into B: 4e-10 measured)
    assert asym < (1e-12 if SHAPES[shape]["gamma"] == 1 else 2e-9), asym
    Bs = 0.5 * (B + B.T)
    w = np.linalg.eigvalsh(Bs)
    assert w[0] > 0, w[:3]
    mu = sla.eigh(box["A2"].toarray(), np.linalg.inv(Bs), eigvals_only=True)  # eigenvalues of B A
    assert mu[0] > 0 and mu[-1] / mu[0] < 50, (mu[0], mu[-1])
