"""The Rayleigh-Ritz step stage by stage against extended precision (tests/rr_reference.py): the partial-spectrum kernels
(k_tridiag_values, k_tridiag_lowest; k_tridiag_invit, the Cholesky-QR and k_tridiag_residual of the wide form) on tridiagonal matrices
where such kernels go wrong, and the whole step (mh_rr_solve: standard form, the solver chosen by order, k_apply_q, back-transformation)
on pencils shaped like the solver's own, each case pinned to the branch it is meant to reach."""
import struct
from pathlib import Path

import numpy as np
import pytest

from tests import rr_reference as ref
from tools import lab

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
LDS_DOUBLES = 16896  # mh_tridiag_lowest declines when m k exceeds this (158 KB of LDS less the kernel's 7 * 256 + 1536 fixed doubles)


@pytest.fixture(scope="module")
def ctx():
    from mesheditor_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _golden():
    raw = (Path(__file__).parent / "golden" / "rr_matrix_order80.bin").read_bytes()
    m = struct.unpack("I", raw[:4])[0]
    a = np.frombuffer(raw[4:], dtype=np.float64).reshape(m, m)
    return 0.5 * (a + a.T)


# ---- partial spectrum -------------------------------------------------------------------------------------------------------
def _largest_k(m):
    return min(m - 1, 128, LDS_DOUBLES // m) if m > 2 else 1


def _check_lowest(ctx, d, e, k, repeats=1, want=None):
    """One call judged against the long-double reference, then `repeats` more that must be bit-identical to it."""
    m = len(d)
    w, z, q, taken = lab.tridiag_lowest(ctx, d, e, k)
    assert taken, (m, k)
    scale = ref.tnorm(d, e)
    floor = 8 * np.finfo(float).tiny  # (the zero matrix: the kernels' pivot floor keeps values and residuals off exact zero)
    if want is None:
        want = ref.tridiag_lowest_values(d, e, k).astype(float)
    assert np.all(np.diff(w) >= 0), (m, k)
    err = np.abs(w - want).max()
    assert err <= 2 * m * EPS * scale + floor, (m, k, err, scale)
    orth = ref.orthonormality(z)
    assert orth <= 1e-12, (m, k, orth)
    res = ref.tridiag_residual(d, e, w, z)
    assert res <= 1e-12 * scale + floor, (m, k, res, scale)
    # the kernel's own measure never under-reports (the float64 evaluation may differ from the long-double one by rounding)
    assert q >= 0.5 * res / max(scale, floor) - 4 * EPS, (m, k, q, res, scale)
    for _ in range(repeats):
        w2, z2, q2, _ = lab.tridiag_lowest(ctx, d, e, k)
        assert np.array_equal(w, w2) and np.array_equal(z, z2) and (q == q2 or (q != q and q2 != q2)), (m, k, "not reproducible")
    return w, z, q


@pytest.mark.parametrize("m", [2, 3, 8, 63, 64, 65, 127, 128, 129, 222, 255, 256])
def test_lowest_pairs_random(ctx, m):
    """Random T at the orders around the kernels' wave and LDS boundaries; k = 1, a middle value and the largest the kernel accepts."""
    d, e = ref.random_t(m, 100 + m)
    kmax = _largest_k(m)
    want = ref.tridiag_lowest_values(d, e, kmax).astype(float)
    for k in sorted({1, max(1, kmax // 2), kmax}):
        _check_lowest(ctx, d, e, k, want=want[:k])


@pytest.mark.parametrize("name", ["glued_1e-14", "glued_1e-8", "split", "graded", "scaled_up", "scaled_down", "zero", "cI"])
def test_lowest_pairs_hard_small(ctx, name):
    """Order 252 (up to k = 67, the largest the one-workgroup kernel accepts there): twelve glued W+_21 (values that coincide in float64),
    a split T (exact multiplets of twelve, k cut inside one), graded and scaled spectra, the zero matrix and cI.  The glued cases five
    times more, bit for bit."""
    d, e = {"glued_1e-14": ref.glued_wilkinson(12, 1e-14), "glued_1e-8": ref.glued_wilkinson(12, 1e-8), "split": ref.split_t(21, 12, 3),
            "graded": ref.graded_t(252, 6), "scaled_up": ref.scaled_t(252, 7, 300), "scaled_down": ref.scaled_t(252, 8, -300),
            "zero": (np.zeros(252), np.zeros(251)), "cI": (np.full(252, 3.5), np.zeros(251))}[name]
    assert len(d) == 252 and _largest_k(252) == 67
    want = ref.tridiag_lowest_values(d, e, 67).astype(float)
    for k in (1, 18, 67):  # (split: 18 and 67 end inside a multiplet of twelve)
        _check_lowest(ctx, d, e, k, repeats=5 if name.startswith("glued") else 1, want=want[:k])


@pytest.mark.parametrize("name", ["glued_1e-14", "glued_1e-8", "split", "random"])
def test_lowest_pairs_hard_wide(ctx, name):
    """Order 756 through the wide form (k up to 256): 36 glued W+_21, a split T of twelve copies of an order-63 block (k = 100 and 256
    cut inside multiplets: the inverse-iteration vectors of an exact multiplet are nearly dependent before the Cholesky-QR)."""
    d, e = {"glued_1e-14": ref.glued_wilkinson(36, 1e-14), "glued_1e-8": ref.glued_wilkinson(36, 1e-8), "split": ref.split_t(63, 12, 4),
            "random": ref.random_t(756, 11)}[name]
    want = ref.tridiag_lowest_values(d, e, 256).astype(float)
    for k in (1, 100, 256):
        _check_lowest(ctx, d, e, k, repeats=5 if name.startswith("glued") else 1, want=want[:k])


def test_lowest_pairs_of_the_captured_matrix(ctx):
    """T of tests/golden/rr_matrix_order80.bin (six values at 1.579e4 beside 5.6e13) by the product's tridiagonalisation."""
    d, e, _, _, _ = lab.tridiagonalize_full(ctx, _golden(), variant=3)
    for k in (6, 20, 79):
        _check_lowest(ctx, d, e, k)


def test_lowest_pairs_decline_boundary(ctx):
    """Both sides of mh_tridiag_lowest's LDS budget (m k <= 16 896) and of its k <= 128, and the wide form's k <= 256."""
    for m, k, taken in ((240, 70, True), (256, 66, True), (240, 80, False), (130, 128, True), (130, 129, False), (756, 256, True), (756, 257, False)):
        d, e = ref.random_t(m, m + k)
        _, _, q, got = lab.tridiag_lowest(ctx, d, e, k)
        assert got == taken, (m, k, got)
        if taken:
            assert q < 1e-12, (m, k, q)
        else:
            assert q != q


# ---- the whole step --------------------------------------------------------------------------------------------------------
# (name, m, nwant, mass kind, reduction, standard solver): every reduction and every solver branch appears at least once
STEP_CASES = [
    ("m5", 5, 0, "given", "given identity", "syevd"),
    ("m8_partial", 8, 3, ("defect", 1e-9), "series", "small partial"),
    ("m8_full", 8, 0, ("defect", 1e-5), "cholesky", "small stedc"),
    ("golden_full", 80, 0, "I", "measured identity", "small stedc"),
    ("golden_identity", 80, 20, ("defect", 8e-12), "measured identity", "small partial"),
    ("golden_series", 80, 20, ("defect", 8e-8), "series", "small partial"),
    ("golden_cholesky", 80, 0, ("cond", 1e4), "cholesky", "small stedc"),
    ("m128", 128, 40, ("defect", 1e-5), "cholesky", "small partial"),
    ("m222", 222, 74, "given", "given identity", "small partial"),
    ("m240_70", 240, 70, ("defect", 1e-9), "series", "small partial"),
    ("m240_80", 240, 80, "I", "measured identity", "small stedc"),  # m k above the LDS budget: the partial kernel declines
    ("m256_66", 256, 66, ("defect", 8e-12), "measured identity", "small partial"),
    ("m257_86", 257, 86, "given", "given identity", "wide partial"),
    ("m720_215", 720, 215, ("defect", 8e-8), "series", "wide partial"),
    ("m720_257", 720, 257, "given", "given identity", "wide stedc+ormtr"),
    ("m720_full", 720, 0, "I", "measured identity", "wide stedc+ormtr"),
    ("m768_256", 768, 256, ("defect", 1e-9), "series", "wide partial"),
    ("m769", 769, 100, "given", "given identity", "syevd"),
]


def _series_standard(a, mm):
    e = mm - np.eye(len(a))
    s = np.eye(len(a)) - 0.5 * e + 0.375 * (e @ e)
    return s @ a @ s


def test_step_cases_cover_every_branch():
    assert {c[4] for c in STEP_CASES} == set(lab.RR_REDUCTIONS)
    assert {c[5] for c in STEP_CASES} == set(lab.RR_SOLVERS)


@pytest.mark.parametrize("case", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_rayleigh_ritz_step(ctx, case):
    """theta within 8 m eps max|theta| of scipy's eigh(A, M) (its own long-double residual checked first); C^T M C - I within 16 m eps;
    every column's residual ||A c - theta M c||_inf within 16 m eps (||A|| + |theta| ||M||) ||c||_inf.  The identity branch ignores
    E = gM - I, so there the bounds widen by ||E||_2 (|theta| for the values): a change to its 1e-11 threshold moves the cases at
    1e-9 and 8e-8 off the series and fails them.  The Cholesky branch widens by cond(M).  Upper triangles are NaN: only the lower
    ones may be read.  A repeat is bit-identical."""
    from scipy.linalg import eigh
    name, m, nwant, kind, reduction, solver = case
    a = _golden() if name.startswith("golden") else ref.rr_matrix(m, m)
    given = kind == "given"
    mm = np.eye(m) if given else ref.rr_mass(m, kind, m + 1)
    poison = np.triu(np.full((m, m), np.nan), 1)
    theta, c, host, tr = lab.rr_solve(ctx, np.tril(a) + poison, np.tril(mm) + poison, nwant=nwant, gm_is_identity=given)
    assert (tr["reduction"], tr["solver"]) == (reduction, solver), (name, tr)
    partial = solver.endswith("partial")
    ncols = nwant if partial else m
    assert c.shape == (m, ncols) and len(theta) == ncols, (name, c.shape)
    if solver == "small partial":
        assert host is not None and np.array_equal(host, theta), name
    else:
        assert host is None, name
    measured_identity = reduction == "measured identity"
    if partial:
        # the self-check samples columns 0, ncols / 2, ncols - 1 of the standard problem: at rounding level (1e-11), or -- where the
        # standard matrix's rows are graded like the captured one's (six rows at 1.6e4 beside 2e13) -- within 10x of the same measure
        # on LAPACK's own vectors (1e-7 .. 1e-6 there for every driver)
        b = a if reduction != "series" else _series_standard(a, mm)
        if reduction == "cholesky":
            lf = np.linalg.cholesky(mm)
            b = np.linalg.solve(lf, np.linalg.solve(lf, a).T)
        tb, zb = np.linalg.eigh(0.5 * (b + b.T))
        cols = [0, ncols // 2, ncols - 1]
        lapack = ref.selfcheck_measure(b, zb[:, cols], tb[cols]).max()
        assert tr["quality"] < 1e-10 and 0 < tr["selfcheck"] <= max(1e-11, 10 * lapack), (name, tr, lapack)
    if not given:
        assert tr["defect"] == np.abs(np.tril(mm) - np.eye(m)).max(), (name, tr["defect"])
    e2 = np.linalg.norm(mm - np.eye(m), 2) if measured_identity else 0.0  # what the identity branch ignores
    cond = np.linalg.cond(mm) if reduction == "cholesky" else 1.0
    mnorm = np.linalg.norm(mm, 2)
    anorm = np.linalg.norm(a, 2)

    # the reference first: scipy's pencil solution, its own long-double residual on the columns compared
    th_ref, c_ref = eigh(a, mm)
    nchk = min(ncols, 128)
    ac, mc = ref.pencil_products(a, None if given else mm, c_ref[:, :nchk])
    res_ref = ref.pencil_residual(ac, mc, th_ref[:nchk])
    assert np.all(res_ref <= 16 * m * EPS * cond * (anorm + np.abs(th_ref[:nchk]) * mnorm) * np.abs(c_ref[:, :nchk]).max(axis=0)), name

    scale = np.abs(th_ref).max()
    err = np.abs(theta - th_ref[:ncols])
    tol = 8 * m * EPS * scale * cond + e2 * np.abs(th_ref[:ncols])
    assert np.all(err <= tol), (name, (err / tol).max())

    ac, mc = ref.pencil_products(a, None if (given or kind == "I") else mm, c)
    orth = ref.orthonormality(c, mc)
    assert orth <= 16 * m * EPS * cond + e2, (name, orth)
    res = ref.pencil_residual(ac, mc, theta)
    cinf = np.abs(c).max(axis=0)
    rtol = (16 * m * EPS * cond * (anorm + np.abs(theta) * mnorm) + e2 * np.abs(theta)) * cinf
    assert np.all(res <= rtol), (name, (res / rtol).max())

    theta2, c2, host2, tr2 = lab.rr_solve(ctx, np.tril(a) + poison, np.tril(mm) + poison, nwant=nwant, gm_is_identity=given)
    assert np.array_equal(theta, theta2) and np.array_equal(c, c2) and tr2["solver"] == solver, (name, "not reproducible")
