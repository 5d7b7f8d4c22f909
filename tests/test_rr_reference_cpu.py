"""The extended-precision references of tests/rr_reference.py, judged before they judge a kernel: the long-double Sturm bisection against
mpmath at 40 digits on small orders, and against scipy's tridiagonal eigensolver at every order the GPU tests use."""
import numpy as np
import pytest

from tests import rr_reference as ref

EPS = np.finfo(float).eps


def _mp_eigvalsh(d, e):
    import mpmath
    with mpmath.workdps(40):
        m = len(d)
        t = mpmath.matrix(m, m)
        for i in range(m):
            t[i, i] = mpmath.mpf(float(d[i]))
            if i + 1 < m:
                t[i, i + 1] = t[i + 1, i] = mpmath.mpf(float(e[i]))
        w = mpmath.eigsy(t, eigvals_only=True)
        return sorted(w)


@pytest.mark.parametrize("name", ["wilkinson21", "glued2", "graded42"])
def test_bisection_agrees_with_40_digits(name):
    """At orders <= 42, every value to 1e-17 ||T||: W+_21 (pairs agreeing to 14 digits), two glued copies of it (values that coincide in
    float64), a graded T over 16 decades."""
    import mpmath
    d, e = {"wilkinson21": ref.wilkinson(21), "glued2": ref.glued_wilkinson(2, 1e-14), "graded42": ref.graded_t(42, 5)}[name]
    m = len(d)
    got = ref.tridiag_lowest_values(d, e, m)
    want = _mp_eigvalsh(d, e)
    scale = ref.tnorm(d, e)
    with mpmath.workdps(40):
        err = max(abs(mpmath.mpf(str(g)) - w) for g, w in zip(got, want))  # str(): the long double's own digits, not a float64 of them
    assert float(err) <= 1e-17 * scale, (name, float(err), scale)
    assert np.all(np.diff(got) >= 0)


def _cases():
    yield "random64", ref.random_t(64, 1), 64
    yield "random255", ref.random_t(255, 2), 128
    yield "glued12_1e-14", ref.glued_wilkinson(12, 1e-14), 67
    yield "glued12_1e-8", ref.glued_wilkinson(12, 1e-8), 67
    yield "glued36_1e-14", ref.glued_wilkinson(36, 1e-14), 256
    yield "split", ref.split_t(21, 12, 3), 67
    yield "split756", ref.split_t(63, 12, 4), 256
    yield "graded", ref.graded_t(128, 6), 64
    yield "scaled_up", ref.scaled_t(127, 7, 300), 64
    yield "scaled_down", ref.scaled_t(127, 8, -300), 64
    yield "zero", (np.zeros(65), np.zeros(64)), 65
    yield "cI", (np.full(65, 3.5), np.zeros(64)), 65


@pytest.mark.parametrize("name,t,k", list(_cases()), ids=[c[0] for c in _cases()])
def test_bisection_agrees_with_scipy(name, t, k):
    """At the orders and matrices of the GPU tests: within a few eps ||T|| of LAPACK's float64 bisection (stebz), and within LAPACK's own
    bound m eps ||T|| of its default solver (stemr, measured up to 11 eps ||T|| off at m = 64)."""
    from scipy.linalg import eigvalsh_tridiagonal
    d, e = t
    got = ref.tridiag_lowest_values(d, e, k).astype(float)
    scale = ref.tnorm(d, e)
    for driver, tol in (("stebz", 4 * EPS * scale), ("auto", len(d) * EPS * scale)):
        want = eigvalsh_tridiagonal(d, e, lapack_driver=driver)[:k]
        assert np.all(np.abs(got - want) <= tol), (name, driver, np.abs(got - want).max() / max(scale, 1e-300))
    assert np.all(np.diff(got) >= 0)


def test_long_double_measures():
    """The residual and orthonormality helpers at rounding level on LAPACK's vectors, and a column scaled by 1 + 1e-13 seen as 2e-13."""
    d, e = ref.random_t(50, 9)
    t = ref.tridiag_matrix(d, e)
    w, z = np.linalg.eigh(t)
    assert ref.tridiag_residual(d, e, w, z) < 50 * EPS * ref.tnorm(d, e)
    assert ref.orthonormality(z) < 50 * EPS
    z2 = z.copy()
    z2[:, 3] *= 1 + 1e-13
    assert 1.5e-13 < ref.orthonormality(z2) < 2.5e-13
    a = ref.rr_matrix(40, 3)
    mm = ref.rr_mass(40, ("defect", 1e-9), 3)
    from scipy.linalg import eigh
    th, c = eigh(a, mm)
    ac, mc = ref.pencil_products(a, mm, c)
    assert ref.pencil_residual(ac, mc, th).max() < 40 * EPS * np.abs(a).max() * np.abs(c).max() * 40
    assert ref.orthonormality(c, mc) < 40 * EPS * 10


def test_generators():
    """Exact multiplets in the split matrix, coinciding float64 values in the glued one, the pencil's shape and mass defects."""
    from scipy.linalg import eigvalsh_tridiagonal
    d, e = ref.split_t(21, 12, 3)
    w = ref.tridiag_lowest_values(d, e, 24)
    assert np.all(w[:12] == w[0]) and np.all(w[12:24] == w[12])
    w = eigvalsh_tridiagonal(*ref.glued_wilkinson(12, 1e-14))
    assert np.any(np.diff(w) == 0)
    s = ref.rr_spectrum(80, 1)
    assert np.all(s[:6] == -ref.SIGMA) and s[6] >= 3.2e9 and s[-1] <= 5.6e13 and np.all(np.diff(s) >= 0)
    for dmax in (8e-12, 1e-9, 8e-8, 1e-5):
        mm = ref.rr_mass(64, ("defect", dmax), 2)
        assert np.array_equal(mm, mm.T) and np.abs(mm - np.eye(64)).max() == pytest.approx(dmax, rel=1e-12)
    mm = ref.rr_mass(64, ("cond", 1e4), 2)
    assert np.linalg.cond(mm) == pytest.approx(1e4, rel=1e-6)
