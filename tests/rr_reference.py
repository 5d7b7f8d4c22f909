"""Plain-numpy references for the Rayleigh-Ritz step (tests/test_rayleigh_ritz_gpu.py judges the kernels by them, tests/
test_rr_reference_cpu.py judges them first): the k lowest eigenvalues of a symmetric tridiagonal matrix by Sturm-count bisection in
extended precision (np.longdouble, a 64-bit mantissa on x86), residual and orthonormality measures evaluated in the same precision,
and seeded generators of the matrices where partial-spectrum kernels go wrong -- coinciding eigenvalues, exact multiplets, graded and
scaled spectra -- and of Rayleigh-Ritz pencils shaped like the solver's own."""
import numpy as np

LD = np.longdouble


def tnorm(d, e):
    """Gershgorin bound max_i |d_i| + |e_{i-1}| + |e_i| (the scale the kernels use for ||T||)."""
    d, e = np.asarray(d, float), np.abs(np.asarray(e, float))
    r = np.abs(d).copy()
    r[:-1] += e
    r[1:] += e
    return float(r.max()) if len(d) else 0.0


def sturm_count(d, e2, x, pivmin):
    """Number of eigenvalues of T (diagonal d, squared off-diagonal e2, both longdouble) below each x (longdouble array): the signs
    of the pivots of T - x I (LAPACK dlaebz, the pivot kept away from 0 by pivmin)."""
    q = d[0] - x
    q = np.where(np.abs(q) < pivmin, -pivmin, q)
    c = (q < 0).astype(np.int64)
    for i in range(1, len(d)):
        q = (d[i] - x) - e2[i - 1] / q
        q = np.where(np.abs(q) < pivmin, -pivmin, q)
        c += q < 0
    return c


def tridiag_lowest_values(d, e, k):
    """The k lowest eigenvalues of the symmetric tridiagonal (d, e) by bisection on Sturm counts in long double, all k intervals at
    once; each interval is halved until its midpoint equals an end (one long-double ulp)."""
    m = len(d)
    dl, el = np.asarray(d, LD), np.asarray(e, LD)
    e2 = el * el
    r = np.abs(dl).copy()
    if m > 1:
        r[:-1] += np.abs(el)
        r[1:] += np.abs(el)
    rad = np.zeros(m, LD)
    if m > 1:
        rad[:-1] += np.abs(el)
        rad[1:] += np.abs(el)
    gl, gh = (dl - rad).min(), (dl + rad).max()
    scale = max(r.max(), LD(np.finfo(float).tiny))
    pivmin = LD(np.finfo(LD).tiny) * max(LD(1), e2.max() if m > 1 else LD(1))
    gl -= 4 * scale * np.finfo(LD).eps * m + 2 * pivmin
    gh += 4 * scale * np.finfo(LD).eps * m + 2 * pivmin
    j = np.arange(k)
    lo, hi = np.full(k, gl, LD), np.full(k, gh, LD)
    for _ in range(20000 // max(m, 1) + 200):
        mid = lo + (hi - lo) / 2
        live = (mid != lo) & (mid != hi)
        if not live.any():
            break
        c = sturm_count(dl, e2, mid, pivmin)
        up = c >= j + 1
        hi = np.where(live & up, mid, hi)
        lo = np.where(live & ~up, mid, lo)
    return lo + (hi - lo) / 2


def tridiag_matrix(d, e):
    return np.diag(np.asarray(d, float)) + np.diag(np.asarray(e, float), 1) + np.diag(np.asarray(e, float), -1)


def tridiag_residual(d, e, w, z):
    """max over the columns of ||T z_j - w_j z_j||_inf, in long double."""
    dl, el, zl, wl = np.asarray(d, LD), np.asarray(e, LD), np.asarray(z, LD), np.asarray(w, LD)
    r = (dl[:, None] - wl[None, :]) * zl
    r[:-1] += el[:, None] * zl[1:]
    r[1:] += el[:, None] * zl[:-1]
    return float(np.abs(r).max())


def orthonormality(z, mz=None):
    """max |Z^T Z - I| (or max |Z^T (M Z) - I| with mz = M Z given), in long double."""
    zl = np.asarray(z, LD)
    g = zl.T @ (zl if mz is None else np.asarray(mz, LD))
    return float(np.abs(g - np.eye(g.shape[0], dtype=LD)).max())


def pencil_products(a, mmat, c):
    """(A C, M C) in long double from the full symmetric matrices; M C is C itself when mmat is None (M = I exactly)."""
    cl = np.asarray(c, LD)
    ac = np.asarray(a, LD) @ cl
    return ac, (cl if mmat is None else np.asarray(mmat, LD) @ cl)


def pencil_residual(ac, mc, theta):
    """Per column ||A c - theta M c||_inf from the products of pencil_products, in long double."""
    return np.abs(ac - mc * np.asarray(theta, LD)[None, :]).max(axis=0).astype(float)


def selfcheck_measure(b, z, theta):
    """The solver's sampled self-check (k_rr_selfcheck) on every column: max_i |(B z - theta z)_i| / (max_i sum_c |b_ic z_c| + |theta| max |z|),
    in long double.  A normwise backward-stable solver stays near eps only where B's rows are scaled like its eigenvalue."""
    bl, zl, tl = np.asarray(b, LD), np.asarray(z, LD), np.asarray(theta, LD)
    r = np.abs(bl @ zl - zl * tl[None, :]).max(axis=0)
    den = (np.abs(bl) @ np.abs(zl)).max(axis=0) + np.abs(tl) * np.abs(zl).max(axis=0)
    return (r / den).astype(float)


# ---- tridiagonal generators ------------------------------------------------------------------------------------------------
def random_t(m, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(m), rng.standard_normal(m - 1)


def wilkinson(n=21):
    """W+_n: d = |n//2 - i|, e = 1 -- its top eigenvalues come in pairs that agree to many digits."""
    h = n // 2
    return np.abs(np.arange(n) - h).astype(float), np.ones(n - 1)


def glued_wilkinson(copies, glue, n=21):
    """`copies` W+_n along the diagonal joined by off-diagonal entries `glue`: clusters of `copies` eigenvalues that coincide in float64."""
    d, e = wilkinson(n)
    dd = np.tile(d, copies)
    ee = np.concatenate([np.concatenate([e, [glue]]) for _ in range(copies)])[:-1]
    return dd, ee


def split_t(block, copies, seed):
    """A random block of order `block` repeated `copies` times with zero off-diagonals at the joints: every eigenvalue of the block
    is an exact multiplet of multiplicity `copies`."""
    d, e = random_t(block, seed)
    dd = np.tile(d, copies)
    ee = np.concatenate([np.concatenate([e, [0.0]]) for _ in range(copies)])[:-1]
    return dd, ee


def graded_t(m, seed, decades=16):
    """Diagonal graded over `decades` decades, off-diagonals geometric means of their neighbours (times a random factor below 1)."""
    rng = np.random.default_rng(seed)
    d = np.logspace(0, -decades, m) * rng.choice([-1.0, 1.0], m)
    e = np.sqrt(np.abs(d[:-1] * d[1:])) * rng.uniform(0.1, 0.9, m - 1)
    return d, e


def scaled_t(m, seed, power):
    d, e = random_t(m, seed)
    return np.ldexp(d, power), np.ldexp(e, power)


# ---- Rayleigh-Ritz pencils ---------------------------------------------------------------------------------------------------
SIGMA = -(2 * np.pi * 20.0) ** 2  # the solver's shift: the rigid-body values of K - sigma M sit at -sigma = 1.579e4


def rr_spectrum(m, seed):
    """Ascending values shaped like a Rayleigh-Ritz step's (tests/golden/rr_matrix_order80.bin): six at -sigma, elastic values from 3.2e9
    in exact triples over the first half of the rest, search directions up to 5.6e13 above them."""
    rng = np.random.default_rng(seed)
    rigid = np.full(min(6, m), -SIGMA)
    rest = m - len(rigid)
    n_el = rest // 2
    triples = np.sort(3.2e9 * np.exp(rng.uniform(0, np.log(30.0), (n_el + 2) // 3)))
    elastic = np.repeat(triples, 3)[:n_el]
    search = np.sort(np.exp(rng.uniform(np.log(2e11), np.log(5.6e13), rest - n_el)))
    return np.concatenate([rigid, elastic, search])


def random_orthogonal(m, seed):
    rng = np.random.default_rng(seed)
    q, r = np.linalg.qr(rng.standard_normal((m, m)))
    return q * np.sign(np.diag(r))[None, :]


def rr_matrix(m, seed):
    """A = Q diag(rr_spectrum) Q^T, symmetric to the bit."""
    q = random_orthogonal(m, seed)
    a = (q * rr_spectrum(m, seed)[None, :]) @ q.T
    return 0.5 * (a + a.T)


def defect_matrix(m, dmax, seed):
    """A dense symmetric E with max |E| = dmax whose square does not cancel: 0.9 dmax 1 1^T plus 0.1 dmax symmetric noise (||E||_2 is about
    0.9 m dmax, and E^2 about 0.8 m dmax^2 1 1^T)."""
    rng = np.random.default_rng(seed)
    n = rng.uniform(-1, 1, (m, m))
    e = 0.9 + 0.1 * 0.5 * (n + n.T)
    return e * (dmax / np.abs(e).max())


def conditioned_spd(m, cond, seed):
    """A symmetric positive definite M with eigenvalues geometric from 1 down to 1 / cond."""
    q = random_orthogonal(m, seed + 1)
    mm = (q * np.logspace(0, -np.log10(cond), m)[None, :]) @ q.T
    return 0.5 * (mm + mm.T)


def rr_mass(m, kind, seed):
    """The Gram matrix gM of a pencil: "I" (exactly the identity), ("defect", dmax) for I + defect_matrix, ("cond", c) for conditioned_spd."""
    if kind == "I":
        return np.eye(m)
    what, val = kind
    if what == "defect":
        return np.eye(m) + defect_matrix(m, val, seed)
    if what == "cond":
        return conditioned_spd(m, val, seed)
    raise ValueError(kind)
