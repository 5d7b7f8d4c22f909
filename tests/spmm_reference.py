"""Extended-precision host reference of the BSR 3x3 block product (mesheditor_amd/csrc/mh_spmm.hip) with error bounds that are derived
here, not fitted to any output: crafted matrices, the products in numpy.longdouble, the bounds, and the comparisons that the GPU tests
(tests/test_spmm_forms_gpu.py) and the CPU test of this module (tests/test_spmm_reference_cpu.py) share.

The product bound.  A kernel forms row i of y = A x as a sum of 3 L products (L = node blocks of the row), accumulated in some order
into up to G partial sums (one per lane group, G <= 8) which a shuffle tree or chain then adds.  Whatever the order, and with or without
contraction of a product and its addition into one fused operation, every product passes through at most 1 rounding of its own and
at most 3 L - 1 + 7 additions, so (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1)

    |y_i - (A x)_i|  <=  gamma(3 L + 8) (|A| |x|)_i,        gamma(k) = k u / (1 - k u),

with u = 2^-53 for the double-precision and mixed forms and u = 2^-24 for the single-precision ones.  The single-precision forms get
their block values and panels as floats, so nothing is rounded before the kernel starts.  The reference itself is evaluated in
numpy.longdouble (u = 2^-64 on x86-64): its own error is 2^-11 of the double-precision bound and is ignored; where longdouble is no
wider than double the bound is widened by one more gamma (reference_slack).
"""
import functools

import numpy as np

LD = np.longdouble
U64, U32 = 2.0 ** -53, 2.0 ** -24
WIDEST = 260  # columns of the shared panel: every narrower width is a column slice of it

SPECIAL_LENGTHS = tuple(range(18)) + (31, 32, 33, 63, 64, 65, 66, 96, 127, 128, 129, 130, 200)


def gamma(k, u):
    k = np.asarray(k, dtype=np.float64)
    return k * u / (1.0 - k * u)


def reference_slack():
    """1 when longdouble is wider than double, else 2: the reference then has the rounding errors of a double-precision product too."""
    return 1.0 if np.finfo(LD).eps < np.finfo(np.float64).eps else 2.0


class Bsr:
    """Node-block matrix: row_ptr (n + 1), col (sorted, distinct per row), vals (nb x 3 x 3, NON-symmetric), mass (nb), uint32 / float64."""

    def __init__(self, row_ptr, col, vals, mass):
        self.row_ptr, self.col, self.vals, self.mass = row_ptr, col, vals, mass
        self.n = len(row_ptr) - 1
        self.lengths = np.diff(row_ptr.astype(np.int64))
        self.row_of = np.repeat(np.arange(self.n), self.lengths)
        self.vals32 = vals.astype(np.float32)  # the single-precision forms' operator: the reference of those forms uses THESE values

    def copy(self):
        return Bsr(self.row_ptr.copy(), self.col.copy(), self.vals.copy(), self.mass.copy())


def make_matrix(n, lengths, seed):
    """Rows of the given block counts (n of them), sorted distinct random columns, block entries of magnitude 10^U(-3, 3) with random
    signs (so that |A| |x| is far above |A x| in places and the bound bites), mass scalars 10^U(-2, 2) with random signs, unrelated
    to the blocks."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    assert len(lengths) == n and lengths.max() <= n
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
    col = np.concatenate([np.sort(rng.choice(n, size=k, replace=False)) for k in lengths] + [np.zeros(0, np.int64)]).astype(np.uint32)
    nb = int(row_ptr[-1])
    vals = 10.0 ** rng.uniform(-3, 3, (nb, 3, 3)) * rng.choice([-1.0, 1.0], (nb, 3, 3))
    mass = 10.0 ** rng.uniform(-2, 2, nb) * rng.choice([-1.0, 1.0], nb)
    return Bsr(row_ptr, col, vals, mass)


@functools.lru_cache(maxsize=None)
def crafted():
    """261 nodes (not a multiple of 8: the padded grids have rows past the end).  Every length of SPECIAL_LENGTHS occurs, the others are
    1 .. 12; the first row is the empty one, the last row is the longest (200 blocks: four strips of the wide kernel, the last of them
    8 blocks), and the 130-block row sits in the last workgroup octet too."""
    n = 261
    rng = np.random.default_rng(2610)
    lengths = rng.integers(1, 13, n)
    slots = rng.permutation(np.arange(1, n - 2))[: len(SPECIAL_LENGTHS) - 3]
    rest = [k for k in SPECIAL_LENGTHS if k not in (0, 130, 200)]
    lengths[slots] = rng.permutation(rest)
    lengths[0], lengths[n - 2], lengths[n - 1] = 0, 130, 200
    assert sorted(set(SPECIAL_LENGTHS) - set(lengths.tolist())) == []
    return make_matrix(n, lengths, 2611)


@functools.lru_cache(maxsize=None)
def one_node():
    return make_matrix(1, [1], 11)


@functools.lru_cache(maxsize=None)
def seven_nodes():
    """Fewer rows than a workgroup octet; lengths 0 .. 7 less one (a row shorter than every lane-group count, and the full row)."""
    return make_matrix(7, [3, 0, 7, 1, 2, 5, 7], 71)


def panel(n3, w, seed, scale=1.0):
    """A float32-representable panel as float64: normal entries times 10^U(-2, 2)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n3, w)) * 10.0 ** rng.uniform(-2, 2, (n3, w)) * scale
    return x.astype(np.float32).astype(np.float64)


def block_product(m, blocks, x, dtype=LD, order=None):
    """sum over a row's node blocks of blocks[p] (3 x 3) times rows 3 col[p] .. 3 col[p] + 2 of x, accumulated in `dtype` block after
    block in the order `order` (a permutation of the blocks; default: storage order).  3 n x w."""
    xb = np.asarray(x, dtype=dtype).reshape(m.n, 3, -1)
    contrib = np.einsum("pij,pjc->pic", np.asarray(blocks, dtype=dtype), xb[m.col.astype(np.int64)])
    y = np.zeros((m.n, 3, xb.shape[2]), dtype=dtype)
    rows = m.row_of
    if order is not None:
        rows, contrib = rows[order], contrib[order]
    np.add.at(y, rows, contrib)
    return y.reshape(3 * m.n, -1)


def mass_blocks(m, mass=None):
    return (m.mass if mass is None else mass)[:, None, None] * np.eye(3)


class Products:
    """A x, M x, |A| |x|, |M| |x| of the widest panel in longdouble, and the per-row gamma factors; width w = the first w columns."""

    def __init__(self, m, x, single=False):
        self.m, self.x, self.u = m, x, U32 if single else U64
        vals = m.vals32.astype(np.float64) if single else m.vals
        self.ax = block_product(m, vals, x)
        self.mx = block_product(m, mass_blocks(m), x)
        self.abs_ax = block_product(m, np.abs(vals), np.abs(x))
        self.abs_mx = block_product(m, mass_blocks(m, np.abs(m.mass)), np.abs(x))
        self.g = np.repeat(gamma(3 * m.lengths + 8, self.u) * reference_slack(), 3)[:, None]  # per DOF row

    def bound_a(self, w):
        return (self.g * self.abs_ax[:, :w]).astype(np.float64)

    def bound_m(self, w):
        return (self.g * self.abs_mx[:, :w]).astype(np.float64)


class Comparison:
    """got against want +- bound; want is NaN where the entry must still hold the sentinel.  `untouched` is the bitwise sentinel test of got."""

    def __init__(self, got, untouched, want, bound):
        expect_write = ~np.isnan(want.astype(np.float64))
        self.missing = int((untouched & expect_write).sum())    # should have been written and was not
        self.stray = int((~untouched & ~expect_write).sum())    # should not have been touched and was
        idx = np.flatnonzero(expect_write & ~untouched)
        g = np.asarray(got).reshape(-1)[idx]
        # the difference in longdouble; the quotient of the (rounded) difference and the bound in double
        err = np.abs(g.astype(LD) - np.asarray(want).reshape(-1)[idx]).astype(np.float64)
        b = np.broadcast_to(np.asarray(bound, dtype=np.float64), np.shape(got)).reshape(-1)[idx]
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(err == 0, 0.0, err / b)  # (an exact entry under a zero bound -- an empty row -- is inside)
        r[~np.isfinite(g.astype(np.float64)) | np.isnan(r)] = np.inf
        ratio = np.zeros(np.shape(got))
        ratio.reshape(-1)[idx] = r
        self.ratio = ratio
        self.worst = float(ratio.max()) if ratio.size else 0.0
        self.outside = int((ratio > 1).sum())

    @property
    def ok(self):
        return self.missing == 0 and self.stray == 0 and self.outside == 0

    def __repr__(self):
        return "missing %d, stray %d, outside the bound %d, worst error / bound %.3g" % (self.missing, self.stray, self.outside, self.worst)


def compare(got, want, bound, untouched=None):
    if untouched is None:
        untouched = np.zeros(np.shape(got), bool)
    return Comparison(got, untouched, want, bound)


def mapped_expectation(y, bound, omap, wreal, ldy):
    """What a mapped launch must leave in an output panel of pitch ldy: column c < wreal of y at column omap[c], the sentinel (NaN here)
    everywhere else -- the columns omap skips, the columns from wreal on (the pad column of an odd count among them) and the gap up to ldy."""
    want = np.full((y.shape[0], ldy), np.nan, dtype=LD)
    bnd = np.ones((y.shape[0], ldy))
    want[:, omap[:wreal]] = y[:, :wreal]
    bnd[:, omap[:wreal]] = bound[:, :wreal]
    return want, bnd


# ---- the residual epilogue ------------------------------------------------------------------------------------------------------
# r and the partial sums are formed from the registers that were stored as y and y2, so they are judged against THOSE values:
#   r = fl(y - fl(theta y2)) (or one fused operation): two roundings at most, each of relative size u / (1 + u), the first on
#   |theta y2|, the second on |y - theta y2 (1 + d)| <= |y| + |theta y2| (1 + u):   |r - (y - theta y2)| <= 2 u (|y| + |theta| |y2|).
#   partial = ((0 + w0 r0^2) + w1 r1^2) + w2 r2^2: per term two products and at most two additions, all terms non-negative (w > 0):
#   relative error gamma(4) <= 6 u.
def residual_bound(y, y2, theta):
    return 2 * U64 * (np.abs(y) + np.abs(theta)[None, :] * np.abs(y2))


def residual_exact(y, y2, theta):
    return np.asarray(y, dtype=LD) - np.asarray(theta, dtype=LD)[None, :] * np.asarray(y2, dtype=LD)


def partial_exact(v, weights):
    """sum over the three rows of a node of weight * v^2: n x w (v: 3 n x w, weights: 3 n or None)."""
    v = np.asarray(v, dtype=LD)
    wgt = np.ones(v.shape[0], dtype=LD) if weights is None else np.asarray(weights, dtype=LD)
    return (wgt[:, None] * v * v).reshape(-1, 3, v.shape[1]).sum(axis=1)


def partial_bound(exact):
    return 6 * U64 * np.abs(exact).astype(np.float64)


def unstored_residual(p, theta, w, weights):
    """Columns whose y and y2 are not stored (wreal <= c < w) still get r and the partials.  r is stored, so its partial is judged
    like every other column's; r itself and the partial of M x are judged against the reference product with the product's bounds
    b_a, b_m carried through: |r - r_ref| <= b_a + |theta| b_m + 2 u (|y| + |theta| |y2|), and with v = (M x)_ref, b = b_m:
    |partial - sum w v^2| <= sum w (2 |v| b + b^2) + 6 u sum w v^2.  Returns (r, its bound, partial of M x, its bound), all of width w."""
    y, y2, ba, bm = p.ax[:, :w], p.mx[:, :w], p.bound_a(w), p.bound_m(w)
    r = residual_exact(y, y2, theta)
    br = ba + np.abs(theta)[None, :] * bm + residual_bound(y.astype(np.float64), y2.astype(np.float64), theta)
    wgt = np.ones(y.shape[0]) if weights is None else np.asarray(weights, dtype=np.float64)
    pm = partial_exact(y2, weights)
    v = np.abs(y2).astype(np.float64)
    return r, br, pm, (wgt[:, None] * (2 * v * bm + bm * bm)).reshape(-1, 3, w).sum(axis=1) + partial_bound(pm)


# ---- the fused Chebyshev step ---------------------------------------------------------------------------------------------------
# In single precision (u = 2^-24), all inputs floats:   t = A d,   r' = r - t,   d' = c1 d + (c2 dinv) r',   x' = x + d'.
# First order, with b_t = gamma(3 L + 8) |A| |d| the product's bound:
#   r' = fl(r - t^):  the product's error passes through unchanged, the subtraction adds u |r'|:          b_r = b_t + u |r'|
#   d' = fl(fl(c1 d) + fl(fl(c2 dinv) r'^)):  an error of r'^ is scaled by |c2 dinv|; c1 d passes one product and one addition (2 u), the
#        other term two products and the addition (3 u) -- fused or not, no more:                         b_d = |c2 dinv| b_r + 4 u (|c1 d| + |c2 dinv r'|)
#   x' = fl(x + d'^):  d's error passes through, the addition adds u |x'|:                                b_x = b_d + u |x'|
# The magnitudes on the right are the reference's own; the terms left out are products of two of the errors above (relative size u
# or gamma against the first-order ones), so each bound is DOUBLED to cover them.
def chebyshev_reference(m, d, r, x, dinv, c1, c2):
    """(r', d', x') in longdouble and their bounds; d, r, x: float32 panels, dinv: 3 n float32, c1, c2: float32 scalars."""
    u = U32
    d64 = d.astype(np.float64)
    vals = m.vals32.astype(np.float64)
    t = block_product(m, vals, d64)
    bt = np.repeat(gamma(3 * m.lengths + 8, u) * reference_slack(), 3)[:, None] * block_product(m, np.abs(vals), np.abs(d64)).astype(np.float64)
    s = (LD(c2) * dinv.astype(LD))[:, None]
    c1d = LD(c1) * d.astype(LD)
    rn = r.astype(LD) - t
    dn = c1d + s * rn
    xn = x.astype(LD) + dn
    f = lambda a: np.abs(a).astype(np.float64)  # noqa: E731
    br = bt + u * f(rn)
    bd = f(s) * br + 4 * u * (f(c1d) + f(s * rn))
    bx = bd + u * f(xn)
    return (rn, 2 * br), (dn, 2 * bd), (xn, 2 * bx)
