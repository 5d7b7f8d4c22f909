"""Extended-precision host reference of the dense tall products (mesheditor_amd/csrc/mh_dense.hip: mh_combine, mh_short_product, mh_gram
and the two coefficient packers) with bounds that are derived here, not fitted to any output.  Shared by the GPU tests
(tests/test_combine_forms_gpu.py) and the CPU test of this module (tests/test_combine_reference_cpu.py).

The operations, restated.  S = [X[:, xmap] | W | P] is n x m (X's logical column k is physical column xmap[k] of a panel of pitch ldx;
no map: column k), Ct is m x nc row-major ("k-major"), Z = S Ct.  Column c < n1 of Z goes to column omap[c] (no map: c) of out1, a panel
of pitch ld1; column c >= n1 to column c - n1 of out2, pitch nc - n1.  With a column range only columns col_begin <= c < col_begin +
col_count are computed and stored.  accumulate: out = old + Z.  mh_pack_coefficients sets two column-major blocks side by side,
Ct = [C1 | C2]; mh_pack_stacked sets them one above the other and scales, Ct = scale [C1; C2]: one multiplication per entry, which numpy
repeats bit for bit.  The Gram product is G = X^T Y[:, ymap], written column-major into a block of a larger matrix.

The bound.  u = 2^-53.  An entry z = sum_k s_k c_k of m terms, evaluated in ANY order by fused or unfused multiply-adds, with or without
zero terms padded in (x + 0 is exact): every term passes through at most one rounding of its own and at most m - 1 additions of two
non-zero operands, so (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1)

    |z^ - z|  <=  gamma(m) sum_k |s_k c_k|,     gamma(m) = m u / (1 - m u)  <=  (m + 1) u   for m <= 2^26.

The bound used is (m + 8) u (|S| |Ct|)_ij: the seven further u pay for the reference's own rounding (longdouble, u = 2^-64: 2^-11 of
a term of the sum) with room to spare, and are nothing beside what the inputs make of a mistake (below).
  accumulate:  out = fl(old + z^) adds one rounding, u |old + z^| <= u |old| + u (1 + gamma) |S| |Ct|: the second part is inside the
      seven spare u, the first is granted twice over:  + 2 u |old_ij|.
  K slices:    each slice is such a sum over its part of the terms; the `slices` partial results are then added one after the other,
      at most `slices` further additions on every term:  + slices u (|S| |Ct|)_ij.
  Gram:        the same sum over the n rows, cut into workgroup partials, wave partials and a fixed-order reduction -- an order like
      any other:  (n + 8) u (|X|^T |Y|)_ij.
Where longdouble is no wider than double the bounds are doubled (spmm_reference.reference_slack).

The inputs.  Magnitudes uniform in [0.5, 2] with random signs, panels and coefficients alike: every single term is at least 0.25 in
magnitude while the bound of an entry is about 4 m^2 u, so a dropped, duplicated or misplaced term is far outside it (min_term_over_bound
measures by how much, and the CPU test asserts a factor of 100 for the shapes used)."""
import numpy as np

from tests.spmm_reference import Comparison, compare, reference_slack  # noqa: F401  (compare: the judgement both suites share)

LD = np.longdouble
U = 2.0 ** -53


WIDEST_M, MOST_SLICES, MOST_GRAM_ROWS = 416, 8, 65536  # the largest sums the GPU tests form (they assert that they stay below)


def worst_case_sensitivity(terms, slices=1, old=False):
    """The smallest possible term (0.25) over the largest possible bound of a sum of `terms` terms of magnitude at most 4 each."""
    return 0.25 / (((terms + 8 + (slices if slices > 1 else 0)) * 4.0 * terms + (4.0 if old else 0.0)) * U * reference_slack())


def values(shape, seed):
    """Magnitudes uniform in [0.5, 2], random signs."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 2.0, shape) * rng.choice([-1.0, 1.0], shape)


def gap_map(count, pitch, first=1):
    """`count` ascending physical columns of a panel of `pitch` columns, starting at `first` (not 0) and with the gaps spread evenly."""
    assert first + count <= pitch
    c = np.arange(count)
    o = first + c + (c * (pitch - first - count)) // max(count, 1)
    assert np.all(np.diff(o) > 0) and o[0] == first and o[-1] < pitch
    return o.astype(np.uint32)


def basis(x=None, w=None, p=None, xmap=None, wx=None):
    """S = [X[:, xmap] | W | P] (float64, n x m); absent parts are None.  Without a map the first wx (default: all) columns of X."""
    parts = []
    if x is not None:
        parts.append(x[:, np.asarray(xmap, dtype=np.int64)] if xmap is not None else x[:, :x.shape[1] if wx is None else wx])
    parts += [a for a in (w, p) if a is not None]
    return np.concatenate(parts, axis=1)


def pack_blocks(c1, c2, m):
    """mh_pack_coefficients: rows 0 .. m - 1 of two matrices (more rows: a larger leading dimension) side by side, k-major."""
    return np.ascontiguousarray(np.concatenate([a[:m] for a in (c1, c2) if a is not None], axis=1))


def pack_stacked(c1, c2, scale):
    """mh_pack_stacked: scale * [c1; c2], k-major."""
    return np.ascontiguousarray(scale * np.concatenate([a for a in (c1, c2) if a is not None], axis=0))


class Product:
    """Z = S Ct in longdouble and |S| |Ct| in double, for the rows `rows` of S (default: all)."""

    def __init__(self, s, ct, rows=None):
        self.rows = np.arange(s.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
        sr = s[self.rows]
        self.m, self.nc = ct.shape
        assert sr.shape[1] == self.m
        self.z = sr.astype(LD) @ ct.astype(LD)
        self.mag = np.abs(sr) @ np.abs(ct)  # (non-negative terms in double: relative error m u, nothing beside the bound's own factor)
        self.min_term = float(np.abs(sr).min() * np.abs(ct[ct != 0]).min()) if sr.size and np.any(ct != 0) else 0.0

    def bound(self, old=None, slices=1):
        """(m + 8) u mag [+ slices u mag] [+ 2 u |old|] (a triangular Ct has fewer terms per column: m still holds)."""
        k = self.m + 8 + (slices if slices > 1 else 0)
        b = k * U * self.mag
        if old is not None:
            b = b + 2 * U * np.abs(old)
        return b * reference_slack()

    def min_term_over_bound(self, **kw):
        return self.min_term / float(self.bound(**kw).max())


def gram_product(x, y, ymap=None):
    """(X^T Y[:, ymap] in longdouble, its bound (n + 8) u |X|^T |Y|, smallest term / largest bound)."""
    ys = y[:, np.asarray(ymap, dtype=np.int64)] if ymap is not None else y
    g = x.astype(LD).T @ ys.astype(LD)
    bound = (x.shape[0] + 8) * U * (np.abs(x).T @ np.abs(ys)) * reference_slack()
    return g, bound, float(np.abs(x).min() * np.abs(ys).min()) / float(bound.max())


def expected_outputs(z, bound, n, n1, ld1, omap=None, col_begin=0, col_count=0, old1=None, old2=None, rows=None):
    """What a launch must leave in out1 (n x ld1) and out2 (n x (nc - n1)): (want1, bound1, want2, bound2).  want is NaN where the
    sentinel must survive -- the columns of out1 that no logical column maps to (the pad column of an odd count among them), and under
    a column range every column outside it.  z and bound cover the rows `rows` (default: all n); the other rows are NaN in `want` too, and
    the caller leaves them out of the comparison.  old1, old2: the accumulate form's start values, in the outputs' own shapes; `bound`
    is then the plain product's, and the start value's 2 u |old| is added here."""
    nc = z.shape[1]
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    cols = np.arange(col_begin, col_begin + col_count) if col_count else np.arange(nc)
    target = np.arange(n1) if omap is None else np.asarray(omap, dtype=np.int64)
    want1, b1 = np.full((n, ld1), np.nan, dtype=LD), np.ones((n, ld1))
    want2, b2 = np.full((n, nc - n1), np.nan, dtype=LD), np.ones((n, nc - n1))
    c1, c2 = cols[cols < n1], cols[cols >= n1]
    for want, b, old, at, c in ((want1, b1, old1, np.ix_(rows, target[c1]), c1), (want2, b2, old2, np.ix_(rows, c2 - n1), c2)):
        want[at] = z[:, c] + (0 if old is None else old[at].astype(LD))
        b[at] = bound[:, c] + (0 if old is None else 2 * U * reference_slack() * np.abs(old[at]))
    return want1, b1, want2, b2


def tile_edge_rows(n, count=2000, seed=0):
    """A fixed sample of about `count` rows of an n-row panel: the first and last 130 rows (both sides of the 64-row tile edges near the
    ends, the clamped last tile among them) and random rows between."""
    edge = np.concatenate([np.arange(min(130, n)), np.arange(max(0, n - 130), n)])
    rnd = np.random.default_rng(seed).integers(0, n, max(0, count - len(edge)))
    return np.unique(np.concatenate([edge, rnd]))
