"""The host reference of the sparse block product (tests/spmm_reference.py) judged on the host: its bounds are neither vacuous (each
simulated kernel mistake on the crafted matrix lands outside them) nor too tight (honest float64 and float32 products, summed in
random order, stay inside).  No device code runs here."""
import numpy as np
import pytest

from tests import spmm_reference as ref

W = 34  # columns used here (even: a mapped launch's pitch)


@pytest.fixture(scope="module")
def case():
    m = ref.crafted()
    x = ref.panel(3 * m.n, W, 5)
    return m, x, ref.Products(m, x), ref.Products(m, x, single=True)


def test_the_crafted_matrices_are_what_the_kernels_need(case):
    m = case[0]
    assert m.n == 261 and m.n % 8 and set(ref.SPECIAL_LENGTHS) <= set(m.lengths.tolist())
    for mat in (m, ref.one_node(), ref.seven_nodes()):
        for i in range(mat.n):
            c = mat.col[mat.row_ptr[i]:mat.row_ptr[i + 1]].astype(np.int64)
            assert np.all(np.diff(c) > 0) and (len(c) == 0 or c.max() < mat.n)
    assert ref.one_node().n == 1 and ref.seven_nodes().n == 7
    a = np.abs(m.vals)
    assert a.min() >= 1e-3 and a.max() <= 1e3 and (m.vals < 0).any() and (m.vals > 0).any()
    # non-symmetric blocks, the diagonal ones included: a transposed read shows in every block
    assert np.abs(m.vals - m.vals.transpose(0, 2, 1)).reshape(len(a), -1).max(axis=1).min() > 0
    # the panel is float-representable, and cancellation is present: |A x| is far below |A| |x| somewhere
    x, p = case[1], case[2]
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.nanmin(np.abs(p.ax) / p.abs_ax) < 1e-3


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_honest_products_stay_inside_the_bound(case, seed):
    m, x, p64, p32 = case
    order = np.random.default_rng(seed).permutation(len(m.col))
    got = ref.block_product(m, m.vals, x, dtype=np.float64, order=order)
    c = ref.compare(got, p64.ax, p64.bound_a(W))
    assert c.ok and 0 < c.worst, c
    got = ref.block_product(m, ref.mass_blocks(m), x, dtype=np.float64, order=order)
    c = ref.compare(got, p64.mx, p64.bound_m(W))
    assert c.ok, c
    got = ref.block_product(m, m.vals32, x.astype(np.float32), dtype=np.float32, order=order)
    assert got.dtype == np.float32
    c = ref.compare(got, p32.ax, p32.bound_a(W))
    assert c.ok and 0 < c.worst, c
    # a float32 product is NOT inside the double-precision bound: the bound is not so wide that the precision does not matter
    assert not ref.compare(got, p64.ax, p64.bound_a(W)).ok


def _rows_outside(c, m, rows):
    """Every node in `rows` has an entry outside the bound."""
    bad = (c.ratio > 1).reshape(m.n, -1).any(axis=1)
    return bool(bad[rows].all())


def test_a_dropped_last_block_is_outside_the_bound(case):
    m, x, p64, p32 = case
    rows = np.flatnonzero(m.lengths > 0)
    bad = m.copy()
    last = bad.row_ptr[rows + 1].astype(np.int64) - 1
    bad.vals[last] = 0.0
    c = ref.compare(ref.block_product(bad, bad.vals, x, dtype=np.float64), p64.ax, p64.bound_a(W))
    assert _rows_outside(c, m, rows), c
    assert not ref.compare(ref.block_product(bad, bad.vals.astype(np.float32), x.astype(np.float32), dtype=np.float32), p32.ax, p32.bound_a(W)).ok
    bad.mass[last] = 0.0
    c = ref.compare(ref.block_product(bad, ref.mass_blocks(bad), x, dtype=np.float64), p64.mx, p64.bound_m(W))
    assert _rows_outside(c, m, rows), c


def test_a_dropped_first_block_of_the_second_strip_is_outside_the_bound(case):
    m, x, p64, p32 = case
    rows = np.flatnonzero(m.lengths > 64)
    assert len(rows) >= 8
    bad = m.copy()
    bad.vals[bad.row_ptr[rows].astype(np.int64) + 64] = 0.0
    c = ref.compare(ref.block_product(bad, bad.vals, x, dtype=np.float64), p64.ax, p64.bound_a(W))
    assert _rows_outside(c, m, rows) and not (c.ratio > 1).reshape(m.n, -1).any(axis=1)[m.lengths <= 64].any(), c
    assert not ref.compare(ref.block_product(bad, bad.vals.astype(np.float32), x.astype(np.float32), dtype=np.float32), p32.ax, p32.bound_a(W)).ok


def test_a_transposed_block_is_outside_the_bound(case):
    m, x, p64, p32 = case
    # one block alone, the DIAGONAL-most one of a long row (symmetric in the solver's matrices, not here)
    for p in (0, int(m.row_ptr[m.n - 1]) + 100, len(m.col) - 1):
        bad = m.copy()
        bad.vals[p] = bad.vals[p].T.copy()
        c = ref.compare(ref.block_product(bad, bad.vals, x, dtype=np.float64), p64.ax, p64.bound_a(W))
        assert _rows_outside(c, m, [m.row_of[p]]) and c.outside <= 3 * W, (p, c)
    bad = m.copy()
    bad.vals = bad.vals.transpose(0, 2, 1).copy()
    assert not ref.compare(ref.block_product(bad, bad.vals.astype(np.float32), x.astype(np.float32), dtype=np.float32), p32.ax, p32.bound_a(W)).ok


def test_the_neighbouring_block_s_mass_is_outside_the_bound(case):
    m, x, p64, _ = case
    rows = np.flatnonzero(m.lengths > 0)
    c = ref.compare(ref.block_product(m, ref.mass_blocks(m, np.roll(m.mass, -1)), x, dtype=np.float64), p64.mx, p64.bound_m(W))
    assert _rows_outside(c, m, rows), c


def test_a_mapped_column_one_off_is_caught(case):
    m, x, p64, _ = case
    wreal, ldy = W - 1, 2 * W
    omap = (np.arange(W) + np.arange(W) // 3).astype(np.int64)  # strictly increasing with gaps
    want, bound = ref.mapped_expectation(p64.ax, p64.bound_a(W), omap, wreal, ldy)
    y = ref.block_product(m, m.vals, x, dtype=np.float64)

    def device_image(target):
        out = np.full((3 * m.n, ldy), np.nan)
        out[:, target[:wreal]] = y[:, :wreal]
        return out, np.isnan(out)

    good, untouched = device_image(omap)
    assert ref.compare(good, want, bound, untouched).ok
    for c, shift in ((5, 1), (5, -1), (2, 1), (wreal - 1, 1)):
        target = omap.copy()
        target[c] += shift
        got, untouched = device_image(target)
        cmp = ref.compare(got, want, bound, untouched)
        assert not cmp.ok and (cmp.stray > 0 or cmp.outside > 0), (c, shift, cmp)
    # the pad column written (wreal odd: the lane's second entry) is a stray write
    target = omap.copy()
    got, untouched = device_image(target)
    got[:, omap[wreal]] = y[:, wreal]
    assert ref.compare(got, want, bound, np.isnan(got)).stray == 3 * m.n


def test_the_neighbouring_column_s_theta_is_outside_the_residual_bound(case):
    m, x, _, _ = case
    theta = 10.0 ** np.random.default_rng(9).uniform(0, 4, W)
    y = ref.block_product(m, m.vals, x, dtype=np.float64)
    y2 = ref.block_product(m, ref.mass_blocks(m), x, dtype=np.float64)
    want, bound = ref.residual_exact(y, y2, theta), ref.residual_bound(y, y2, theta)
    assert ref.compare(y - theta[None, :] * y2, want, bound).ok
    c = ref.compare(y - np.roll(theta, -1)[None, :] * y2, want, bound)
    nonempty = np.repeat(m.lengths > 0, 3)
    assert (c.ratio > 1)[nonempty].all(), c


def test_the_carried_bounds_of_unstored_columns(case):
    """Columns past wreal have no stored y, y2: an honest float64 residual and partial stay inside the bounds carried from the product's,
    the neighbouring theta does not."""
    m, x, p64, _ = case
    theta = 10.0 ** np.random.default_rng(9).uniform(0, 2, W)
    y = ref.block_product(m, m.vals, x, dtype=np.float64)
    y2 = ref.block_product(m, ref.mass_blocks(m), x, dtype=np.float64)
    r, br, pm, bpm = ref.unstored_residual(p64, theta, W, None)
    assert ref.compare(y - theta[None, :] * y2, r, br).ok
    assert ref.compare((y2 * y2).reshape(m.n, 3, W).sum(axis=1), pm, bpm).ok
    assert not ref.compare(y - np.roll(theta, -1)[None, :] * y2, r, br).ok
    assert not ref.compare((y * y).reshape(m.n, 3, W).sum(axis=1), pm, bpm).ok


@pytest.mark.parametrize("weighted", [False, True])
def test_the_partial_sums_bound(case, weighted):
    m, x, _, _ = case
    rng = np.random.default_rng(10)
    dinv = 10.0 ** rng.uniform(-3, 0, 3 * m.n)
    r = ref.block_product(m, m.vals, x, dtype=np.float64)
    wgt = dinv if weighted else np.ones(3 * m.n)
    honest = np.zeros((m.n, W))
    for i in range(3):  # the kernel's order: row after row of the node
        honest = honest + wgt[i::3, None] * (r[i::3] * r[i::3])
    want = ref.partial_exact(r, dinv if weighted else None)
    assert ref.compare(honest, want, ref.partial_bound(want)).ok
    if weighted:  # dinv of row i taken as that of row 3 * node
        wrong = (np.repeat(dinv[0::3], 3)[:, None] * r * r).reshape(m.n, 3, W).sum(axis=1)
        c = ref.compare(wrong, want, ref.partial_bound(want))
        assert (c.ratio > 1)[m.lengths > 0].all(), c


def test_the_chebyshev_bounds(case):
    m = case[0]
    rng = np.random.default_rng(12)
    f32 = np.float32
    d, r, xs = (ref.panel(3 * m.n, 20, s, scale).astype(f32) for s, scale in ((20, 1.0), (21, 300.0), (22, 1.0)))
    dinv = (10.0 ** rng.uniform(-3, 0, 3 * m.n)).astype(f32)
    c1, c2 = f32(0.3), f32(0.7)
    (rn, br), (dn, bd), (xn, bx) = ref.chebyshev_reference(m, d, r, xs, dinv, c1, c2)
    order = rng.permutation(len(m.col))

    def step(vals32, dinv_rows):
        t = ref.block_product(m, vals32, d, dtype=f32, order=order)
        r1 = r - t
        d1 = c1 * d + (c2 * dinv_rows)[:, None] * r1
        return r1, d1, xs + d1

    r1, d1, x1 = step(m.vals32, dinv)
    assert r1.dtype == d1.dtype == x1.dtype == f32
    assert ref.compare(r1, rn, br).ok and ref.compare(d1, dn, bd).ok and ref.compare(x1, xn, bx).ok
    # dinv of row 3 * node for all three rows: r' is still right, d' and x' are not
    r1, d1, x1 = step(m.vals32, np.repeat(dinv[0::3], 3))
    assert ref.compare(r1, rn, br).ok and not ref.compare(d1, dn, bd).ok and not ref.compare(x1, xn, bx).ok
    # a transposed operator: everything is wrong
    r1, d1, x1 = step(m.vals32.transpose(0, 2, 1).copy(), dinv)
    assert not ref.compare(r1, rn, br).ok and not ref.compare(d1, dn, bd).ok and not ref.compare(x1, xn, bx).ok
