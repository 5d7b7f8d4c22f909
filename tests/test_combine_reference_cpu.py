"""The host reference of the dense tall products (tests/combine_reference.py) judged on the host: honest float64 evaluations of the same
products stay inside its bounds, each simulated kernel mistake -- a few lines of numpy -- lands outside them, and the inputs make every
single term of a sum at least 100 times the bound of its entry.  No device code runs here."""
import numpy as np
import pytest

from tests import combine_reference as ref

N, B, WA, WW, WP = 200, 80, 53, 21, 19  # rows; X's pitch and mapped columns; W, P: m = 93 (the last K chunk of 16 holds 13)
M = WA + WW + WP
NC, N1 = 40, 20                          # the strip of columns 16 .. 31 straddles n1
LD1 = (N1 + 1) & ~1


@pytest.fixture(scope="module")
def case():
    x, w, p = ref.values((N, B), 1), ref.values((N, WW), 2), ref.values((N, WP), 3)
    xmap = ref.gap_map(WA, B)
    ct = ref.values((M, NC), 4)
    s = ref.basis(x, w, p, xmap)
    return x, w, p, xmap, ct, s, ref.Product(s, ct)


def inside(got, prod, **kw):
    return ref.compare(got, prod.z, prod.bound(**kw))


def test_the_inputs(case):
    x, w, p, xmap, ct, s, prod = case
    for a in (x, w, p, ct):
        assert 0.5 <= np.abs(a).min() and np.abs(a).max() <= 2.0 and (a < 0).any() and (a > 0).any()
    assert xmap[0] > 0 and np.all(np.diff(xmap.astype(np.int64)) >= 1) and (np.diff(xmap.astype(np.int64)) > 1).any() and xmap[-1] < B
    assert s.shape == (N, M) and np.array_equal(s[:, 5], x[:, xmap[5]]) and np.array_equal(s[:, WA], w[:, 0]) and np.array_equal(s[:, M - 1], p[:, -1])


def test_every_term_is_a_hundred_times_the_bound_of_its_entry(case):
    prod = case[6]
    old = ref.values((N, NC), 5)
    assert prod.min_term >= 0.25
    assert prod.min_term_over_bound() >= 100 and prod.min_term_over_bound(old=old) >= 100 and prod.min_term_over_bound(slices=8) >= 100
    # whatever the values drawn, for the largest sums the GPU tests form
    assert ref.worst_case_sensitivity(ref.WIDEST_M, old=True) >= 100
    assert ref.worst_case_sensitivity(ref.WIDEST_M, slices=ref.MOST_SLICES) >= 100
    assert ref.worst_case_sensitivity(ref.MOST_GRAM_ROWS) >= 100
    _, _, sens = ref.gram_product(ref.values((N, 17), 6), ref.values((N, 9), 7))
    assert sens >= 100


# ---- part one: honest products stay inside the bound --------------------------------------------------------------------------------
def chunked(s, ct, chunk=16, k0=0, k1=None):
    """K in chunks of `chunk`, accumulated left to right."""
    out = np.zeros((s.shape[0], ct.shape[1]))
    for k in range(k0, s.shape[1] if k1 is None else k1, chunk):
        e = min(k + chunk, s.shape[1] if k1 is None else k1)
        out = out + s[:, k:e] @ ct[k:e]
    return out


def test_honest_products_stay_inside_the_bound(case):
    _, _, _, _, ct, s, prod = case
    c = inside(s @ ct, prod)
    assert c.ok and 0 < c.worst, c
    assert inside(chunked(s, ct), prod).ok
    kslice = -(-(-(-M // 8)) // 16) * 16  # as the kernel cuts the K range
    sliced = np.zeros((N, NC))
    for q in range(8):
        sliced = sliced + chunked(s, ct, 16, min(M, q * kslice), min(M, (q + 1) * kslice))
    assert inside(sliced, prod, slices=8).ok
    old = ref.values((N, NC), 5)
    assert ref.compare(old + s @ ct, old.astype(ref.LD) + prod.z, prod.bound(old=old)).ok
    # single precision is NOT inside: the bound is not so wide that the precision does not matter
    assert not inside((s.astype(np.float32) @ ct.astype(np.float32)).astype(np.float64), prod).ok


def test_an_honest_gram_by_row_slabs_stays_inside_the_bound(case):
    x, w = case[0], case[1]
    ymap = ref.gap_map(WA, B)
    g, bound, _ = ref.gram_product(w, x, ymap)
    got = np.zeros(g.shape)
    for r0 in range(0, N, 32):
        got = got + w[r0:r0 + 32].T @ x[r0:r0 + 32][:, ymap.astype(np.int64)]
    c = ref.compare(got, g, bound)
    assert c.ok and 0 < c.worst, c


def test_the_packers_are_exact(case):
    ct = case[4]
    ld = M + 3
    full = np.asfortranarray(np.concatenate([ct, ref.values((3, NC), 8)], axis=0))  # column-major with a larger leading dimension
    assert np.array_equal(ref.pack_blocks(full[:, :N1], full[:, N1:], M), ct) and full.shape[0] == ld
    assert np.array_equal(ref.pack_stacked(ct[:WA], ct[WA:], -1.0), -ct)
    assert np.array_equal(ref.pack_stacked(ct, None, -1.0), -ct)


# ---- part two: simulated kernel mistakes fall outside it ----------------------------------------------------------------------------
def every_entry_outside(c):
    return c.outside == c.ratio.size


def test_a_dropped_last_partial_chunk_is_outside(case):
    _, _, _, _, ct, s, prod = case
    assert M % 16
    assert every_entry_outside(inside(chunked(s, ct, 16, 0, M // 16 * 16), prod))


def test_the_first_column_of_w_read_from_x_is_outside(case):
    x, w, p, xmap, ct, s, prod = case
    bad = s.copy()
    bad[:, WA] = x[:, min(int(xmap[-1]) + 1, B - 1)]  # the part boundary one column late: X's next physical column
    assert every_entry_outside(inside(bad @ ct, prod))


def test_an_ignored_xmap_is_outside(case):
    x, w, p, xmap, ct, s, prod = case
    assert every_entry_outside(inside(ref.basis(x, w, p, None, WA) @ ct, prod))


def images(z, n1, ld1, omap=None):
    """The device images of out1 and out2 that storing z leaves, NaN where nothing is stored; and the bitwise untouched masks."""
    o1, o2 = np.full((z.shape[0], ld1), np.nan), z[:, n1:].copy()
    o1[:, np.arange(n1) if omap is None else np.asarray(omap, dtype=np.int64)] = z[:, :n1]
    return o1, o2


def test_an_ignored_omap_and_a_strip_written_wholly_to_out1_are_caught(case):
    _, _, _, _, ct, s, prod = case
    z = s @ ct
    ld = 2 * N1
    omap = ref.gap_map(N1, ld)
    want1, b1, want2, b2 = ref.expected_outputs(prod.z, prod.bound(), N, N1, ld, omap)
    o1, o2 = images(z, N1, ld, omap)
    assert ref.compare(o1, want1, b1, np.isnan(o1)).ok and ref.compare(o2, want2, b2).ok
    o1, _ = images(z, N1, ld, None)
    c = ref.compare(o1, want1, b1, np.isnan(o1))
    assert not c.ok and c.stray > 0 and c.missing > 0
    # the strip of columns 16 .. 31 written wholly to out1 (pitch LD1: its columns 20 .. 31 land in the next row, and past the end),
    # none to out2; rows stored last to first, one of the orders a grid may take
    want1, b1, want2, b2 = ref.expected_outputs(prod.z, prod.bound(), N, N1, LD1)
    flat = np.full(N * LD1 + 16, np.nan)
    o2 = np.full((N, NC - N1), np.nan)
    o2[:, 32 - N1:] = z[:, 32:]
    for r in reversed(range(N)):
        flat[r * LD1:r * LD1 + 32] = z[r, :32]
    o1 = flat[:N * LD1].reshape(N, LD1)
    assert not np.isnan(flat[N * LD1:N * LD1 + 32 - LD1]).any()  # (what the guard behind the panel is for)
    assert not ref.compare(o1, want1, b1, np.isnan(o1)).ok
    c = ref.compare(o2, want2, b2, np.isnan(o2))
    assert c.missing == N * (32 - N1)


def test_accumulate_treated_as_overwrite_is_outside(case):
    _, _, _, _, ct, s, prod = case
    old = ref.values((N, NC), 5)
    want = old.astype(ref.LD) + prod.z
    assert ref.compare(old + s @ ct, want, prod.bound(old=old)).ok
    assert every_entry_outside(ref.compare(s @ ct, want, prod.bound(old=old)))


def test_one_tile_computed_from_the_updated_x_is_outside(case):
    """The in-place hazard: rows 64 .. 127 of X already hold the result when (part of) their product is formed."""
    x = case[0]
    w = 17
    v = np.ascontiguousarray(x[:, :w])
    ct = np.triu(ref.values((w, w), 9))  # Linv, column-major lower triangular, read k-major
    prod = ref.Product(v, ct)
    good = v @ ct
    assert inside(good, prod).ok
    bad = good.copy()
    half = v[64:128].copy()
    half[:, :8] = good[64:128, :8]  # the columns a quicker wave had stored
    bad[64:128] = half @ ct
    c = inside(bad, prod)
    rows = (c.ratio > 1).any(axis=1)
    assert rows[64:128].all() and not rows[:64].any() and not rows[128:].any(), c


def test_an_untransposed_ct_and_a_dropped_pack_scale_are_outside(case):
    _, _, _, _, ct, s, prod = case
    sq = ref.values((M, M), 10)
    psq = ref.Product(s, sq)
    assert inside(s @ sq, psq).ok and every_entry_outside(inside(s @ sq.T, psq))
    neg = ref.Product(s, ref.pack_stacked(ct, None, -1.0))
    assert inside(-(s @ ct), neg).ok and every_entry_outside(inside(s @ ct, neg))


def test_a_gram_written_at_the_wrong_leading_dimension_is_caught(case):
    x, w = case[0], case[1]
    wa, wb, ld, cols = WW, 30, WW + 30, 40  # the block at (wb, 0)... of a G of ld rows: rows 30 .. 50, columns 0 .. 29
    y = np.ascontiguousarray(x[:, :wb])
    g, bound, _ = ref.gram_product(w, y)
    want, b = np.full((ld, cols), np.nan, dtype=ref.LD), np.ones((ld, cols))
    want[30:30 + wa, :wb], b[30:30 + wa, :wb] = g, bound

    def image(pitch):  # column-major storage at leading dimension `pitch`, starting at row 30 of column 0
        flat = np.full(ld * cols, np.nan)
        for j in range(wb):
            flat[30 + j * pitch:30 + j * pitch + wa] = (w.T @ y)[:, j]
        return flat.reshape(cols, ld).T

    good = image(ld)
    assert ref.compare(good, want, b, np.isnan(good)).ok
    bad = image(wa)
    c = ref.compare(bad, want, b, np.isnan(bad))
    assert not c.ok and c.missing > 0 and c.stray > 0


def test_the_sampled_rows_cover_the_tile_edges():
    for n in (65535, 65536):
        rows = ref.tile_edge_rows(n)
        assert 1900 <= len(rows) <= 2100 and rows[0] == 0 and rows[-1] == n - 1
        assert {63, 64, 127, 128, n - 65, n - 64, (n - 1) // 64 * 64 - 1, (n - 1) // 64 * 64} <= set(rows.tolist())
        assert np.array_equal(rows, ref.tile_edge_rows(n))
