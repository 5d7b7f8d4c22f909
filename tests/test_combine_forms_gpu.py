"""Every form of the dense tall products (mesheditor_amd/csrc/mh_dense.hip: mh_combine and mh_short_product on k_combine, mh_gram, the two
coefficient packers) on crafted panels, each against the extended-precision host product of tests/combine_reference.py under the bound
derived there.  The lab entry (tools/lab.py: dense_form) calls the solver's own dispatchers on the caller's arrays, so the launch selection
is the solver's; every output -- and X, which is an output when a call runs in place and must be bit-unchanged otherwise -- comes back
with its guards and with a sentinel in whatever nobody wrote.  Every call is made twice: our own kernels must repeat bit for bit; for the
vendor dgemm branch the outcome is recorded (REPEATS) and not asserted.

Which instantiation a call reaches: k_combine<NT, ACCUMULATE, MAPPED, ALSO> with NT = the even number of 16-column strips that covers the
launch's columns (2 .. 16), accumulate -> <true, false>, a second destination -> <false, true, true>, an xmap -> <false, true>, else
<false, false>; mh_short_product always <false, false> with gridDim.y = slices.  REACHED collects (form, NT) as the tests run.

MH_TEST=own_gemm, which sends the vendor branch's shapes through our kernels, is read once per process and is therefore not toggled
here: the vendor cases run the vendor branch, and the same inputs one row short (n = 65535) run our own kernel."""
import numpy as np
import pytest

from tests import combine_reference as ref
from tools import lab

pytestmark = pytest.mark.gpu
MH_OK, MH_EINVAL = 0, 1
ROWS = (1, 63, 64, 65, 200)  # the tile edge and the clamped last tile
WORST = {}    # form -> worst error / bound seen (information for docs/LAB_NOTEBOOK.md, never a criterion)
REACHED = set()
REPEATS = {}  # vendor case: whether its two calls agreed bit for bit, and whether it equals our own kernel's result (recorded, not asserted)


@pytest.fixture(scope="module")
def ctx():
    from mesheditor_amd import api
    c = api.Context(0)
    yield c
    c.close()
    for form in sorted(WORST):
        print("worst error / bound, %-28s %.3g" % (form, WORST[form]))
    by_form = {}
    for form, nt in sorted(REACHED):
        by_form.setdefault(form, []).append(nt)
    for form, nts in by_form.items():
        print("reached, %-28s NT = %s" % (form, ", ".join(map(str, nts))))
    for what, answer in sorted(REPEATS.items()):
        print("%s: %s" % (what, answer))


@pytest.fixture(scope="module")
def big_n(ctx):
    """64 * 8 * CUs + 100 rows: k_combine's grid is capped at 8 workgroups per CU, so this is the smallest n at which some workgroup is dealt
    a second 64-row tile (and the last tile is a clamped one)."""
    r = lab.dense_form(ctx, "pack", m=1, nc=1, stacked=(np.asfortranarray(np.ones((1, 1))), None, 1.0))
    assert r.rc == MH_OK and r.cu_count > 0
    return 64 * 8 * r.cu_count + 100


_VALUES = {}


def values(shape, seed):
    """ref.values, kept: inputs are shared between cases and never written."""
    key = (tuple(shape), seed)
    if key not in _VALUES:
        _VALUES[key] = ref.values(shape, seed)
        _VALUES[key].setflags(write=False)
    return _VALUES[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def judge(form, got, want, bound, what):
    c = ref.compare(got, want, bound, lab.untouched(got))
    WORST[form] = max(WORST.get(form, 0.0), c.worst if np.isfinite(c.worst) else 0.0)
    assert c.ok, (form, what, c)


def twice(ctx, kind, own=True, case=None, **kw):
    """The call twice on the same inputs: equal status, guards untouched, and (our own kernels) bit-identical outputs.  The first result."""
    a, b = lab.dense_form(ctx, kind, **kw), lab.dense_form(ctx, kind, **kw)
    assert a.rc == b.rc and a.dispatched and b.dispatched, (a.rc, b.rc, a.dispatched)
    same = True
    for k, (body, guards) in a.out.items():
        assert lab.untouched(guards).all() and lab.untouched(b.out[k][1]).all(), (kind, k, "guard written")
        same = same and np.array_equal(bits(body), bits(b.out[k][0]))
        assert same or not own, (kind, k, "not reproducible")
    if not own:
        REPEATS[case + ": two calls bit-identical"] = same
    return a


def reach(form, cols):
    chunks = -(-cols // 256)
    step = (-(-cols // chunks) + 15) // 16 * 16
    for c0 in range(0, cols, step):
        REACHED.add((form, 2 * ((-(-min(step, cols - c0) // 16) + 1) // 2)))


def combine(ctx, form, n, x=None, w=None, p=None, xmap=None, ldx=0, ct=None, stacked=None, blocks=None, n1=None, ld1=0, omap=None, col_begin=0, col_count=0,
            accumulate=False, in_place=0, second=False, rows=None, own=True):
    """One mh_combine call, twice, judged whole: out1 and out2 against the reference (the sentinel wherever nothing may be stored), X
    bit-unchanged -- or, in place, the output --, a second destination bit-equal to out1.  rows: judge these rows only (the pattern of
    written and untouched entries is still checked on every row)."""
    wx = 0 if x is None else len(xmap) if xmap is not None else x.shape[1]
    s = ref.basis(x, w, p, xmap)
    m = s.shape[1]
    assert m <= ref.WIDEST_M
    ctr = ct if ct is not None else ref.pack_stacked(*stacked) if stacked is not None else ref.pack_blocks(blocks[0], blocks[1], m)
    nc = ctr.shape[1]
    n1 = nc if n1 is None else n1
    pitch1 = ld1 or n1
    prod = ref.Product(s, ctr, rows)
    old1 = values((n, pitch1), 101) if accumulate else None
    old2 = values((n, nc - n1), 102) if accumulate and nc > n1 else None
    kw = dict(n=n, x=x, wx=wx, ldx=ldx, w=w, p=p, nc=nc, n1=n1, ld1=ld1, col_begin=col_begin, col_count=col_count, accumulate=accumulate, xmap=xmap, omap=omap,
              ct=ct, blocks=blocks, stacked=stacked, in_place=in_place, old1=old1, old2=old2)
    if second:  # the basis update's second store: into X through the map X is read by, or (in_place 0) into a panel of X's shape
        kw.update(omap_also=xmap, ld1_also=ldx, also=in_place != 2)
    r = twice(ctx, "combine", own=own, case=form, **kw)
    assert r.rc == MH_OK, (form, r.rc)
    if own:
        reach(form, col_count or nc)
    if ct is None:
        assert np.array_equal(bits(r.body("ct")), bits(ctr)), (form, "packed coefficients")
    tag = (form, n, m, nc, n1)
    want1, b1, want2, b2 = ref.expected_outputs(prod.z, prod.bound(), n, n1, (ldx or wx) if in_place == 1 else pitch1, omap, col_begin, col_count, old1, old2, rows)
    sel = slice(None) if rows is None else prod.rows
    got1 = r.body("x") if in_place == 1 else r.body("out1")
    if rows is not None:  # every row: written where the sampled rows are written, untouched where they are not
        written = ~np.isnan(want1[prod.rows[0]].astype(np.float64))
        assert not lab.untouched(got1[:, written]).any() and (accumulate or lab.untouched(got1[:, ~written]).all()), tag
    if in_place == 1:  # X is out1: columns nobody stores keep X's own values
        keep = np.isnan(want1[prod.rows[0]].astype(np.float64))
        assert np.array_equal(bits(got1[:, keep]), bits(x[:, keep])), tag + ("X outside the output columns",)
        judge(form, got1[sel][:, ~keep], want1[sel][:, ~keep], b1[sel][:, ~keep], tag + ("X in place",))
    else:
        if accumulate:  # nothing holds the sentinel: what is not written keeps its start value
            keep = np.isnan(want1.astype(np.float64))
            want1 = np.where(keep, old1.astype(ref.LD), want1)
            b1 = np.where(keep, 0.0, b1)
        judge(form, got1[sel], want1[sel], b1[sel], tag + ("out1",))
    if nc > n1:
        judge(form, r.body("out2")[sel], want2[sel], b2[sel], tag + ("out2",))
        assert rows is None or not lab.untouched(r.body("out2")).any()
    if x is not None and in_place == 0:
        assert np.array_equal(bits(r.body("x")), bits(x)), tag + ("X changed",)
    if second:
        dst = r.body("x") if in_place == 2 else r.body("out1_also")
        cols = np.asarray(xmap, dtype=np.int64)
        src = got1[:, :n1] if omap is None else got1[:, np.asarray(omap, dtype=np.int64)]
        assert np.array_equal(bits(dst[:, cols[:n1]]), bits(src)), tag + ("second destination differs from out1",)
        other = np.ones(dst.shape[1], bool)
        other[cols[:n1]] = False
        if in_place == 2:
            assert np.array_equal(bits(dst[:, other]), bits(x[:, other])), tag + ("X outside the map",)
        else:
            assert lab.untouched(dst[:, other]).all(), tag + ("second destination outside the map",)
    return r


def split3(m):
    """m columns over X, W and P: thirds, the boundaries in the middle of K chunks; fewer parts when m is small."""
    a = m // 3
    return (m, 0, 0) if m < 3 else (a, a, m - 2 * a)


def panels(n, wx, ww, wp, seed=0):
    return tuple(np.ascontiguousarray(values((n, wd), seed + k)) if wd else None for k, wd in enumerate((wx, ww, wp)))


# ---- the plain form -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 15, 16, 17, 31, 32, 33, 47, 48, 49])
def test_plain_k_edges(ctx, m):
    ct = values((m, 33), 10)
    for n in ROWS:
        x, w, p = panels(n, *split3(m))
        combine(ctx, "plain", n, x, w, p, ct=ct, n1=20)


@pytest.mark.parametrize("widths", [(5, 7, 9), (13, 0, 20), (0, 7, 9), (0, 0, 21), (21, 0, 0), (16, 16, 0), (1, 1, 1)])
def test_plain_part_boundaries_and_absent_parts(ctx, widths):
    """Boundaries in the middle of a 16-chunk; an absent part is a null pointer of width 0."""
    ct = values((sum(widths), 20), 11)
    for n in ROWS:
        x, w, p = panels(n, *widths)
        combine(ctx, "plain", n, x, w, p, ct=ct, n1=12)


@pytest.mark.parametrize("nc", [1, 15, 16, 17, 31, 32, 33, 48, 97, 128, 129, 240, 255, 256])
def test_plain_output_widths(ctx, nc):
    """Every NT, and both forms of the last two strips' tails."""
    ct = values((21, nc), 12)
    for n in ROWS:
        x, w, p = panels(n, 5, 7, 9)
        combine(ctx, "plain", n, x, w, p, ct=ct)
        combine(ctx, "plain", n, x, w, p, ct=ct, n1=nc // 2)


@pytest.mark.parametrize("nc,n1", [(40, 0), (40, 40), (40, 16), (40, 32), (40, 20), (40, 17), (40, 31), (97, 50), (255, 129), (256, 255), (17, 1)])
def test_plain_split_across_out1_and_out2(ctx, nc, n1):
    ct = values((21, nc), 13)
    for n in ROWS:
        x, w, p = panels(n, 5, 7, 9)
        combine(ctx, "plain", n, x, w, p, ct=ct, n1=n1)
        combine(ctx, "plain", n, x, w, p, ct=ct, n1=n1, ld1=n1 + 3)  # a pitch wider than the columns: the rest keeps the sentinel


@pytest.mark.parametrize("nc,n1,col_begin,col_count", [(100, 40, 23, 50), (100, 40, 48, 52), (300, 100, 7, 270)])
def test_plain_column_sub_range(ctx, nc, n1, col_begin, col_count):
    """Only columns [col_begin, col_begin + col_count) are computed and stored; the others keep the sentinel.  The solver never passes a
    proper sub-range (every call of mh_combine leaves col_count 0): the argument is tested because the dispatcher offers it."""
    ct = values((21, nc), 14)
    for n in ROWS:
        x, w, p = panels(n, 5, 7, 9)
        combine(ctx, "plain, column range", n, x, w, p, ct=ct, n1=n1, col_begin=col_begin, col_count=col_count)


def test_plain_second_tile_of_a_workgroup(ctx, big_n):
    x, w, p = panels(big_n, 5, 7, 9, seed=20)
    combine(ctx, "plain", big_n, x, w, p, ct=values((21, 20), 15), n1=12)


# ---- accumulate, through mh_pack_stacked with scale -1 ------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [7, 40, 80])
def test_accumulate_the_projection_s_three_calls(ctx, w):
    """W += [X | P] (-H): X alone (all b columns), P alone in the W slot, X and P stacked; the start value of W is not zero."""
    b, wp = w + 3, w
    h, h2 = np.asfortranarray(values((b, w), 16)), np.asfortranarray(values((wp, w), 17))
    for n in ROWS:
        x, pp, _ = panels(n, b, wp, 0, seed=30)
        combine(ctx, "accumulate", n, x, stacked=(h, None, -1.0), accumulate=True)
        combine(ctx, "accumulate", n, None, pp, stacked=(h2, None, -1.0), accumulate=True)
        combine(ctx, "accumulate", n, x, pp, stacked=(h, h2, -1.0), accumulate=True)


# ---- in place, unmapped: the Cholesky-QR call ---------------------------------------------------------------------------------------
def linv(w):
    """Linv as the solver passes it: column-major lower triangular, which k_combine reads k-major (Ct[k][j] = Linv[j][k], zero for k > j)."""
    return np.ascontiguousarray(np.triu(values((w, w), 18)))


@pytest.mark.parametrize("w", [1, 8, 17, 64, 80, 128, 200])
def test_in_place_cholesky_qr(ctx, w):
    for n in ROWS:
        combine(ctx, "in place (QR)", n, panels(n, w, 0, 0, seed=40)[0], ct=linv(w), in_place=1)


def test_in_place_cholesky_qr_second_tile_of_a_workgroup(ctx, big_n):
    combine(ctx, "in place (QR)", big_n, panels(big_n, 17, 0, 0, seed=41)[0], ct=linv(17), in_place=1)


# ---- mapped: the basis update -------------------------------------------------------------------------------------------------------
def basis_update(ctx, n, b, wa, wp_new, second, in_place, seed=50):
    """X_active, P <- [X[:, xmap] | W | P] [Cx | Cp]: X n x b read through an ascending map with gaps that does not start at column 0, out1 a
    compact panel of even pitch (wa odd: a pad column), coefficients through mh_pack_coefficients at leading dimension m as update_basis has them."""
    wp = wa - wp_new  # (P absent where new directions are formed, present where they are not: both occur in a solve)
    x, w, p = panels(n, b, wa, wp, seed=seed)
    m = 2 * wa + wp
    cx = np.asfortranarray(values((m, wa), 19))
    cp = np.asfortranarray(values((m, wp_new), 20)) if wp_new else None
    form = "mapped, second destination" if second else "mapped"
    return combine(ctx, form, n, x, w, p, xmap=ref.gap_map(wa, b), ldx=b, blocks=(cx, cp), n1=wa, ld1=(wa + 1) & ~1, second=second, in_place=in_place)


@pytest.mark.parametrize("b,wa", [(12, 8), (12, 7), (80, 53), (80, 54), (128, 85), (128, 86)])
@pytest.mark.parametrize("wp_new_is_wa", [False, True])
def test_mapped_basis_update_with_the_second_store_into_x(ctx, b, wa, wp_new_is_wa):
    """The basis update's own call: out1_also = X, omap_also = xmap, while other workgroups still read X."""
    for n in ROWS:
        basis_update(ctx, n, b, wa, wa if wp_new_is_wa else 0, second=True, in_place=2)


@pytest.mark.parametrize("b,wa", [(12, 7), (130, 87), (130, 86)])
@pytest.mark.parametrize("wp_new_is_wa", [False, True])
def test_mapped_basis_update_without_a_second_destination(ctx, b, wa, wp_new_is_wa):
    for n in ROWS:
        basis_update(ctx, n, b, wa, wa if wp_new_is_wa else 0, second=False, in_place=0)


def test_mapped_second_destination_apart_from_x(ctx):
    for n in ROWS:
        basis_update(ctx, n, 80, 53, 53, second=True, in_place=0)


def test_mapped_with_an_output_map(ctx):
    """An omap of the caller's on out1 (no call of the solver passes one today): out1's columns through a map with gaps."""
    for n in ROWS:
        x, w, p = panels(n, 40, 9, 0, seed=51)
        combine(ctx, "mapped", n, x, w, p, xmap=ref.gap_map(25, 40), ldx=40, ct=values((34, 30), 21), n1=21, ld1=36, omap=ref.gap_map(21, 36, first=2))


@pytest.mark.parametrize("wp_new", [0, 8])
def test_mapped_basis_update_second_tile_of_a_workgroup(ctx, big_n, wp_new):
    """Nothing of a later tile may be fetched before the tile's stores: here workgroups are dealt a second tile of the X they write."""
    basis_update(ctx, big_n, 12, 8, wp_new, second=True, in_place=2, seed=52)


# ---- every strip count of every form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [2, 4, 6, 8, 10, 12, 14, 16])
def test_every_strip_count_of_every_form(ctx, nt):
    """The widths above follow the solver's shapes and leave some NT of some forms out (the plain form's 6, 12 and 14 among them): here
    nc = 16 NT - 5 -- the last strip partial, the one before it full -- through all four instantiations, split inside a strip."""
    nc = 16 * nt - 5
    wa = nc - 20  # mapped: all but the last 20 columns are X's new active columns
    b = wa + wa // 2 + 2
    ct, ctm = values((21, nc), 24), values((wa + 16, nc), 25)
    for n in (65, 200):
        x, w, p = panels(n, 5, 7, 9)
        xm = panels(n, b, 0, 0, seed=53)[0]
        xmap = ref.gap_map(wa, b)
        combine(ctx, "plain", n, x, w, p, ct=ct, n1=wa)
        combine(ctx, "accumulate", n, x, w, p, ct=ct, n1=wa, accumulate=True)
        combine(ctx, "mapped", n, xm, w, p, xmap=xmap, ldx=b, ct=ctm, n1=wa, ld1=(wa + 1) & ~1)
        combine(ctx, "mapped, second destination", n, xm, w, p, xmap=xmap, ldx=b, ct=ctm, n1=wa, ld1=(wa + 1) & ~1, second=True, in_place=2)


# ---- more than 256 output columns ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [257, 300, 513])
def test_more_than_256_output_columns(ctx, nc):
    """The column-chunk loop: c0 != 0 and the 16-rounded step; a split inside a chunk, and at the chunk edge."""
    x, w, p = panels(200, 5, 7, 9)
    ct = values((21, nc), 22)
    step = (-(-nc // -(-nc // 256)) + 15) // 16 * 16
    for n1 in (nc, nc // 2 + 3, step, 0):
        combine(ctx, "plain, column chunks", 200, x, w, p, ct=ct, n1=n1)
    xm = panels(200, 30, 0, 0, seed=53)[0]
    combine(ctx, "mapped, column chunks", 200, xm, w, p, xmap=ref.gap_map(5, 30), ldx=30, ct=ct, n1=nc // 2 + 3)
    combine(ctx, "accumulate, column chunks", 200, x, w, p, ct=ct, n1=nc // 2 + 3, accumulate=True)


# ---- the vendor branch --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain", "mapped", "accumulate"])
def test_vendor_branch_and_the_same_inputs_one_row_short(ctx, name):
    """m = 401 >= 400, nc = 129 >= 128, n = 65536: the vendor dgemm branch (k_spread_rows for the mapped case: xmap given, no omap; beta = 1
    from the first call on under accumulate); the first 65535 rows of the same inputs: our own kernel.  Both judged on ref.tile_edge_rows."""
    n, mapped = 65536, name == "mapped"
    wx, ldx, ww, wp = (100, 150, 160, 141) if mapped else (135, 0, 135, 131)
    x, w, p = panels(n, ldx or wx, ww, wp, seed=60)
    kw = dict(xmap=ref.gap_map(wx, ldx) if mapped else None, ldx=ldx, ct=values((401, 129), 23), n1=wx if mapped else 60, accumulate=name == "accumulate")
    vendor = combine(ctx, "vendor branch, " + name, n, x, w, p, rows=ref.tile_edge_rows(n), own=False, **kw)
    n -= 1
    ours = combine(ctx, name, n, x[:n], w[:n], p[:n], rows=ref.tile_edge_rows(n), **kw)
    # (information: the two paths round differently, so equal bits throughout would mean the larger call did not take the vendor branch)
    REPEATS["vendor branch, " + name + ": equal to our kernel's bits"] = bool(np.array_equal(bits(vendor.body("out1")[:n]), bits(ours.body("out1"))))


# ---- the short product --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [6, 16, 17, 100, 390])
def test_short_product(ctx, m):
    """n = m as in the coarse solve.  m = 6 in 8 slices: an empty K slice still stores its zeros."""
    a = np.ascontiguousarray(values((m, m), 70))
    for nc in (1, 3, 64, 80, 81, 256):
        ct = values((m, nc), 71)
        prod = ref.Product(a, ct)
        for slices in (1, ref.MOST_SLICES):
            r = twice(ctx, "short_product", n=m, x=a, ct=ct, nc=nc, slices=slices)
            assert r.rc == MH_OK
            REACHED.add(("short product", 2 * ((-(-nc // 16) + 1) // 2)))
            assert np.array_equal(bits(r.body("x")), bits(a))
            judge("short product, %d slice%s" % (slices, "s" if slices > 1 else ""), r.body("out1"), prod.z, prod.bound(slices=slices), (m, nc, slices))
            if slices > 1:
                part = r.body("partial")
                assert not lab.untouched(part).any(), (m, nc, "a slice stored nothing")
                kslice = -(-(-(-m // slices)) // 16) * 16
                for q in range(slices):
                    assert (q * kslice < m) or not part[q].any(), (m, nc, q, "an empty slice is not zero")
                total = np.zeros((m, nc))
                for q in range(slices):
                    total = total + part[q]
                assert np.array_equal(bits(total), bits(r.body("out1"))), (m, nc, "the slices' sum, in order")


def test_short_product_refuses_more_than_256_columns(ctx):
    a = np.ascontiguousarray(values((17, 17), 70))
    for slices in (1, 8):
        r = twice(ctx, "short_product", n=17, x=a, ct=values((17, 257), 71), nc=257, slices=slices)
        assert r.rc == MH_EINVAL and all(lab.untouched(body).all() for body, _ in r.out.values())


# ---- the Gram product ---------------------------------------------------------------------------------------------------------------
def gram(ctx, n, wa, wb, mapped, form=None, sample=None, own=True, xy=None):
    """G block = X^T Y[:, ymap] as the solver's mh_gram(ctx, n, W, w, AX, wa, gA + wa, m, b, idx_d): Y at a pitch wider than its columns (and
    through a map), the block in the interior of a larger G whose other entries keep the sentinel.  sample: judge these rows of the
    block only (columns of X: the reference of a long panel is formed for them alone); the others must still be written."""
    assert n <= ref.MOST_GRAM_ROWS
    ldy = wb + wb // 2 + 2 if mapped else wb + 3
    x, y = xy if xy is not None else panels(n, wa, ldy, 0, seed=80)[:2]
    ymap = ref.gap_map(wb, ldy) if mapped else None
    r0, c0, ld, cols = 3, 2, wa + 8, wb + 5
    form = form or ("gram, mapped" if mapped else "gram")
    r = twice(ctx, "gram", own=own, case=form, n=n, x=x, w=y, ww=wb, ldy=ldy, ymap=ymap, ld=ld, g_cols=cols, g_row0=r0, g_col0=c0)
    assert r.rc == MH_OK
    rows = np.arange(wa) if sample is None else np.asarray(sample)
    g, bound, _ = ref.gram_product(np.ascontiguousarray(x[:, rows]), y if mapped else y[:, :wb], ymap)
    want, b = np.full((ld, cols), np.nan, dtype=ref.LD), np.ones((ld, cols))
    want[r0 + rows, c0:c0 + wb], b[r0 + rows, c0:c0 + wb] = g, bound
    got = np.ascontiguousarray(r.body("g"))
    block = np.zeros((ld, cols), bool)
    block[r0:r0 + wa, c0:c0 + wb] = True
    assert not lab.untouched(got[block]).any() and lab.untouched(got[~block]).all(), (form, n, wa, wb, "the block and nothing else is written")
    judged = np.zeros(ld, bool)
    judged[r0 + rows] = True
    judged[:r0] = judged[r0 + wa:] = True
    judge(form, np.ascontiguousarray(got[judged]), want[judged], b[judged], (n, wa, wb, mapped))
    assert np.array_equal(bits(r.body("x")), bits(x))
    return r


@pytest.mark.parametrize("wa,wb,mapped", [(80, 53, True), (80, 53, False), (80, 80, True), (80, 80, False), (161, 97, True), (161, 97, False), (97, 161, True),
                                          (97, 161, False), (200, 129, True), (1, 1, False), (17, 5, True)])
def test_gram_into_the_interior_of_a_larger_matrix(ctx, wa, wb, mapped):
    """Widths either side of the dispatcher's cuts (160 columns on the long side, 96 on the short one, the even cut of a short remainder)."""
    for n in (1, 31, 200):
        gram(ctx, n, wa, wb, mapped)


def test_gram_ragged_last_row_range_of_many_workgroups(ctx):
    """20 011 rows: 313 workgroups of 64 rows -- two staged steps each -- and a last one of 43: one full step and a clamped one of 11."""
    gram(ctx, 20011, 33, 21, True)
    gram(ctx, 20011, 33, 21, False)


def test_gram_vendor_branch_and_the_same_inputs_one_row_short(ctx):
    """wa, wb >= 128 and n = 65536 without a map: the vendor's batched dgemm over 128 row slabs and k_gram_reduce; the first 65535 rows
    of the same panels: our own kernel, cut 160 + 16-rounded rest by two.  Judged on a sample of G's rows (the reference of all 130 x
    129 sums of 65 536 terms would take a minute); every entry of the block must be written."""
    n, wa, wb = ref.MOST_GRAM_ROWS, 130, 129
    x, y, _ = panels(n, wa, wb + 3, 0, seed=81)
    sample = [0, 15, 16, 64, 127, 129]
    gram(ctx, n, wa, wb, False, form="vendor branch, gram", sample=sample, own=False, xy=(x, y))
    gram(ctx, n - 1, wa, wb, False, sample=sample, xy=(x[:n - 1], y[:n - 1]))


# ---- the packers alone --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,a,b", [(1, 1, 0), (21, 7, 9), (93, 53, 0), (93, 0, 53), (300, 129, 257)])
def test_packers(ctx, m, a, b):
    ld = m + 3
    c1 = np.asfortranarray(values((ld, a), 90)) if a else None
    c2 = np.asfortranarray(values((ld, b), 91)) if b else None
    r = twice(ctx, "pack", m=m, nc=a + b, blocks=(c1, c2))
    assert r.rc == MH_OK and np.array_equal(bits(r.body("ct")), bits(ref.pack_blocks(c1, c2, m)))
    s1 = np.asfortranarray(values((a, m), 92)) if a else None
    s2 = np.asfortranarray(values((b, m), 93)) if b else None
    for scale in (-1.0, 1.0, 0.3):
        r = twice(ctx, "pack", m=a + b, nc=m, stacked=(s1, s2, scale))
        assert r.rc == MH_OK and np.array_equal(bits(r.body("ct")), bits(ref.pack_stacked(s1, s2, scale)))


# ---- host refusals ------------------------------------------------------------------------------------------------------------------
def refused(ctx, **kw):
    """The dispatcher itself (dispatched) answers MH_EINVAL; every host array is as passed: the sentinel, or accumulate's start values."""
    r = twice(ctx, "combine", **kw)
    assert r.rc == MH_EINVAL and r.dispatched, (r.rc, r.dispatched)
    for k, (body, _) in r.out.items():
        start = kw.get({"out1": "old1", "out2": "old2"}.get(k))
        assert np.array_equal(bits(body), bits(start)) if start is not None else lab.untouched(body).all(), (k, "written by a refused call")


REFUSALS = {
    "a second destination without maps": dict(in_place=2, ld1_also=30),
    "a second destination without its own map": dict(in_place=2, ld1_also=30, xmap=ref.gap_map(20, 30)),
    "a second destination with accumulate": dict(in_place=2, ld1_also=30, xmap=ref.gap_map(20, 30), omap_also=ref.gap_map(20, 30), accumulate=True),
    "a second destination with more than 256 columns": dict(in_place=2, ld1_also=30, xmap=ref.gap_map(20, 30), omap_also=ref.gap_map(20, 30), nc=257),
    "maps with accumulate": dict(xmap=ref.gap_map(20, 30), accumulate=True),
    "a column range past the last column": dict(col_begin=30, col_count=11),
    "more than 1024 mapped output columns without an omap": dict(xmap=ref.gap_map(20, 30), nc=1030, n1=1025, ld1=1026),
}


@pytest.mark.parametrize("why", sorted(REFUSALS))
def test_the_dispatcher_refuses_on_the_host_and_nothing_is_written(ctx, why):
    kw = dict(REFUSALS[why])
    n, nc = 65, kw.pop("nc", 40)
    n1 = kw.pop("n1", 20)
    x = np.ascontiguousarray(values((n, 30), 94))
    mapped = "xmap" in kw
    m = 20 + 9 if mapped else 30 + 9
    old = dict(old1=values((n, kw.get("ld1", n1)), 95), old2=values((n, nc - n1), 96)) if kw.get("accumulate") else {}
    refused(ctx, n=n, x=x, ldx=30 if mapped else 0, w=np.ascontiguousarray(values((n, 9), 97)), ct=values((m, nc), 98), nc=nc, n1=n1, **old, **kw)
