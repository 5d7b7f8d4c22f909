"""Every form of the BSR 3x3 product (mesheditor_amd/csrc/mh_spmm.hip) on crafted matrices, each against the extended-precision host
product of tests/spmm_reference.py under the bound derived there: the plain double-precision forms (A, M, and both in one launch), the
single-precision and mixed forms, the column-mapped form with and without its residual epilogue, and the fused Chebyshev step.  The
lab entry (tools/lab.py: spmm_form) calls the product's own dispatchers on the caller's arrays, so the launch selection is the
solver's; every output comes back with its guards and with a sentinel in whatever nobody wrote.  Every call is made twice and must
repeat bit for bit (the kernels promise a fixed fold order).

Which kernel a width reaches (launch_spmm, launch_spmm_wide): double precision, aligned, even w <= 128: k_spmm_wide V = 2 with CL = 8
(w <= 16), 16 (<= 32), 32 (<= 64), 64; odd w <= 16: k_spmm_wide V = 1 (CL = 8, 16); everything else, and every even width behind the
misalignment switch above 16 columns: k_spmm with (CW, NC) = (64, 1) up to 64 columns, (64, 2) up to 128, (64, 3) up to 192, (64, 4)
beyond.  k_spmm's CW = 8 form cannot be reached: V = 1 of the wide kernel takes every width up to 16 first.  The UR = 4 / PRE
instantiations behind latency_bound_level are switched off at compile time, cannot be reached and are not tested here."""
import numpy as np
import pytest

from tests import spmm_reference as ref
from tools import lab

pytestmark = pytest.mark.gpu
MH_OK, MH_EINVAL = 0, 1
MATRICES = ("crafted", "one_node", "seven_nodes")
WORST = {}  # form -> worst error / bound seen (information for docs/LAB_NOTEBOOK.md, never a criterion)


@pytest.fixture(scope="module")
def ctx():
    from mesheditor_amd import api
    c = api.Context(0)
    yield c
    c.close()
    for form in sorted(WORST):
        print("worst error / bound, %-22s %.3f" % (form, WORST[form]))


@pytest.fixture(scope="module")
def cases():
    """Per matrix: the matrix, the widest panel, and the reference products for double- and single-precision operators (computed once)."""
    out = {}
    for k, name in enumerate(MATRICES):
        m = getattr(ref, name)()
        x = ref.panel(3 * m.n, ref.WIDEST, 40 + k)
        out[name] = (m, x, ref.Products(m, x), ref.Products(m, x, single=True))
    return out


@pytest.fixture(scope="module")
def cheb_cases():
    f32 = np.float32
    out = {}
    for k, name in enumerate(MATRICES):
        m = getattr(ref, name)()
        d, r, xs = (ref.panel(3 * m.n, 256, 60 + 3 * k + j, scale).astype(f32) for j, scale in enumerate((1.0, 300.0, 1.0)))
        dinv = (10.0 ** np.random.default_rng(70 + k).uniform(-3, 0, 3 * m.n)).astype(f32)
        c1, c2 = f32(0.3), f32(0.7)
        out[name] = (m, d, r, xs, dinv, c1, c2, ref.chebyshev_reference(m, d, r, xs, dinv, c1, c2))
    return out


def _bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def run(ctx, form, m, x, expect_rc=MH_OK, **kw):
    """The form twice on the same inputs: equal status, bit-identical outputs; guards untouched.  (rc, taken, out) of the first call."""
    rc, taken, out = lab.spmm_form(ctx, form, m.row_ptr, m.col, x, **kw)
    rc2, taken2, out2 = lab.spmm_form(ctx, form, m.row_ptr, m.col, x, **kw)
    assert rc == rc2 == expect_rc and taken == taken2, (form, rc, rc2, expect_rc)
    for k, (body, guards) in out.items():
        assert np.array_equal(_bits(body), _bits(out2[k][0])), (form, k, "not reproducible")
        assert lab.spmm_untouched(guards).all() and lab.spmm_untouched(out2[k][1]).all(), (form, k, "guard written")
    return rc, taken, {k: v[0] for k, v in out.items()}


def judge(form, got, want, bound, what):
    c = ref.compare(got, want, bound, lab.spmm_untouched(got))
    WORST[form] = max(WORST.get(form, 0.0), c.worst if np.isfinite(c.worst) else 0.0)
    assert c.ok, (form, what, c)


def all_untouched(out):
    return all(lab.spmm_untouched(a).all() for a in out.values())


# ---- the plain double-precision forms ---------------------------------------------------------------------------------------------
F64_WIDTHS = (1, 2, 3, 5, 15, 16, 17, 33, 64, 65, 97, 127, 128, 129, 130, 192, 193, 240, 256)


@pytest.mark.parametrize("w,misalign", [(w, False) for w in F64_WIDTHS] + [(w, True) for w in F64_WIDTHS if w % 2 == 0])
def test_double_precision_a_m_and_both(ctx, cases, w, misalign):
    for name in MATRICES:
        m, x, p, _ = cases[name]
        xw = np.ascontiguousarray(x[:, :w])
        tag = (name, w, misalign)
        _, _, out = run(ctx, "f64_a", m, xw, vals9=m.vals, misalign=misalign)
        judge("fp64 A", out["y"], p.ax[:, :w], p.bound_a(w), tag)
        _, _, out = run(ctx, "f64_m", m, xw, mscal=m.mass, misalign=misalign)
        judge("fp64 M", out["y2"], p.mx[:, :w], p.bound_m(w), tag)
        _, _, out = run(ctx, "f64_am", m, xw, vals9=m.vals, mscal=m.mass, misalign=misalign)
        judge("fp64 A and M", out["y"], p.ax[:, :w], p.bound_a(w), tag + ("y",))
        judge("fp64 A and M", out["y2"], p.mx[:, :w], p.bound_m(w), tag + ("y2",))


# ---- single precision and mixed ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [4, 8, 20, 32, 36, 64, 76, 80, 84, 128, 200, 256, 7, 30, 260])
def test_single_precision_a(ctx, cases, w):
    """Multiples of 4 up to 256: the wide kernel (76 and 80: 20 lanes x 3 groups); 7: its one-entry-per-lane form; 30 and 260: k_spmm."""
    for name in MATRICES:
        m, x, _, p = cases[name]
        _, _, out = run(ctx, "f32_a", m, np.ascontiguousarray(x[:, :w]).astype(np.float32), vals9=m.vals32)
        assert out["y"].dtype == np.float32
        judge("fp32 A", out["y"], p.ax[:, :w], p.bound_a(w), (name, w))


@pytest.mark.parametrize("w", [4, 32, 76, 80, 128, 256])
def test_mixed_precision(ctx, cases, w):
    for name in MATRICES:
        m, x, p, _ = cases[name]
        _, _, out = run(ctx, "mixed", m, np.ascontiguousarray(x[:, :w]).astype(np.float32), vals9=m.vals)
        judge("mixed", out["y"], p.ax[:, :w], p.bound_a(w), (name, w))


@pytest.mark.parametrize("w", [1, 6, 30, 258])
def test_mixed_precision_refuses_a_pitch_that_is_no_multiple_of_four(ctx, cases, w):
    m, x, _, _ = cases["crafted"]
    _, _, out = run(ctx, "mixed", m, np.ascontiguousarray(x[:, :w]).astype(np.float32), expect_rc=MH_EINVAL, vals9=m.vals)
    assert all_untouched(out)


# ---- the column-mapped form -------------------------------------------------------------------------------------------------------
def _omap(w, ldy, gaps):
    """Identity, or strictly increasing with ldy - w gaps spread over the columns."""
    c = np.arange(w)
    o = c + (c + 1) * (ldy - w) // (w + 1) if gaps else c
    assert np.all(np.diff(o) > 0) and o[-1] < ldy and (not gaps or o[-1] > w - 1)
    return o.astype(np.uint32)


def _wreals(w):
    out = {1, max(1, (w // 2) | 1 if w > 2 else 1), w - 1, w}
    if w > 128:  # mh_spmm_mapped: column ranges of `step` columns
        ranges = -(-w // 128)
        step = (-(-w // ranges) + 1) & ~1
        out |= {step - 3, step, step + 5}
    return sorted(v for v in out if 1 <= v <= w)


def _check_mapped(form, out, p, w, wreal, omap, ldy, tag):
    want, bound = ref.mapped_expectation(p.ax[:, :w], p.bound_a(w), omap.astype(np.int64), wreal, ldy)
    judge(form, out["y"], want, bound, tag + ("y",))
    want, bound = ref.mapped_expectation(p.mx[:, :w], p.bound_m(w), omap.astype(np.int64), wreal, ldy)
    judge(form, out["y2"], want, bound, tag + ("y2",))


@pytest.mark.parametrize("w", [2, 16, 34, 64, 80, 128, 130, 160, 240])
def test_mapped_a_and_m(ctx, cases, w):
    for name in MATRICES:
        m, x, p, _ = cases[name]
        xw = np.ascontiguousarray(x[:, :w])
        for wreal in _wreals(w):
            for ldy, gaps in ((w, False), (w + 3, False), (2 * w, False), (w + 3, True), (2 * w, True)):
                omap = _omap(w, ldy, gaps)
                _, _, out = run(ctx, "mapped", m, xw, vals9=m.vals, mscal=m.mass, ldy=ldy, wreal=wreal, omap=omap[:wreal].copy())
                _check_mapped("mapped A and M", out, p, w, wreal, omap, ldy, (name, w, wreal, ldy, gaps))


# ---- the residual epilogue --------------------------------------------------------------------------------------------------------
def _theta(w):
    return 10.0 ** np.random.default_rng(80 + w).uniform(0, 2, w)  # distinct per column, one entry per column of the pitch


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("w", [2, 16, 34, 80, 128])
def test_residual_epilogue(ctx, cases, w, weighted):
    theta = _theta(w)
    assert len(set(theta.tolist())) == w
    for name in MATRICES:
        m, x, p, _ = cases[name]
        xw = np.ascontiguousarray(x[:, :w])
        dinv = 10.0 ** np.random.default_rng(90).uniform(-3, 0, 3 * m.n) if weighted else None
        for wreal in (w - 1, w):  # odd and even
            for ldy, gaps in ((w, False), (w + 3, True)):
                omap = _omap(w, ldy, gaps)
                tag = (name, w, wreal, ldy, weighted)
                _, _, out = run(ctx, "mapped_res", m, xw, vals9=m.vals, mscal=m.mass, ldy=ldy, wreal=wreal, omap=omap[:wreal].copy(), theta=theta, dinv=dinv)
                _check_mapped("residual epilogue: y, y2", out, p, w, wreal, omap, ldy, tag)
                r, part = out["r_out"], out["partial"].reshape(m.n, 2, w)
                assert not lab.spmm_untouched(r).any() and not lab.spmm_untouched(part).any(), tag  # the pad column and the columns up to w too
                # stored columns: against the launch's own y, y2 (the same registers)
                cols = omap[:wreal].astype(np.int64)
                y, y2 = out["y"][:, cols], out["y2"][:, cols]
                judge("residual epilogue: r", r[:, :wreal], ref.residual_exact(y, y2, theta[:wreal]), ref.residual_bound(y, y2, theta[:wreal]), tag + ("r",))
                want = ref.partial_exact(r, dinv)  # every column, the unstored ones included: r itself is stored
                judge("residual epilogue: partials", part[:, 0, :], want, ref.partial_bound(want), tag + ("sum r^2",))
                want = ref.partial_exact(y2, dinv)
                judge("residual epilogue: partials", part[:, 1, :wreal], want, ref.partial_bound(want), tag + ("sum (M x)^2",))
                if wreal < w:  # the columns whose y, y2 are not stored: against the reference product, its bounds carried through
                    rr, br, pm, bpm = ref.unstored_residual(p, theta, w, dinv)
                    judge("residual epilogue: unstored columns", r[:, wreal:], rr[:, wreal:], br[:, wreal:], tag + ("r, unstored",))
                    judge("residual epilogue: unstored columns", part[:, 1, wreal:], pm[:, wreal:], bpm[:, wreal:], tag + ("sum (M x)^2, unstored",))


@pytest.mark.parametrize("form,w", [("mapped", 33), ("mapped_res", 33), ("mapped_res", 130), ("mapped_res", 160)])
def test_mapped_forms_refuse_on_the_host(ctx, cases, form, w):
    """An odd pitch, and a residual epilogue on more than 128 columns: MH_EINVAL before any launch, nothing written."""
    m, x, _, _ = cases["crafted"]
    kw = dict(theta=_theta(w)) if form == "mapped_res" else {}
    _, _, out = run(ctx, form, m, np.ascontiguousarray(x[:, :w]), expect_rc=MH_EINVAL, vals9=m.vals, mscal=m.mass, ldy=w + 3, wreal=w - 1,
                    omap=_omap(w, w + 3, True)[: w - 1].copy(), **kw)
    assert all_untouched(out)


# ---- the fused Chebyshev step -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [4, 20, 32, 76, 80, 84, 128, 256])
def test_fused_chebyshev_step(ctx, cheb_cases, w):
    for name in MATRICES:
        m, d, r, xs, dinv, c1, c2, ((rn, br), (dn, bd), (xn, bx)) = cheb_cases[name]
        dw, rw, xw = (np.ascontiguousarray(a[:, :w]) for a in (d, r, xs))
        _, taken, out = run(ctx, "f32_cheb", m, dw, vals9=m.vals32, dinv=dinv, c1=float(c1), c2=float(c2), r=rw, xs=xw)
        assert taken, (name, w)
        assert np.array_equal(_bits(out["d_in"]), _bits(dw)), (name, w, "d_in changed")
        judge("Chebyshev step: r", out["r"], rn[:, :w], br[:, :w], (name, w, "r"))
        judge("Chebyshev step: d", out["d_out"], dn[:, :w], bd[:, :w], (name, w, "d_out"))
        judge("Chebyshev step: x", out["x"], xn[:, :w], bx[:, :w], (name, w, "x"))


@pytest.mark.parametrize("w", [2, 6, 30, 258, 260])
def test_fused_chebyshev_step_declines_and_touches_nothing(ctx, cheb_cases, w):
    m, _, _, _, dinv, c1, c2, _ = cheb_cases["crafted"]
    dw, rw, xw = (ref.panel(3 * m.n, w, 100 + j).astype(np.float32) for j in range(3))
    _, taken, out = run(ctx, "f32_cheb", m, dw, vals9=m.vals32, dinv=dinv, c1=float(c1), c2=float(c2), r=rw, xs=xw)
    assert not taken
    assert lab.spmm_untouched(out["d_out"]).all()
    for k, a in (("d_in", dw), ("r", rw), ("x", xw)):
        assert np.array_equal(_bits(out[k]), _bits(a)), (w, k)
