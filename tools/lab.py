"""ctypes binding of libmodalhip_lab.so (mesheditor_amd/csrc/lab): measurement and experiment entry points that are NOT part of
the path's ABI -- timing loops around the product's kernels, the tridiagonalisation variants called directly, the matrix-free
element-by-element operator.  Used by tests, tools/ and bench.py's secondary figures; the product never loads it."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO_PATH = os.path.join(ROOT, "mesheditor_amd", "libmodalhip_lab.so")
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        from mesheditor_amd import _lib as core
        core.lib()  # the product library first (the lab bench links it)
        if not os.path.exists(SO_PATH):
            raise RuntimeError(f"{SO_PATH} is missing: run __graft_entry__.build()")
        L = C.CDLL(SO_PATH)
        vp, u32, i32, f64p = C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_double)
        L.mhl_system_bench_spmm.restype, L.mhl_system_bench_spmm.argtypes = i32, [vp, u32, u32, f64p, f64p]
        L.mhl_system_bench_elementwise.restype, L.mhl_system_bench_elementwise.argtypes = i32, [vp, u32, u32, f64p]
        L.mhl_system_elementwise_matvec.restype, L.mhl_system_elementwise_matvec.argtypes = i32, [vp, vp, vp, u32]
        L.mhl_context_bench_dense.restype, L.mhl_context_bench_dense.argtypes = i32, [vp, i32, C.c_uint64, u32, u32, u32, f64p]
        L.mhl_context_tridiagonalize.restype, L.mhl_context_tridiagonalize.argtypes = i32, [vp, i32, u32, vp, vp, vp, u32, f64p]
        L.mhl_context_bench_stream.restype, L.mhl_context_bench_stream.argtypes = i32, [vp, C.c_uint64, u32, f64p, f64p]
        L.mhl_context_gram.restype, L.mhl_context_gram.argtypes = i32, [vp, C.c_uint64, vp, u32, vp, u32, vp]
        L.mhl_context_pool_stats.restype, L.mhl_context_pool_stats.argtypes = i32, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.mhl_context_potrf_inverse.restype, L.mhl_context_potrf_inverse.argtypes = i32, [vp, u32, vp, vp, vp, vp, vp]
        L.mhl_context_spd_inverse.restype, L.mhl_context_spd_inverse.argtypes = i32, [vp, u32, vp, vp, u32, f64p]
        L.mhl_context_small_gemm.restype, L.mhl_context_small_gemm.argtypes = i32, [vp, i32, i32, u32, u32, u32, C.c_double, vp, u32, vp, u32, C.c_double, vp, u32, u32, f64p]
        L.mhl_context_tridiagonalize_full.restype, L.mhl_context_tridiagonalize_full.argtypes = i32, [vp, i32, u32, vp, vp, vp, vp, vp, u32, f64p]
        L.mhl_graph_aggregates.restype, L.mhl_graph_aggregates.argtypes = u32, [vp, vp, u32, u32, u32, vp]
        L.mhl_context_tridiag_lowest.restype, L.mhl_context_tridiag_lowest.argtypes = i32, [vp, u32, u32, vp, vp, vp, vp, f64p, C.POINTER(i32)]
        L.mhl_context_rr_solve.restype, L.mhl_context_rr_solve.argtypes = i32, [vp, u32, vp, vp, u32, i32, vp, vp, C.POINTER(u32), vp, vp]
        L.mhl_system_precondition.restype, L.mhl_system_precondition.argtypes = i32, [vp, C.c_double, i32, vp, vp, u32]
        L.mhl_system_hierarchy_sizes.restype, L.mhl_system_hierarchy_sizes.argtypes = i32, [vp, C.c_double, i32, vp]
        L.mhl_system_hierarchy_export.restype, L.mhl_system_hierarchy_export.argtypes = i32, [vp, u32, vp, vp, vp, vp, vp, vp, vp]
        L.mhl_system_patch_export.restype, L.mhl_system_patch_export.argtypes = i32, [vp, i32, vp, vp, vp, vp, vp, vp]
        L.mhl_context_spmm_form.restype, L.mhl_context_spmm_form.argtypes = i32, [vp, C.POINTER(SpmmRequest)]
        L.mhl_context_dense_form.restype, L.mhl_context_dense_form.argtypes = i32, [vp, C.POINTER(DenseRequest)]
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def bench_spmm(system, width, reps=20):
    """(average ms, algorithmic bytes) of one fp64 K x product over an n x width panel."""
    ms, by = C.c_double(0), C.c_double(0)
    system.ctx.check(lib().mhl_system_bench_spmm(system.h, width, reps, C.byref(ms), C.byref(by)))
    return ms.value, by.value


def bench_elementwise(system, width, reps=20):
    ms = C.c_double(0)
    system.ctx.check(lib().mhl_system_bench_elementwise(system.h, width, reps, C.byref(ms)))
    return ms.value


def elementwise_matvec(system, x):
    """(K - sigma M) x at the reference's shift, element by element without the assembled matrix."""
    x = np.asfortranarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    y = np.zeros_like(x, order="F")
    system.ctx.check(lib().mhl_system_elementwise_matvec(system.h, _p(x), _p(y), x.shape[1]))
    return y


def bench_dense(ctx, kind, n, wa, wb, reps=10):
    ms = C.c_double(0)
    ctx.check(lib().mhl_context_bench_dense(ctx.h, kind, n, wa, wb, reps, C.byref(ms)))
    return ms.value


def tridiagonalize(ctx, a, variant=0, reps=1):
    """(d, e, average ms) of the Householder tridiagonalisation of a symmetric matrix (order <= 256)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    m = a.shape[0]
    d, e, ms = np.zeros(m), np.zeros(m - 1), C.c_double(0)
    ctx.check(lib().mhl_context_tridiagonalize(ctx.h, variant, m, _p(a), _p(d), _p(e), reps, C.byref(ms)))
    return d, e, ms.value


def tridiagonalize_full(ctx, a, variant=2, reps=1):
    """(d, e, reflectors [column-major m x m, LAPACK's lower storage], tau, average ms); variant 2 = the wide kernel (order <= 768)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    m = a.shape[0]
    d, e, refl, tau, ms = np.zeros(m), np.zeros(m - 1), np.zeros((m, m)), np.zeros(m), C.c_double(0)
    ctx.check(lib().mhl_context_tridiagonalize_full(ctx.h, variant, m, _p(a), _p(d), _p(e), _p(refl), _p(tau), reps, C.byref(ms)))
    return d, e, refl.T.copy(), tau, ms.value  # (the device's column-major image read as rows: transposed back)


def tridiag_lowest(ctx, d, e, k):
    """(w [k], z [m x k], quality, taken) of the k lowest eigenpairs of the symmetric tridiagonal (d, e) by the Rayleigh-Ritz step's
    partial-spectrum kernels (orders <= 256: one workgroup; 257 .. 768: the wide form).  quality is the kernels' own residual measure
    (NaN when a factorisation failed); taken is False when the call declined the problem (w, z zero, quality NaN)."""
    d = np.ascontiguousarray(d, dtype=np.float64)
    e = np.ascontiguousarray(e, dtype=np.float64)
    m = len(d)
    assert len(e) == m - 1
    w, z, q, taken = np.zeros(k), np.zeros((m, k), order="F"), C.c_double(np.nan), C.c_int(0)
    ctx.check(lib().mhl_context_tridiag_lowest(ctx.h, m, k, _p(d), _p(e), _p(w), _p(z), C.byref(q), C.byref(taken)))
    return w, z, q.value, bool(taken.value)


RR_REDUCTIONS = ("given identity", "measured identity", "series", "cholesky")
RR_SOLVERS = ("syevd", "small partial", "small stedc", "wide partial", "wide stedc+ormtr")


def rr_solve(ctx, a, mmat=None, nwant=0, gm_is_identity=False):
    """One Rayleigh-Ritz step (the solver's rr_solve) on the pencil (a, mmat), lower triangles used.  Returns (theta, C, host_evals,
    trace): the ncols eigenvalues and gM-orthonormal vectors (m x ncols; ncols = nwant on a partial path, else m), the eigenvalues the
    partial path read back on the host (None when it did not), and a dict of what ran: reduction, defect (None when not measured),
    solver, quality (NaN when no partial spectrum ran) and selfcheck (the sampled self-check word; 0 when none ran)."""
    af = np.asfortranarray(a, dtype=np.float64)
    m = af.shape[0]
    mf = None if mmat is None else np.asfortranarray(mmat, dtype=np.float64)
    ev, vec, hv, tr, ncols = np.zeros(m), np.zeros((m, m), order="F"), np.zeros(max(nwant, 1)), np.zeros(6), C.c_uint32(0)
    ctx.check(lib().mhl_context_rr_solve(ctx.h, m, _p(af), None if mf is None else _p(mf), nwant, int(gm_is_identity), _p(ev), _p(vec), C.byref(ncols), _p(hv), _p(tr)))
    n = ncols.value
    trace = {"reduction": RR_REDUCTIONS[int(tr[0])], "defect": None if tr[1] < 0 else float(tr[1]), "solver": RR_SOLVERS[int(tr[2])], "quality": float(tr[3]),
             "selfcheck": float(tr[4])}
    vectors = vec.reshape(-1, order="F")[: m * n].reshape((m, n), order="F").copy()
    return ev[:n].copy(), vectors, (hv[: int(tr[5])].copy() if tr[5] > 0 else None), trace


def gram(ctx, x, y):
    """X^T Y through the solver's Gram kernel (x: n x wa, y: n x wb)."""
    xc, yc = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    n, wa = xc.shape
    wb = yc.shape[1]
    g = np.zeros((wb, wa))  # column-major wa x wb
    ctx.check(lib().mhl_context_gram(ctx.h, n, _p(xc), wa, _p(yc), wb, _p(g)))
    return g.T.copy()


# The guard and sentinel conventions of the "form" entries (modalhip_lab.h: MHL_GUARD, MHL_SENTINEL*): every output is a host array of
# GUARD + entries + GUARD values that comes back whole from a device buffer pre-filled with the sentinel.
GUARD = 64
SENTINEL = {np.dtype(np.float64): np.uint64(0x7FF8A5A5A5A5A5A5), np.dtype(np.float32): np.uint32(0x7FD5A5A5)}


def untouched(a):
    """Boolean array: which entries of an output of a form entry still hold the sentinel, bit for bit."""
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32) == SENTINEL[a.dtype]


def _guarded(entries, dtype=np.float64, body=None):
    """A host output buffer: sentinels, the body `body` when given."""
    buf = np.empty(entries + 2 * GUARD, dtype)
    buf.view(np.uint64 if dtype == np.float64 else np.uint32)[:] = SENTINEL[np.dtype(dtype)]
    if body is not None:
        buf[GUARD:GUARD + entries] = np.asarray(body, dtype=dtype).reshape(-1)
    return buf


def _body_and_guards(buf, shape):
    return buf[GUARD:len(buf) - GUARD].reshape(shape), np.concatenate([buf[:GUARD], buf[len(buf) - GUARD:]])


SPMM_FORMS = ("f64_a", "f64_m", "f64_am", "f32_a", "mixed", "mapped", "mapped_res", "f32_cheb")  # modalhip_lab.h: MHL_SPMM_*
SPMM_GUARD, SPMM_SENTINEL, spmm_untouched = GUARD, SENTINEL, untouched


class SpmmRequest(C.Structure):
    _fields_ = [("form", C.c_int32), ("misalign", C.c_uint32), ("n_nodes", C.c_uint32), ("w", C.c_uint32), ("ldy", C.c_uint32), ("wreal", C.c_uint32),
                ("c1", C.c_float), ("c2", C.c_float), ("row_ptr", C.c_void_p), ("col", C.c_void_p), ("omap", C.c_void_p), ("vals9", C.c_void_p),
                ("mscal", C.c_void_p), ("x", C.c_void_p), ("theta", C.c_void_p), ("dinv", C.c_void_p), ("dinv32", C.c_void_p), ("r", C.c_void_p),
                ("xs", C.c_void_p), ("y", C.c_void_p), ("y2", C.c_void_p), ("r_out", C.c_void_p), ("partial", C.c_void_p), ("cheb_r", C.c_void_p),
                ("cheb_d_out", C.c_void_p), ("cheb_x", C.c_void_p), ("cheb_d_in", C.c_void_p), ("taken", C.c_int32)]


def spmm_form(ctx, form, row_ptr, col, x, vals9=None, mscal=None, misalign=False, ldy=0, wreal=0, omap=None, theta=None, dinv=None, c1=0.0, c2=0.0,
              r=None, xs=None):
    """One form (SPMM_FORMS) of the BSR 3x3 product on the caller's matrix through the product's own dispatchers.  x: the row-major panel
    (3 n_nodes x w; float32 for f32_a, mixed and f32_cheb, where it is d); vals9 (n_blocks x 9) is handed over as float32 for f32_a and
    f32_cheb and as float64 otherwise, WITHOUT conversion (a wrong dtype is an error).  Returns (rc, taken, out): the entry's status,
    whether the Chebyshev step took the panel, and per output its (body, guards): the body in its panel shape and the two guard regions
    joined.  Entries nobody wrote hold the sentinel (spmm_untouched); when the dispatcher refused on the host every entry does."""
    f = SPMM_FORMS.index(form)
    f32_vals, f32_x = form in ("f32_a", "f32_cheb"), form in ("f32_a", "mixed", "f32_cheb")
    keep = []

    def arr(a, dtype):
        if a is None:
            return None
        a = np.asarray(a)
        assert a.dtype == dtype and a.flags.c_contiguous, (a.dtype, dtype)
        keep.append(a)
        return _p(a)

    x = np.asarray(x)
    n3, w = x.shape
    nn = len(row_ptr) - 1
    assert n3 == 3 * nn
    outs = {}

    def out(name, rows, pitch, dtype):
        buf = _guarded(rows * pitch, dtype)
        outs[name] = (buf, rows, pitch)
        return _p(buf)

    q = SpmmRequest(form=f, misalign=int(misalign), n_nodes=nn, w=w, ldy=ldy, wreal=wreal, c1=c1, c2=c2)
    q.row_ptr, q.col, q.omap = arr(row_ptr, np.uint32), arr(col, np.uint32), arr(omap, np.uint32)
    q.vals9, q.mscal = arr(vals9, np.float32 if f32_vals else np.float64), arr(mscal, np.float64)
    q.x = arr(x, np.float32 if f32_x else np.float64)
    q.theta, q.dinv = arr(theta, np.float64), arr(dinv, np.float64) if form != "f32_cheb" else None
    if form == "f32_cheb":
        q.dinv32, q.r, q.xs = arr(dinv, np.float32), arr(r, np.float32), arr(xs, np.float32)
        q.cheb_r, q.cheb_d_out, q.cheb_x, q.cheb_d_in = (out(k, n3, w, np.float32) for k in ("r", "d_out", "x", "d_in"))
    else:
        pitch = ldy if form.startswith("mapped") else w
        if form != "f64_m":
            q.y = out("y", n3, pitch, np.float32 if form == "f32_a" else np.float64)
        if form in ("f64_m", "f64_am", "mapped", "mapped_res"):
            q.y2 = out("y2", n3, pitch, np.float64)
        if form == "mapped_res":
            q.r_out, q.partial = out("r_out", n3, w, np.float64), out("partial", 2 * nn, w, np.float64)
    rc = lib().mhl_context_spmm_form(ctx.h, C.byref(q))
    return rc, bool(q.taken), {k: _body_and_guards(b, (rows, pitch)) for k, (b, rows, pitch) in outs.items()}


DENSE_FORMS = ("combine", "short_product", "gram", "pack")  # modalhip_lab.h: MHL_DENSE_*


class DenseRequest(C.Structure):
    _fields_ = [("form", C.c_int32), ("in_place", C.c_int32), ("accumulate", C.c_int32), ("coeff_layout", C.c_int32), ("n", C.c_uint64),
                ("wx", C.c_uint32), ("ldx", C.c_uint32), ("ww", C.c_uint32), ("wp", C.c_uint32), ("nc", C.c_uint32), ("n1", C.c_uint32), ("ld1", C.c_uint32),
                ("ld1_also", C.c_uint32), ("col_begin", C.c_uint32), ("col_count", C.c_uint32), ("slices", C.c_uint32), ("pack_a", C.c_uint32),
                ("pack_b", C.c_uint32), ("pack_ld", C.c_uint32), ("ldy", C.c_uint32), ("ld", C.c_uint32), ("g_cols", C.c_uint32), ("g_row0", C.c_uint32),
                ("g_col0", C.c_uint32), ("pad_", C.c_uint32), ("pack_scale", C.c_double), ("xmap", C.c_void_p), ("omap", C.c_void_p), ("omap_also", C.c_void_p),
                ("ymap", C.c_void_p), ("x", C.c_void_p), ("w", C.c_void_p), ("p", C.c_void_p), ("ct", C.c_void_p), ("c1", C.c_void_p), ("c2", C.c_void_p),
                ("x_out", C.c_void_p), ("out1", C.c_void_p), ("out2", C.c_void_p), ("out1_also", C.c_void_p), ("partial", C.c_void_p), ("ct_out", C.c_void_p),
                ("g", C.c_void_p), ("cu_count", C.c_int32), ("dispatched", C.c_int32)]


class DenseResult:
    """rc, dispatched (False: the lab entry itself rejected the request, the dispatcher never saw it), cu_count, and per output its
    (body, guards) in `out`: x (n x pitch), out1, out2, out1_also, partial (slices x n x nc), ct (m x nc), g (ld x g_cols, as a matrix)."""

    def __init__(self, rc, q, out):
        self.rc, self.dispatched, self.cu_count, self.out = rc, bool(q.dispatched), int(q.cu_count), out

    def body(self, k):
        return self.out[k][0]


def dense_form(ctx, form, n=0, x=None, wx=None, ldx=0, w=None, p=None, nc=0, n1=0, ld1=0, col_begin=0, col_count=0, accumulate=False, slices=1, xmap=None,
               omap=None, omap_also=None, ld1_also=0, also=False, ct=None, blocks=None, stacked=None, in_place=0, old1=None, old2=None, ymap=None, ww=None,
               ldy=0, ld=0, g_cols=0, g_row0=0, g_col0=0, m=None):
    """One form (DENSE_FORMS) of the dense tall products through the solver's own dispatchers (modalhip_lab.h: mhl_dense_request).
    x, w, p: row-major float64 panels of n rows, or None (an absent part: null pointer, width 0); x has ldx columns when ldx is given, of
    which wx (default: all, or len(xmap)) are read.  Coefficients: ct (m x nc, k-major), or blocks = (c1, c2) -- matrices of pack_ld rows whose
    first m rows mh_pack_coefficients sets side by side -- or stacked = (c1, c2, scale) for mh_pack_stacked; None for an absent block.
    in_place: 1 = out1 is X, 2 = out1_also is X; also = True: a separate second destination of pitch ld1_also.  old1, old2: the start
    values of out1 (n x pitch), out2 under accumulate.  Gram: y = w with ww logical columns (through ymap) at pitch ldy, g (ld x g_cols)
    written at (g_row0, g_col0).  `m` is needed by the pack form alone.  Returns a DenseResult."""
    f = DENSE_FORMS.index(form)
    keep = []

    def arr(a, dtype=np.float64, order="C"):
        if a is None:
            return None
        a = np.asarray(a)
        assert a.dtype == dtype and (a.flags.c_contiguous if order == "C" else a.flags.f_contiguous), (a.dtype, dtype, order)
        keep.append(a)
        return _p(a)

    if wx is None:
        wx = 0 if x is None else len(xmap) if xmap is not None else x.shape[1]
    if ww is None:
        ww = 0 if w is None else len(ymap) if ymap is not None else w.shape[1]
    wp = 0 if p is None else p.shape[1]
    if m is None:
        m = wx + ww + wp
    else:
        wx = m  # (the pack form: no panels)
    for a, width in ((x, ldx or wx), (w, (ldy or ww) if form == "gram" else ww)):
        assert a is None or a.shape == (n, width), (a.shape, n, width)
    q = DenseRequest(form=f, in_place=in_place, accumulate=int(accumulate), n=n, wx=wx, ldx=ldx, ww=ww, wp=wp, nc=nc, n1=n1, ld1=ld1, ld1_also=ld1_also,
                     col_begin=col_begin, col_count=col_count, slices=slices, ldy=ldy, ld=ld, g_cols=g_cols, g_row0=g_row0, g_col0=g_col0)
    q.x, q.w, q.p = arr(x), arr(w), arr(p)
    q.xmap, q.omap, q.omap_also, q.ymap = (arr(a, np.uint32) for a in (xmap, omap, omap_also, ymap))
    bufs = {}

    def out(name, shape, body=None):
        bufs[name] = (_guarded(int(np.prod(shape)), body=body), shape)
        return _p(bufs[name][0])

    if blocks is not None:
        c1, c2 = blocks
        q.coeff_layout, q.pack_a, q.pack_b = 1, 0 if c1 is None else c1.shape[1], 0 if c2 is None else c2.shape[1]
        q.pack_ld = (c1 if c1 is not None else c2).shape[0]
        q.c1, q.c2 = arr(c1, order="F"), arr(c2, order="F")
    elif stacked is not None:
        c1, c2, scale = stacked
        q.coeff_layout, q.pack_a, q.pack_b, q.pack_scale = 2, 0 if c1 is None else c1.shape[0], 0 if c2 is None else c2.shape[0], scale
        q.c1, q.c2 = arr(c1, order="F"), arr(c2, order="F")
    elif form != "gram":
        assert ct.shape == (m, nc)
        q.ct = arr(ct)
    if q.coeff_layout:
        q.ct_out = out("ct", (m, nc))
    if form != "pack" and x is not None:
        q.x_out = out("x", x.shape)
    if form == "combine":
        pitch1 = ld1 or n1
        if in_place != 1:
            q.out1 = out("out1", (n, pitch1), old1)
        if nc > n1:
            q.out2 = out("out2", (n, nc - n1), old2)
        if also:
            q.out1_also = out("out1_also", (n, ld1_also))
    elif form == "short_product":
        q.out1 = out("out1", (n, nc))
        if slices > 1:
            q.partial = out("partial", (slices, n, nc))
    elif form == "gram":
        q.g = out("g", (g_cols, ld))
    rc = lib().mhl_context_dense_form(ctx.h, C.byref(q))
    res = {k: _body_and_guards(b, shape) for k, (b, shape) in bufs.items()}
    if "g" in res:
        res["g"] = (res["g"][0].T, res["g"][1])  # column-major ld x g_cols
    return DenseResult(rc, q, res)


def mapped_update_mismatches(ctx, n, wa, wb, gaps):
    """The eigensolver's column-mapped basis update in its two forms (compact panel; compact panel and the mapped columns of X) on the same
    inputs: the number of entries in which the second differs from the first one's result scattered on the host (0 = equal)."""
    bad = C.c_double(-1)
    ctx.check(lib().mhl_context_bench_dense(ctx.h, 3 if gaps else 2, n, wa, wb, 1, C.byref(bad)))
    return int(bad.value)


def bench_stream(ctx, nbytes=4 << 30, reps=10):
    """(copy GB/s counting read + written bytes, read GB/s) of streaming kernels over `nbytes`: the device's measured HBM ceilings."""
    c, r = C.c_double(0), C.c_double(0)
    ctx.check(lib().mhl_context_bench_stream(ctx.h, nbytes, reps, C.byref(c), C.byref(r)))
    return c.value, r.value


def pool_stats(ctx):
    """(bytes held from the device, bytes idle in the cache, cap on the idle bytes) of the context's device pool."""
    r, i, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    ctx.check(lib().mhl_context_pool_stats(ctx.h, C.byref(r), C.byref(i), C.byref(c)))
    return r.value, i.value, c.value


def potrf_inverse(ctx, a, dscale):
    """(L, L^-1, info[2]) of the Cholesky-QR step's one-launch kernel: L = diag(1 / dscale) chol(a) (rows with dscale <= 0: identity rows)."""
    af = np.asfortranarray(a, dtype=np.float64)
    d = np.ascontiguousarray(dscale, dtype=np.float64)
    l, linv, info = np.zeros_like(af, order="F"), np.zeros_like(af, order="F"), np.zeros(2, np.int32)
    ctx.check(lib().mhl_context_potrf_inverse(ctx.h, af.shape[0], _p(af), _p(d), _p(l), _p(linv), _p(info)))
    return l, linv, info


def spd_inverse(ctx, a, reps=1):
    """(a^-1, average ms) through the coarse set-up's one-workgroup Gauss-Jordan kernel (order <= 128)."""
    af = np.asfortranarray(a, dtype=np.float64)
    out, ms = np.zeros_like(af, order="F"), C.c_double(0)
    ctx.check(lib().mhl_context_spd_inverse(ctx.h, af.shape[0], _p(af), _p(out), reps, C.byref(ms)))
    return out, ms.value


def small_gemm(ctx, a, b, c=None, ta=False, tb=False, alpha=1.0, beta=0.0, reps=1):
    """(alpha op(a) op(b) + beta c, average ms) through the Rayleigh-Ritz step's small-product kernel; a, b, c are numpy matrices
    (handed over column-major)."""
    af, bf = np.asfortranarray(a, dtype=np.float64), np.asfortranarray(b, dtype=np.float64)
    M, K = (af.shape[1], af.shape[0]) if ta else af.shape
    N = bf.shape[0] if tb else bf.shape[1]
    cf = np.asfortranarray(np.zeros((M, N)) if c is None else c, dtype=np.float64).copy(order="F")
    ms = C.c_double(0)
    ctx.check(lib().mhl_context_small_gemm(ctx.h, int(ta), int(tb), M, N, K, alpha, _p(af), af.shape[0], _p(bf), bf.shape[0], beta, _p(cf), M, reps, C.byref(ms)))
    return cf, ms.value


def graph_aggregates(row_ptr, col, target=16, max_order=6144):
    """(aggregate of every node, aggregate count) for a CSR node graph with its diagonal entries (host code, no device)."""
    rp = np.ascontiguousarray(row_ptr, np.uint32)
    cl = np.ascontiguousarray(col, np.uint32)
    n = len(rp) - 1
    out = np.zeros(n, np.uint32)
    na = lib().mhl_graph_aggregates(_p(rp), _p(cl), n, target, max_order, _p(out))
    return out, int(na)


SIGMA = -(2 * np.pi * 20.0) ** 2  # the reference's shift (mesh2modes.cpp:460)


def precondition(system, x, precision=1, sigma=SIGMA):
    """B x: the eigensolver's preconditioner cycle at `sigma` with single- (precision 0) or double-precision (1) smoothers, columns in the
    reference's DOF order (at most 1 024; above 256 the eigensolver's column slabs)."""
    x = np.asfortranarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    y = np.zeros_like(x, order="F")
    system.ctx.check(lib().mhl_system_precondition(system.h, sigma, precision, _p(x), _p(y), x.shape[1]))
    return y


def _level_patches(system, level, o):
    """The sliver patches and clusters of level 2 (P2) or 1 (P1), node ids and DOF rows in the reference numbering of that level."""
    npatch, npe, ncl, crows, cvals = (int(v) for v in o[:5])
    nodes, weight, inv = np.zeros((npatch, npe), np.uint32), np.zeros(npatch), np.zeros((npatch, 3 * npe, 3 * npe))
    crow, cptr, cinv = np.zeros(crows, np.uint32), np.zeros(ncl + 1, np.uint32), np.zeros(cvals)
    system.ctx.check(lib().mhl_system_patch_export(system.h, level, _p(nodes), _p(weight), _p(inv), _p(crow), _p(cptr), _p(cinv)))
    clusters, off = [], 0
    for c in range(ncl):
        rows = crow[cptr[c]:cptr[c + 1]].astype(np.int64)
        clusters.append((rows, cinv[off:off + len(rows) ** 2].reshape(len(rows), len(rows))))
        off += len(rows) ** 2
    return {"nodes": nodes.astype(np.int64), "weight": weight, "inv64": inv, "clusters": clusters, "n_bad_elements": int(o[5]), "largest_cluster": int(o[6]),
            "dropped": int(o[7])}


def hierarchy(system, sigma=SIGMA, width=64, rebuild=False):
    """The preconditioner's hierarchy built at `sigma` (anew when `rebuild`), exported in the reference's numbering: sizes, both levels'
    spectral bounds, the coarse lift, the cycle shape for `width` columns, per mesh point its aggregate and 3 x 6 rigid-body block, the P1
    operator's node blocks, the coarse inverse a0, and the sliver patches and clusters of both smoothed levels."""
    sizes = np.zeros(20, np.uint64)
    system.ctx.check(lib().mhl_system_hierarchy_sizes(system.h, sigma, int(rebuild), _p(sizes)))
    npts, nagg, n0, nb1 = (int(v) for v in sizes[:4])
    sc, agg, tm = np.zeros(10), np.zeros(npts, np.uint32), np.zeros((npts, 3, 6))
    r1, c1, v1, a0 = np.zeros(nb1, np.uint32), np.zeros(nb1, np.uint32), np.zeros((nb1, 3, 3)), np.zeros((n0, n0), order="F")
    system.ctx.check(lib().mhl_system_hierarchy_export(system.h, width, _p(sc), _p(agg), _p(tm), _p(r1), _p(c1), _p(v1), _p(a0)))
    return {"n_points": npts, "n_agg": nagg, "n0": n0, "lmax2": sc[0], "lmax1": sc[1], "lift": sc[2],
            "shape": {"deg2": int(sc[3]), "ratio": sc[4], "deg1": int(sc[5]), "gamma": int(sc[6]), "ratio1": sc[7]}, "sigma": sc[8], "worst_quality": sc[9],
            "agg_of": agg.astype(np.int64), "agg_t": tm, "l1_row": r1.astype(np.int64), "l1_col": c1.astype(np.int64), "l1_val": v1, "a0": a0,
            "patches2": _level_patches(system, 2, sizes[4:12]), "patches1": _level_patches(system, 1, sizes[12:20])}
