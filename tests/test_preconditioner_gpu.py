"""The eigensolver's preconditioner B (mh_eigs.hip: Precond) as an operation, against its float64 host restatement
(tests/precond_reference.py).  A wrong B does not change a converged answer -- it only slows the iteration -- so the eigenvalue tests
cannot see it: here the hierarchy's pieces (rigid-body prolongator, P1 operator, coarse inverse, patch and cluster inverses, spectral
bounds) and the whole cycle are compared with the host, and B's own properties (symmetric, positive definite, B A well conditioned,
independent of the panel width) are checked as a dense matrix on small meshes.

Every tolerance below was measured on the MI355X (the value seen is beside each bound)."""
import threading

import numpy as np
import pytest
import scipy.linalg as sla

from mesheditor_amd import meshes
from tests import precond_reference as ref
from tools import lab

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
SIGMA = lab.SIGMA


def _two_bodies():
    p1, t1 = meshes.kuhn_box(3, 3, 3, 0.1, 0.1, 0.1)
    p2, t2 = meshes.kuhn_box(2, 2, 4, 0.05, 0.05, 0.12, origin=(0.3, 0.0, 0.0))
    return np.concatenate([p1, p2]), np.concatenate([t1, t2 + len(p1)]).astype(np.uint32), meshes.MATERIALS["Ceramic"]


def _flat_uv_sphere():
    """A 32 x 16 UV sphere's fill with 60 interior points moved to 1e-6 of a face: flat cells, hence clusters and double-precision smoothers."""
    from mesheditor_amd import tets as fe
    v, f = meshes.uv_sphere_surface(0.15, 32, 16)
    p, t, _ = fe.tetrahedralize(v, f)
    fp, _ = meshes.with_flat_cells(p, t, len(v), count=60, eps=1e-6, seed=32)
    return fp, t, meshes.MATERIALS["Ceramic"]


# name: (mesh, dense checks, smoother precisions the product runs there, widths compared with the host, what the mesh is there for)
CASES = {
    "cube_small": (lambda: meshes.workload("cube_small")[:3], True, (1, 0), (1, 3, 5, 64, 80, 81, 256, 257, 300), "surface, n0 < 128"),
    "cube_s10k": (lambda: meshes.workload("cube_s10k")[:3], False, (1, 0), (3, 257), "bulk, n0 in several ragged 128-column steps"),
    "bar_thin": (lambda: meshes.workload("bar_thin")[:3], True, (1, 0), (1, 3, 5, 64, 80, 81, 256, 257, 300), "surface"),
    "scan_small": (lambda: meshes.skillet_scan_tets(0.05, 0.04) + (meshes.MATERIALS["Iron"],), True, (1, 0), (1, 3, 5, 64, 80, 81, 256, 257, 300), "patches"),
    "scan_s30k": (lambda: meshes.workload("scan_s30k")[:3], False, (1, 0), (1, 5), "patches"),
    "flat_uv32": (_flat_uv_sphere, False, (1,), (1, 3, 257), "clusters"),
    "two_bodies": (_two_bodies, True, (1, 0), (1, 5, 81, 257), "bulk"),
}
DENSE = [k for k, v in CASES.items() if v[1]]


@pytest.fixture(scope="module")
def ctx():
    from mesheditor_amd import api
    c = api.Context(0)
    yield c
    c.close()


_CACHE = {}


def _problem(ctx, name):
    """(device system, exported hierarchy, host restatement pieces) of one case, built once per module."""
    if name in _CACHE:
        return _CACHE[name]
    from mesheditor_amd import api
    p, t, mat = CASES[name][0]()
    mesh = api.Mesh(ctx, p, t)
    s = api.System(ctx, mesh, api.material(*mat))
    h = lab.hierarchy(s, SIGMA, width=64)
    K, M = s.to_scipy()
    A2 = ref.shifted_operator(K, M, SIGMA)
    en = s.element_nodes().astype(np.int64)
    npts = h["n_points"]
    P = ref.prolongation(en, s.node_count, npts)
    A1 = ref.p1_operator(h["l1_row"], h["l1_col"], h["l1_val"], npts)
    tb = ref.rigid_body_blocks(p[:npts], h["agg_of"], h["n_agg"])
    T = ref.rigid_body_t(tb, h["agg_of"], h["n_agg"])
    a0 = ref.coarse_operator(A1, T, h["lift"])
    rows = lambda nodes: ref._node_rows(nodes)  # noqa: E731
    lv = {}
    for level, A in ((2, A2), (1, A1)):
        ps = h["patches%d" % level]
        patches = [(rows(nd), w) for nd, w in zip(ps["nodes"], ps["weight"])]
        clusters = [r for r, _ in ps["clusters"]]
        dev = list(ps["inv64"]) + [c for _, c in ps["clusters"]]
        lv[level] = {"patches": patches, "clusters": clusters, "Minv": ref.smoother_scaling(A, patches, clusters),
                     "Minv_device_inverses": ref.smoother_scaling(A, patches, clusters, dev)}
    a0inv = np.linalg.inv(a0)
    host = {"A2": A2, "A1": A1, "A1_galerkin": (P.T @ A2 @ P).tocsr(), "P": P, "T": T, "t_blocks": tb, "a0": a0, "a0inv": 0.5 * (a0inv + a0inv.T), "levels": lv,
            "points": p, "mesh": mesh}
    _CACHE[name] = (s, h, host)
    return _CACHE[name]


def _host_cycle(s, h, host, width, own_inverses=False):
    """The host cycle for `width` columns, by default with the device's coarse, patch and cluster inverses (each judged on its own:
    test_coarse_level_matches_the_host, test_patch_and_cluster_inverses_match_the_host).  With the host's own inverses the comparison
    measures cond(A0) or cond(A_ee) times the rounding of the device's operators -- 1e-9 .. 2e-6 here -- instead of the cycle."""
    sh = lab.hierarchy(s, SIGMA, width=width)["shape"]
    lv = host["levels"]
    m = "Minv" if own_inverses else "Minv_device_inverses"
    return ref.Cycle(host["A2"], lv[2][m], h["lmax2"], host["P"], host["A1"], lv[1][m], h["lmax1"], host["T"], host["a0inv"] if own_inverses else h["a0"], sh)


def _panel(n, w, seed):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((n, w)))


def _colrel(got, want):
    return (np.linalg.norm(got - want, axis=0) / np.linalg.norm(want, axis=0)).max()


# ---- what each case was chosen for ---------------------------------------------------------------------------------------------
def test_each_mesh_has_the_structure_it_was_chosen_for(ctx):
    """A generator change must not silently remove a test's subject: the cycle shape, the coarse order, patches with overlap weights below
    1, clusters above 128 rows (the blocked inverse), two bodies."""
    seen = {}
    for name in CASES:
        s, h, _ = _problem(ctx, name)
        p2, p1 = h["patches2"], h["patches1"]
        seen[name] = (h["shape"], h["n0"], len(p2["weight"]), float(p2["weight"].min()) if len(p2["weight"]) else None, len(p2["clusters"]),
                      p2["largest_cluster"], h["worst_quality"])
        assert p2["dropped"] == 0 and p1["dropped"] == 0, name
    # (384 tetrahedra on 125 points: fewer than 4.5 per point, so the product gives cube_small the surface-dominated shape; a Kuhn cube is
    # bulk from 10 cells a side on, too large for the dense checks)
    assert seen["cube_small"][0] == {"deg2": 5, "ratio": 60.0, "deg1": 16, "gamma": 1, "ratio1": 250.0} and seen["cube_small"][1] < 128
    assert seen["cube_s10k"][0] == {"deg2": 2, "ratio": 8.0, "deg1": 12, "gamma": 1, "ratio1": 100.0} and seen["cube_s10k"][1] > 3 * 128 and seen["cube_s10k"][1] % 128 != 0  # several steps, the last one ragged
    assert seen["bar_thin"][0] == {"deg2": 5, "ratio": 60.0, "deg1": 16, "gamma": 1, "ratio1": 250.0} and seen["bar_thin"][2] == 0
    for name in ("scan_small", "scan_s30k"):
        assert seen[name][2] > 0 and seen[name][3] < 1.0 and seen[name][4] == 0 and seen[name][6] > 1e-4, (name, seen[name])  # overlapping element patches, fp32 mesh
    assert seen["scan_small"][0]["deg2"] == 5 and seen["scan_small"][0]["ratio"] == 60.0
    assert seen["flat_uv32"][6] < 1e-4 and seen["flat_uv32"][4] > 0 and seen["flat_uv32"][5] > 42, seen["flat_uv32"]  # a cluster of more than 128 rows
    s, h, _ = _problem(ctx, "two_bodies")
    assert h["n_agg"] >= 2


# ---- a. coarse level -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_coarse_level_matches_the_host(ctx, name):
    """T equals its restatement from k_aggregate_t; the device's P1 operator is the Galerkin product P^T A2 P to rounding;
    a0 is exactly symmetric and inverts the host's T^T A1 T (with the lift) to cond(A0) eps."""
    s, h, host = _problem(ctx, name)
    t_err = np.abs(h["agg_t"] - host["t_blocks"]).max() / np.abs(host["t_blocks"]).max()
    A1, Ag = host["A1"], host["A1_galerkin"]
    g_err = abs(A1 - Ag).max() / abs(Ag).max()  # (over both patterns: an entry of either alone counts in full)
    a0 = h["a0"]
    cond = np.linalg.cond(host["a0"])
    res = np.abs(host["a0"] @ a0 - np.eye(h["n0"])).max()
    # the device formed its own T^T A1 T: entries that cancel from |T|^T |A1| |T| down to A0 carry that much more rounding into the inverse
    Tabs = abs(host["T"])
    rho = (Tabs.T @ abs(A1) @ Tabs).max() / np.abs(host["a0"]).max()
    print("COARSE %s t %.3e galerkin %.3e n0 %d cond %.3e rho %.3e res %.3e res/(cond eps rho) %.4f" % (name, t_err, g_err, h["n0"], cond, rho, res, res / (cond * EPS * rho)))
    assert t_err <= 4e-14, t_err  # (6e-16 .. 1.5e-14 measured)
    assert g_err <= 1e-13, g_err  # (3e-16 .. 1.1e-15)
    assert np.array_equal(a0, a0.T)
    assert res <= COARSE_RES.get(name, 1.0) * cond * EPS, (res, cond, res / (cond * EPS))


# ||A0_host a0 - I||_max / (cond(A0) eps): 0.06 .. 0.44 measured; the thin bar's and the flat cells' coarse operators cancel more in the
# device's own Galerkin product (the matrix a0 inverts), 249 and 6 459 measured
COARSE_RES = {"bar_thin": 1000.0, "flat_uv32": 26000.0}


# ---- b. coarse inverse reproducibility -----------------------------------------------------------------------------------------
def test_coarse_inverse_is_bit_identical_across_builds_and_under_load(ctx):
    """The elimination with its pivot inverses one step ahead on a third stream (mh_build_hierarchy) gives the same a0 bit for bit when built
    again, and when built while another context runs a wide solve (a 120-pair block: rocBLAS's LDS-heavy kernels beside it).  Run once."""
    from mesheditor_amd import api
    s, h, _ = _problem(ctx, "cube_s10k")
    first = h["a0"].copy()
    again = lab.hierarchy(s, SIGMA, rebuild=True)["a0"]
    assert np.array_equal(first, again)
    p, t = meshes.jittered_box(12, 1001)
    other = api.Context(0)
    errs, running, done = [], threading.Event(), threading.Event()

    def wide():
        try:
            m = api.Mesh(other, p, t)
            sy = api.System(other, m, api.material(*meshes.MATERIALS["Glass"]))
            running.set()
            sy.eigs(120, SIGMA, 1e-5)
            sy.close()
            m.close()
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e)[:200])
        finally:
            running.set()
            done.set()
    th = threading.Thread(target=wide)
    th.start()
    running.wait()
    loaded, overlapped = [], 0
    while not done.is_set() or not loaded:
        loaded.append(lab.hierarchy(s, SIGMA, rebuild=True)["a0"])
        overlapped += not done.is_set()
        if len(loaded) >= 4:
            break
    th.join()
    other.close()
    assert not errs, errs
    assert overlapped > 0
    assert all(np.array_equal(first, a) for a in loaded)


# ---- c. patches ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["scan_small", "scan_s30k", "flat_uv32"])
def test_patch_and_cluster_inverses_match_the_host(ctx, name):
    """Every weighted element-patch inverse and every cluster inverse equals its host inverse to cond eps; nothing was dropped."""
    s, h, host = _problem(ctx, name)
    worst = 0.0
    for level, A in ((2, host["A2"]), (1, host["A1"])):
        ps = h["patches%d" % level]
        assert ps["dropped"] == 0
        for (rows, w), inv in zip(host["levels"][level]["patches"], ps["inv64"]):
            blk = A[rows][:, rows].toarray()
            want = w * np.linalg.inv(blk)
            worst = max(worst, np.abs(inv - want).max() / np.abs(want).max() / (np.linalg.cond(blk) * EPS))
        for rows, cinv in ps["clusters"]:
            blk = A[rows][:, rows].toarray()
            want = np.linalg.inv(blk)
            worst = max(worst, np.abs(cinv - want).max() / np.abs(want).max() / (np.linalg.cond(blk) * EPS))
    print("PATCH %s worst/(cond eps) %.3e" % (name, worst))
    assert worst <= 4.0, worst  # (0.11 .. 0.76 measured)


# ---- d. spectral bounds --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_spectral_bounds_lie_above_the_spectrum(ctx, name):
    """Each smoothed level's lmax lies in (lambda_max(M^-1 A), 1.1 lambda_max(M^-1 A)] (DESIGN: a margin of 6-9 %)."""
    s, h, host = _problem(ctx, name)
    for level, A, lmax in ((2, host["A2"], h["lmax2"]), (1, host["A1"], h["lmax1"])):
        lam = ref.spectral_radius(A, host["levels"][level]["Minv"])
        print("LMAX %s level %d lmax/lambda %.4f" % (name, level, lmax / lam))
        assert lam < lmax <= 1.1 * lam * (1 + 1e-9), (level, lmax / lam)  # (1.050 .. 1.099 measured)


# ---- e, f. the whole cycle -----------------------------------------------------------------------------------------------------
FP32_BOUND = 3e-5  # (1.1e-6 .. 7.7e-6 measured)


@pytest.mark.parametrize("name", list(CASES))
def test_cycle_matches_the_host_restatement(ctx, name):
    """B X from the device against the host's float64 cycle, at every width of the case (above 256: the eigensolver's column slabs), with
    double- and (where the product runs them) single-precision smoothers; and the two precisions against each other."""
    s, h, host = _problem(ctx, name)
    n = s.n
    precisions, widths = CASES[name][2], CASES[name][3]
    for w in widths:
        cyc = _host_cycle(s, h, host, w)
        # one P1 cycle: rounding only (1e-15 .. 1e-14 measured).  Three (the patch meshes' shape up to 128 columns) form r1 - A1 x1 three times
        # and carry cond(A1) eps of it into B -- as in the host's own restatement (tests/test_precond_reference_cpu.py): 5e-10 .. 1.5e-8 measured;
        # flat cells do the same through their clusters' blocks (condition ~ 1 / shape): 2.1e-10 at 257 columns, one P1 cycle
        bound64 = 1e-13 if cyc.gamma == 1 and h["worst_quality"] >= 1e-4 else 2e-7
        X = _panel(n, w, w)
        want = cyc.apply(X)
        got64 = lab.precondition(s, X, 1)
        e64 = _colrel(got64, want)
        print("CYCLE %s w %d gamma %d fp64 %.3e own-inverses %.3e" % (name, w, cyc.gamma, e64, _colrel(got64, _host_cycle(s, h, host, w, True).apply(X)) if w == widths[0] else -1))
        e32 = 0.0
        if 0 in precisions:
            got32 = lab.precondition(s, X, 0)
            e32 = _colrel(got32, want)
            print("CYCLE %s w %d fp32 %.3e fp32-fp64 %.3e" % (name, w, e32, _colrel(got32, got64)))
        assert e64 <= bound64, (w, e64)
        assert e32 <= FP32_BOUND, (w, e32)


@pytest.mark.parametrize("name", DENSE)
def test_dense_cycle_is_symmetric_positive_definite_and_well_conditioning(ctx, name):
    """B formed densely from identity panels: symmetric to rounding, positive definite, and cond(B A) below the measured value x 1.25."""
    s, h, host = _problem(ctx, name)
    n = s.n
    A = host["A2"].toarray()
    dense = {}
    for prec in sorted(CASES[name][2], reverse=True):
        B = np.zeros((n, n))
        for c0 in range(0, n, 1024):
            c1 = min(n, c0 + 1024)
            E = np.zeros((n, c1 - c0), order="F")
            E[np.arange(c0, c1), np.arange(c1 - c0)] = 1.0
            B[:, c0:c1] = lab.precondition(s, E, prec)
        dense[prec] = B
        asym = np.abs(B - B.T).max() / np.abs(B).max()
        if prec == 0:
            # single-precision smoothers: symmetric and equal to the double-precision B at their own rounding level.  (Definiteness is not
            # theirs to keep: B's smallest eigenvalues lie 1e-6 ... 1e-8 below its largest, the size of that rounding -- measured on scan_small,
            # whose fp32 B has a slightly negative one.)
            agree = np.abs(B - dense[1]).max() / np.abs(dense[1]).max()
            print("DENSE %s prec 0 asym %.3e fp32-fp64 %.3e" % (name, asym, agree))
            assert asym <= 1e-4, asym  # (2e-6 .. 2.7e-5 measured)
            assert agree <= 1e-4, agree  # (2.7e-6 .. 2.5e-5)
            continue
        Bs = 0.5 * (B + B.T)
        w = np.linalg.eigvalsh(Bs)
        mu = sla.eigh(A, np.linalg.inv(Bs), eigvals_only=True)
        cond = mu[-1] / mu[0]
        print("DENSE %s prec %d asym %.3e lmin %.3e cond(BA) %.4f" % (name, prec, asym, w[0], cond))
        assert asym <= 1e-12, asym
        assert w[0] > 0
        assert cond <= COND_BA[name] * 1.25, cond


COND_BA = {"cube_small": 1.5804, "bar_thin": 16.9511, "scan_small": 19.9186, "two_bodies": 2.3633}  # measured, double-precision smoothers


# ---- g. width independence -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube_small", "bar_thin", "scan_small"])
def test_panel_equals_its_columns_one_at_a_time(ctx, name):
    """B applied to a panel equals B applied to each of its columns alone -- bit for bit, with either smoother precision, on these three
    meshes (measured): every kernel of the cycle computes a column from that column alone, in an order that does not depend on the width."""
    s, h, host = _problem(ctx, name)
    X = _panel(s.n, 12, 7)
    for prec in CASES[name][2]:
        whole = lab.precondition(s, X, prec)
        cols = np.column_stack([lab.precondition(s, X[:, [j]], prec)[:, 0] for j in range(X.shape[1])])
        err = _colrel(cols, whole)
        print("WIDTH %s prec %d err %.3e bitwise %s" % (name, prec, err, np.array_equal(cols, whole)))
        assert np.array_equal(cols, whole), err
