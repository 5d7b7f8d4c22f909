"""CPU-side checks of junction groups (MH_JUNCTION_SHARED, include/modalhip.h): every layer declares the flag and the group size, the
scalar solve of a group's step 4 -- the per-subset inverses by elimination without pivoting, the consistent subset of lowest mask -- agrees
with exact enumeration in numpy.longdouble within a stated number of eps, never pulls on a unilateral member and has no jump where the
active set changes, and the restatement the GPU tests trust (tests/group_harness.py) agrees with closed forms on two modes."""
import os
import re

import numpy as np
import pytest

from tests import group_harness as gh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_mirror_and_binding_carry_the_shared_flag():
    header = open(os.path.join(ROOT, "include", "modalhip.h")).read()
    assert re.search(r"#define\s+MH_JUNCTION_SHARED\s+4u", header) and re.search(r"#define\s+MH_JUNCTION_GROUP\s+4\b", header)
    from mesheditor_amd import _lib, bank
    assert bank.JUNCTION_SHARED == 4 and _lib.JUNCTION_SHARED == 4 and _lib.JUNCTION_GROUP == 4 and gh.GROUP == 4
    a = (3, 2, (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 2.0)
    assert bank.Junction.of(a, None, 5.0).flags == 0
    assert bank.Junction.of(a, None, 5.0, shared=True).flags == 4
    assert bank.Junction.of(a, None, 5.0, bilateral=True, shared=True).flags == 5
    assert bank.Junction.of(a, None, 5.0, hertz=True, shared=True).flags == 6
    assert gh.record(gh.spec(gh.side(3, 2), None, 5.0)).flags == 4 and gh.record(gh.spec(gh.side(3, 2), None, 5.0, shared=False)).flags == 0
    assert gh.record((gh.side(3, 2), None, 5.0, True)).flags == 1  # a spec of tests/junction_harness.py: unflagged
    mirror = open(os.path.join(ROOT, "mesheditor_amd", "cpp", "include", "modal", "bank.hpp")).read()
    assert re.search(r"ModalJunctionShared\{4\}", mirror)  # (its value is held by the static_assert of tests/cpp/modal_group_test.cpp)


# ---- the scalar solve alone ----
# The largest deviation of the working-precision tree's f from the longdouble solution over the cases below, in eps of the format, relative
# to max|f| of the case.  Measured here (this file prints it): 9.6 eps in float32 (n = 3), 13.3 eps in float64 (n = 3).  Asserted with a
# margin of 2 x.
SOLVE_EPS = {np.float32: 2 * 9.6, np.float64: 2 * 13.3}
CASES = 300


def _cases(n, T, count=CASES, seed=20250118):
    """Fixed-seed random groups of n: C = diag(s) G with G a random Gram matrix (PSD) and s > 0, K_i C_ii log-uniform in 1e-3 ... 1e3,
    x of mixed signs; every number already one of format T.  Yields (x, C, K, bilateral)."""
    rng = np.random.default_rng(seed + n)
    for _ in range(count):
        V = rng.standard_normal((n, n + 1))
        G = V @ V.T
        s = 10.0 ** rng.uniform(-9, -5, n)
        C = (s[:, None] * G).astype(T)
        K = (10.0 ** rng.uniform(-3, 3, n) / np.diag(C).astype(float)).astype(T)
        x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, -3)).astype(T)
        bilateral = [bool(b) for b in rng.random(n) < 0.2]
        yield x, C, K, bilateral


@pytest.mark.parametrize("n", [2, 3, 4])
def test_exactly_one_subset_is_consistent_in_longdouble(n):
    seen = set()
    for x, C, K, bilateral in _cases(n, np.float64):
        f, masks = gh.solve_exact(x, C, K, bilateral)
        assert len(masks) == 1, (masks, x)
        assert all(f[j] >= 0 for j in range(n) if not bilateral[j])
        seen.add(masks[0])
    assert 0 in seen and (1 << n) - 1 in seen and len(seen) >= min(6, 1 << n), seen  # the empty set, the full set, and others


@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("n", [2, 3, 4])
def test_the_working_precision_tree_reaches_the_longdouble_solution(n, T):
    """f >= 0 on unilateral members; f within SOLVE_EPS eps of the longdouble solution relative to max|f|, whichever subsets the two
    precisions take -- a case in which they take different ones is a point near a boundary between two active sets, where the solution is
    continuous: no jump."""
    L, eps = np.longdouble, float(np.finfo(T).eps)
    worst, other_set, last_resort = 0.0, 0, 0
    for x, C, K, bilateral in _cases(n, T):
        sets, status = gh.prepare(C, K, bilateral, T)
        assert status == 1
        f, mask = gh.solve(x, C, K, bilateral, T, sets)
        assert f.dtype == T and np.isfinite(f).all()
        assert all(f[j] >= 0 for j in range(n) if not bilateral[j]), f
        want, masks = gh.solve_exact(x.astype(L), C.astype(L), K.astype(L), bilateral)
        other_set += mask != masks[0]
        last_resort += mask < 0
        peak = float(np.abs(want).max())
        if peak == 0:
            assert not f.any()
            continue
        worst = max(worst, float(np.abs(f.astype(L) - want).max()) / peak / eps)
    print("%s, n = %d: f within %.3g eps of the longdouble solution over %d cases (%d took another subset, %d the clamped full set)" % (T.__name__, n, worst, CASES, other_set, last_resort))
    assert worst <= SOLVE_EPS[T], worst


@pytest.mark.parametrize("n", [2, 3, 4])
def test_the_force_has_no_jump_where_the_active_set_changes(n):
    """Along a straight line in x the active set changes several times; the solution of the complementarity problem is continuous and
    piecewise linear, so a step dx moves f by at most max_A ||diag(K_A) M_A||_inf |dx|_inf (and a few eps of |f| of rounding)."""
    T, L = np.float64, np.longdouble
    walked = 0
    for (x0, C, K, bilateral), (x1, _, _, _) in zip(_cases(n, T, 12, 7), _cases(n, T, 12, 8)):
        bilateral = [False] * n
        sets, status = gh.prepare(C, K, bilateral, T)
        assert status == 1
        slope = max(float(np.abs(K.astype(L)[:, None] * M.astype(L)).sum(axis=1).max()) for _, M in sets)
        steps = 400
        scale = float(np.abs(x0).max() / np.abs(x1).max())
        path = [((1 - t) * x0 - t * x1 * scale).astype(T) for t in np.linspace(0, 1, steps)]
        solved = [gh.solve(x, C, K, bilateral, T, sets) for x in path]
        masks = [m for _, m in solved]
        walked += len(set(masks)) > 1
        for (fa, _), (fb, _), xa, xb in zip(solved, solved[1:], path, path[1:]):
            jump, step = float(np.abs(fb - fa).max()), float(np.abs(xb - xa).max())
            assert jump <= slope * step * (1 + 1e-9) + 1e-10 * float(np.abs(fa).max()), (jump, slope * step, masks)
    assert walked >= 6, walked


@pytest.mark.parametrize("n", [2, 3, 4])
def test_two_precisions_that_take_different_subsets_agree(n):
    """Cases moved onto a boundary between two active sets (bisection along the segment from x to -|x|, where the group is open, to the
    last bit of float64), then rounded to float32: there the float32 tree and the longdouble enumeration may take different subsets, and
    some do (asserted).  f still deviates by no more than SOLVE_EPS eps of the size of the force at the segment's start."""
    T, L = np.float32, np.longdouble
    eps, differ, worst = float(np.finfo(T).eps), 0, 0.0
    for x, C, K, bilateral in _cases(n, np.float32, 240, 99):
        bilateral = [False] * n
        x64, C64, K64 = x.astype(np.float64), C.astype(np.float64), K.astype(np.float64)
        sets64, _ = gh.prepare(C64, K64, bilateral, np.float64)
        f0, m0 = gh.solve(x64, C64, K64, bilateral, np.float64, sets64)
        if m0 == 0:
            continue
        lo, hi = 0.0, 1.0  # the mask at lo is m0, at hi it is another
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            _, m = gh.solve((1 - mid) * x64 - mid * np.abs(x64), C64, K64, bilateral, np.float64, sets64)
            lo, hi = (mid, hi) if m == m0 else (lo, mid)
        at = ((1 - hi) * x64 - hi * np.abs(x64)).astype(T)
        f, mask = gh.solve(at, C, K, bilateral, T)
        want, masks = gh.solve_exact(at.astype(L), C.astype(L), K.astype(L), bilateral, every=False)
        differ += mask != masks[0]
        assert all(f[j] >= 0 for j in range(n))
        worst = max(worst, float(np.abs(f.astype(L) - want).max()) / float(np.abs(f0).max()) / eps)
    print("n = %d: on a boundary %d cases took another subset than longdouble; f within %.3g eps" % (n, differ, worst))
    assert differ >= 2, differ
    assert worst <= SOLVE_EPS[T], worst


@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("n", [2, 3, 4])
def test_the_kernels_lane_layout_is_the_headers_tree(n, T):
    """The kernel keeps one matrix per lane (rows of M_A on the subset, rows of C off it), eliminates in place and forms y for every
    member, also off the subset: group_harness.lane_solve restates that layout, and it must give the bits of group_harness.solve -- the
    header's tree -- on random cases and on cases moved onto a boundary between two active sets, where no subset is consistent and the
    least-failing one is clamped: there a member outside the taken subset has f = +0 (its y is a product with a row of C, not a
    displacement), which is what this test is for."""
    resorts, off_subset = 0, 0
    for x, C, K, bilateral in _cases(n, T, 240, 99):
        f, mask = gh.solve(x, C, K, bilateral, T)
        g, lane = gh.lane_solve(x, C, K, bilateral, T)
        assert lane == mask and np.array_equal(f, g) and not (np.signbit(g) & (g == 0)).any(), (mask, lane, f, g)
        plain = [False] * n
        x64, C64, K64 = x.astype(np.float64), C.astype(np.float64), K.astype(np.float64)
        sets64, _ = gh.prepare(C64, K64, plain, np.float64)
        _, m0 = gh.solve(x64, C64, K64, plain, np.float64, sets64)
        if m0 == 0:
            continue
        lo, hi = 0.0, 1.0
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            _, m = gh.solve((1 - mid) * x64 - mid * np.abs(x64), C64, K64, plain, np.float64, sets64)
            lo, hi = (mid, hi) if m == m0 else (lo, mid)
        for edge in (lo, hi):
            at = ((1 - edge) * x64 - edge * np.abs(x64)).astype(T)
            f, mask = gh.solve(at, C, K, plain, T)
            g, lane = gh.lane_solve(at, C, K, plain, T)
            assert lane == mask and np.array_equal(f, g), (mask, lane, f, g)
            if mask < 0:
                resorts += 1
                outside = [j for j in range(n) if not (-1 - mask) >> j & 1]
                off_subset += len(outside)
                assert all(g[j] == 0 and not np.signbit(g[j]) for j in outside)
    print("%s, n = %d: %d boundary cases took the last resort, %d members outside the taken subset" % (T.__name__, n, resorts, off_subset))
    if n >= 3:  # (in a group of two the boundary cases' last resort is the full set: nobody is outside it)
        assert resorts >= 2 and off_subset >= 1, (resorts, off_subset)


def test_a_group_out_of_contact_gives_exact_zeros():
    for T in (np.float32, np.float64):
        for x, C, K, _ in _cases(3, T, 20):
            f, mask = gh.solve(-np.abs(x), C, K, [False] * 3, T)
            assert mask == 0 and not f.any() and not np.signbit(f).any()
            f, mask = gh.solve(np.zeros(3, T), C, K, [False] * 3, T)
            assert mask == 0 and not f.any()


def test_a_group_that_would_amplify_is_refused():
    """A negative coupling makes a C_ii negative; with K_i C_ii <= -1 the pivot of {i} is not above 0: status 2.  Numbers that are not
    finite refuse too."""
    T = np.float32
    C = np.array([[2e-6, 1e-6], [1e-6, -3e-6]], T)
    assert gh.prepare(C, np.array([1e5, 1e5], T), [False, False], T)[1] == 1
    assert gh.prepare(C, np.array([1e5, 1e6], T), [False, False], T)[1] == 2
    assert gh.prepare(C, np.array([1e5, np.inf], T), [False, False], T)[1] == 2
    assert gh.prepare(np.array([[2e-6, np.nan], [1e-6, 3e-6]], T), np.array([1e5, 1e5], T), [False, False], T)[1] == 2
    # a subset that is not admissible plays no part: with member 1 bilateral, {0} alone is never formed, {1} and {0, 1} are
    assert [m for m, _ in gh.prepare(C, np.array([1e5, 1e5], T), [False, True], T)[0]] == [2, 3]


# ---- the restatement on two modes ----
class _TwoModes:
    """One object, two modes, four points: the columns a Scene would return."""
    c = (0.875 + 0.3125j, 0.75 + 0.5j)  # (binary fractions: the same numbers in every format)
    rad, defl, defl_scale = (2.0, 1.5), (0.25, 0.5), 0.5
    shape_x = [0.125, 0.5, 0.25, -0.25, 0.5, 0.125, 0.75, 0.25]  # [point][mode]
    shape_y = [0.375, 0.25, -0.125, 0.5, 0.0625, -0.5, 0.25, 0.125]
    shape_z = [0.0, 0.125, 0.5, 0.25, -0.25, 0.375, 0.125, -0.125]

    def column(self, name):
        table = {"CoeffRe": [v.real for v in self.c], "CoeffIm": [v.imag for v in self.c], "RadiationGain": self.rad, "DeflectionGain": self.defl, "OutPhaseRe": [0.0, 0.0],
                 "OutPhaseIm": [1.0, 1.0], "ShapeX": self.shape_x, "ShapeY": self.shape_y, "ShapeZ": self.shape_z, "OutGain": [1.0], "ListenerGain": [1.0],
                 "DeflectionScale": [self.defl_scale]}
        return np.asarray(table[name], float)


def _pair(stiffness, bilateral):
    return [gh.spec(gh.side(0, 1, direction=(1.0, 0.5, 0.0), coupling=2.0), None, stiffness[0], bilateral),
            gh.spec(gh.side(0, 2, direction=(0.25, -1.0, 0.5), coupling=3.0), None, stiffness[1], bilateral)]


@pytest.mark.parametrize("dtype", [np.longdouble, np.float64, np.float32])
def test_a_bilateral_pair_on_two_modes_is_the_closed_form(dtype):
    """Two exciter junctions on one two-mode object at rest, both bilateral: C is the 2 x 2 matrix of the gains' products, the first frame's
    forces are the solution of the 2 x 2 system (I + C diag(K)) y = u by Cramer's rule, f = K y, and in every frame each force meets its
    law at the next frame's displacement: f_i[s] = K_i (u_i[s] - read1_i[s])."""
    s, frames = _TwoModes(), 16
    r = gh.Restatement(s, [2], dtype, np.float64)
    sides = [sp[0] for sp in _pair([0, 0], True)]
    a, g_re = [r.side_gains(sd)[0].astype(float) for sd in sides], [r.side_gains(sd)[2].astype(float) for sd in sides]
    C = np.array([[float(np.sum(g_re[i] * a[j])) for j in range(2)] for i in range(2)])
    assert (np.diag(C) != 0).all() and C[0, 1] != 0
    K = [float(np.float32(4.0 / abs(C[0, 0]))), float(np.float32(0.5 / abs(C[1, 1])))]
    specs = _pair(K, True)
    t = np.arange(frames)
    u = np.array([1e-3 * np.cos(0.4 * t), -2e-3 * np.sin(0.3 * t + 1.0)], np.float32)
    trace = {}
    out, forces, comp, status = r.render_grouped([], specs, u, frames, trace)
    assert list(status) == [1, 1]
    tol = 256 * max(float(np.finfo(dtype).eps), float(np.finfo(np.float64).eps))
    assert np.abs(comp - np.diag(C)).max() <= tol * np.abs(C).max()
    b00, b01, b10, b11 = 1 + C[0, 0] * K[0], C[0, 1] * K[1], C[1, 0] * K[0], 1 + C[1, 1] * K[1]
    det = b00 * b11 - b01 * b10
    y = [(b11 * float(u[0, 0]) - b01 * float(u[1, 0])) / det, (b00 * float(u[1, 0]) - b10 * float(u[0, 0])) / det]
    for i in range(2):
        assert abs(float(forces[i, 0]) - K[i] * y[i]) <= tol * max(abs(K[j] * y[j]) for j in range(2)), i
        law = K[i] * (u[i].astype(float) - np.asarray(trace["read1"][i], float))
        assert np.abs(np.asarray(forces[i], float) - law).max() <= 64 * tol * np.abs(law).max(), i
    assert (np.asarray(forces) < 0).any() and np.abs(out).max() > 0  # bilateral: it pulls too


@pytest.mark.parametrize("dtype", [np.longdouble, np.float32])
def test_a_unilateral_pair_on_two_modes_never_pulls_and_meets_its_law(dtype):
    s, frames = _TwoModes(), 48
    r = gh.Restatement(s, [2], dtype, np.float64)
    C = r.compliance_matrix(_pair([0, 0], False)).astype(float)
    specs = _pair([3.0 / abs(C[0, 0]), 20.0 / abs(C[1, 1])], False)
    t = np.arange(frames)
    u = np.array([1e-3 * np.cos(0.4 * t), -2e-3 * np.sin(0.3 * t + 1.0)], np.float32)
    trace = {}
    _, forces, _, status = r.render_grouped([], specs, u, frames, trace)
    assert list(status) == [1, 1] and (forces >= 0).all()
    assert len(set(trace["sets"].tolist())) >= 3, set(trace["sets"].tolist())
    tol = 4096 * float(np.finfo(np.float32 if dtype == np.float32 else np.float64).eps)
    for i in range(2):
        k = float(np.float32(specs[i][2]))
        law = k * np.maximum(u[i].astype(float) - np.asarray(trace["read1"][i], float), 0)
        assert np.abs(np.asarray(forces[i], float) - law).max() <= tol * np.abs(np.asarray(forces, float)).max(), i
