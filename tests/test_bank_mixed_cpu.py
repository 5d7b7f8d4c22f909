"""CPU tests of step 4m, the solve of a junction group with a Hertz member (include/modalhip.h, mh_bank_render_mixed),
on the numpy restatement of tests/mixed_harness.py, and of the layers that need no device: the group decision, the header, the binding.

Case sets (mixed_harness.cases, fixed seeds): C = D G with G a random Gram matrix, a nearly rank-one one, one with two nearly opposite
rows; n = 2, 3, 4; all-Hertz groups and mixed ones; 1 000 cases each; K C_ii sqrt|x| or K C_ii = 1e-3 .. 1e3, x = +-(1e-6 .. 1).  No case
is filtered."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import group_harness as gh
from tests import mixed_harness as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = np.longdouble
COUNT = 1000
ASSERTED = 2.4  # what test_the_tree_is_within_the_margin_of_the_linear_solve asserts: twice the largest ratio measured (1.19), inside MARGIN
MARGIN = 4  # x the error of section 3e's linear solve on the linearisation: the project's margin for "same work, different order"
SETS = [(kind, n, mixed) for mixed in (False, True) for kind in mh.KINDS for n in (2, 3, 4)]
FORMATS = [np.float32, np.float64]
_CACHE = {}


def _set(kind, n, mixed, T):
    """The set's cases rounded to T, the longdouble reference on those numbers, and the yardstick."""
    key = (kind, n, mixed, T)
    if key not in _CACHE:
        x, C, K, hertz, bilateral = mh.cases(kind, n, COUNT, mixed, 7000 + 100 * int(mixed) + 10 * mh.KINDS.index(kind) + n)
        x, C, K = x.astype(T), C.astype(T), K.astype(T)
        f_ref, y_ref, res = mh.reference(x, C, K, hertz, bilateral)
        yard = mh.linearised(x, C, K, hertz, bilateral, y_ref, f_ref, T)
        _CACHE[key] = (x, C, K, hertz, bilateral, f_ref, y_ref, res, yard)
    return _CACHE[key]


def _errors(f, f_ref):
    top = np.abs(f_ref).max(axis=1)
    return (np.abs(f.astype(L) - f_ref).max(axis=1) / np.where(top > 0, top, 1)).astype(float)


@pytest.mark.parametrize("T", FORMATS, ids=["fp32", "fp64"])
def test_the_reference_reaches_its_fixed_point(T):
    for kind, n, mixed in SETS:
        x, _, _, _, _, f_ref, _, res, _ = _set(kind, n, mixed, T)
        assert len(x) >= 1000 and np.isfinite(f_ref.astype(float)).all()
        assert float(res.max()) <= 1e-15, (kind, n, mixed, float(res.max()))


@pytest.mark.parametrize("T", FORMATS, ids=["fp32", "fp64"])
def test_every_case_converges(T):
    """No case of any set fails the residual test, in either format, and every force is finite."""
    for kind, n, mixed in SETS:
        x, C, K, hertz, bilateral = _set(kind, n, mixed, T)[:5]
        f, _, bad = mh.solve(x, C, K, hertz, bilateral, T)
        assert f.dtype == T and np.isfinite(f).all()
        assert not bad.any(), (kind, n, mixed, int(bad.sum()))


def _ratios(T, steps):
    out = {}
    for kind, n, mixed in SETS:
        x, C, K, hertz, bilateral, f_ref, _, _, yard = _set(kind, n, mixed, T)
        f, _, _ = mh.solve(x, C, K, hertz, bilateral, T, steps=steps)
        err = _errors(f, f_ref)
        out[(kind, n, mixed)] = (err.max(), yard.max())
    return out


@pytest.mark.parametrize("T", FORMATS, ids=["fp32", "fp64"])
def test_the_tree_is_within_the_margin_of_the_linear_solve(T):
    """Per set: the largest |f - f*| / max |f*| against the largest error of section 3e's linear solve, in the same format, on the
    linearisations at the solutions.  The issue allows 4 x; asserted is twice the largest ratio measured (this test prints every set): 0.00 - 1.19 x over the 36 sets -- the tree is within 1.4 - 2.3 eps of max |f*| in every set, float32 and float64, where the linear solve is at 1.5 eps (random Gram matrices, n = 2) to 5 600 eps (nearly rank one); the largest ratio is the float64 random set with n = 2."""
    got = _ratios(T, mh.STEPS)
    for (kind, n, mixed), (err, yard) in got.items():
        print("%s %s n=%d %s: tree %.2e (%.1f eps), linear solve %.2e (%.1f eps), ratio %.2f" % (T.__name__, kind, n, "mixed" if mixed else "hertz", err, err / np.finfo(T).eps, yard, yard / np.finfo(T).eps, err / yard))
    for key, (err, yard) in got.items():
        assert err <= ASSERTED * yard, (key, err, yard, err / yard)


def test_one_newton_step_fewer_is_not_enough():
    """With STEPS - 1 steps (and SWEEPS sweeps) some set is outside the margin the issue allows: STEPS is the smallest count."""
    fewer = max(err / yard for T in FORMATS for err, yard in _ratios(T, mh.STEPS - 1).values())
    full = max(err / yard for T in FORMATS for err, yard in _ratios(T, mh.STEPS).values())
    assert fewer > MARGIN and fewer > full, (fewer, full)


def test_one_sweep_fewer_is_not_enough():
    """With SWEEPS - 1 Gauss-Seidel sweeps and STEPS Newton steps some set is outside the margin the issue allows, or has cases that fail
    the residual test: (SWEEPS, STEPS) is a smallest pair.  (Measured, DESIGN.md section 3h: 0, 1, 2, 3 sweeps need 13, 10, 12, 12 steps.)"""
    worst, unconverged = 0.0, 0
    for T in FORMATS:
        for kind, n, mixed in SETS:
            x, C, K, hertz, bilateral, f_ref, _, _, yard = _set(kind, n, mixed, T)
            f, _, bad = mh.solve(x, C, K, hertz, bilateral, T, sweeps=mh.SWEEPS - 1)
            err = _errors(f, f_ref)
            worst, unconverged = max(worst, float(np.where(np.isnan(err), np.inf, err).max() / yard.max())), unconverged + int(bad.sum())
    assert mh.SWEEPS >= 1 and worst > MARGIN and unconverged > 0, (worst, unconverged)


LINES, POINTS = 25, 120


@pytest.mark.parametrize("T", FORMATS, ids=["fp32", "fp64"])
def test_the_forces_are_continuous_along_a_line_in_x(T):
    """Along the line from one case's x to the next case's (C, K and the laws of the first; 120 points; the signs are mixed, so the members
    cross their kinks one after another and the tree's selects -- x > 0, g < x, [y > 0], the clamps, the sweep -- all switch on the way)
    no step of f is larger than L |dx| plus the accuracy bound at either end.  L is the Lipschitz bound of the exact solution on the
    line: f' = S = K phi' (I + C K phi')^-1 wherever it exists, so |f(b) - f(a)| <= sup |S|_2 |b - a|, the sup taken over the line's
    points from the longdouble solution.  The accuracy bound is ASSERTED x the linear solve's error of the set, per end."""
    steps_checked = 0
    for kind, n, mixed in SETS[::3]:
        x, C, K, hertz, bilateral, _, _, _, yard = _set(kind, n, mixed, T)
        t = np.linspace(0.0, 1.0, POINTS).astype(T)[None, :, None]
        xs = (x[:LINES, None, :] + t * (np.roll(x, -1, axis=0)[:LINES, None, :] - x[:LINES, None, :])).astype(T).reshape(LINES * POINTS, n)
        rep = lambda v: np.repeat(v[:LINES], POINTS, axis=0)
        Cs, Ks, hs, bs = rep(C), rep(K), rep(hertz), rep(bilateral)
        f_ref, y_ref, res = mh.reference(xs, Cs, Ks, hs, bs)
        assert float(res.max()) <= 1e-15
        f, _, bad = mh.solve(xs, Cs, Ks, hs, bs, T)
        assert not bad.any()
        _, dphi = mh.laws(y_ref.astype(np.float64), hs, bs, np.float64)
        a = Ks.astype(np.float64) * dphi
        S = a[:, :, None] * np.linalg.inv(np.eye(n)[None] + Cs.astype(np.float64) * a[:, None, :])
        lipschitz = np.linalg.norm(S, 2, axis=(1, 2)).reshape(LINES, POINTS).max(axis=1)
        f, xs64 = f.astype(np.float64).reshape(LINES, POINTS, n), xs.astype(np.float64).reshape(LINES, POINTS, n)
        top = np.abs(f_ref.astype(np.float64)).reshape(LINES, POINTS, n).max(axis=2)
        jump = np.linalg.norm(np.diff(f, axis=1), axis=2)
        reach = np.linalg.norm(np.diff(xs64, axis=1), axis=2)
        allowed = lipschitz[:, None] * reach + ASSERTED * yard.max() * np.sqrt(n) * (top[:, 1:] + top[:, :-1])
        assert (jump <= allowed).all(), (kind, n, mixed, float((jump / allowed).max()))
        assert (jump > 0).any()
        steps_checked += jump.size
    assert steps_checked == len(SETS[::3]) * LINES * (POINTS - 1)


@pytest.mark.parametrize("T", FORMATS, ids=["fp32", "fp64"])
def test_the_kernels_layout_gives_the_trees_bits(T):
    """k_bank_modes_grouped's step 4m runs the tree on the group padded to four members (K = 0, C = 0, x = 0), the same in every lane."""
    for kind, n, mixed in SETS:
        x, C, K, hertz, bilateral = _set(kind, n, mixed, T)[:5]
        f, y, bad = mh.solve(x[:200], C[:200], K[:200], hertz[:200], bilateral[:200], T)
        fp, yp, badp = mh.solve(x[:200], C[:200], K[:200], hertz[:200], bilateral[:200], T, pad=True)
        assert np.array_equal(f, fp) and np.array_equal(y, yp) and np.array_equal(bad, badp)


@pytest.mark.parametrize("T", FORMATS, ids=["fp32", "fp64"])
def test_degenerate_inputs(T):
    x, C, K, hertz, bilateral = _set("gram", 3, True, T)[:5]
    f, _, _ = mh.solve(x, C, K, hertz, bilateral, T)
    assert (f[~bilateral] >= 0).all()
    # every x_j <= 0 (no bilateral member): exact zeros
    hz = np.ones_like(hertz)
    f, _, bad = mh.solve(-np.abs(x), C, K, hz, ~hz, T)
    assert not f.any() and not bad.any()
    # x = 0, C = 0 and K C_ii = 1e30: finite wherever the group is solved (in float32 1e30 is beyond the range the header states for
    # C_ij K_j, and every such group is refused; in float64 every one is solved)
    for xs, Cs, Ks, solved in ((np.zeros_like(x), C, K, 1.0), (x, np.zeros_like(C), K, 1.0), (x, C, (T(1e30) / np.einsum("nii->ni", C)).astype(T), 0.0 if T == np.float32 else 1.0)):
        f, y, _ = mh.solve(xs, Cs, Ks, hertz, bilateral, T)
        kept = mh.status(Cs, Ks, hertz, T) == 1
        assert kept.mean() == solved
        assert np.isfinite(f[kept]).all() and np.isfinite(y[kept]).all()


@pytest.mark.parametrize("T", FORMATS, ids=["fp32", "fp64"])
def test_a_start_that_is_off_changes_the_result_within_the_margin(T):
    """cbrt need not be correctly rounded: a cube root off by +-1e-3 moves f by no more than the accuracy bound asserted above."""
    for kind, n, mixed in SETS[::4]:
        x, C, K, hertz, bilateral, f_ref, _, _, yard = _set(kind, n, mixed, T)
        plain, _, _ = mh.solve(x, C, K, hertz, bilateral, T)
        top = np.abs(f_ref).max(axis=1).astype(float)
        for offset in (1e-3, -1e-3):
            f, _, bad = mh.solve(x, C, K, hertz, bilateral, T, offset=offset)
            change = (np.abs(f.astype(L) - plain.astype(L)).max(axis=1).astype(float) / np.where(top > 0, top, 1)).max()
            assert not bad.any() and change <= ASSERTED * yard.max(), (kind, n, mixed, offset, change, yard.max())


# ---- the group decision ----
def _decision():
    """include/modalhip_groups.hpp's add(), compiled into a small shared object by the C++ compiler the host mirror is built with."""
    import subprocess
    import tempfile
    src = '#include "modalhip_groups.hpp"\nextern "C" int decide(unsigned n, const unsigned *f, const unsigned *a, const unsigned *b, int in_groups, int *kept) {\n' \
          '    MhJunctionGroups g(16);\n    for (unsigned j = 0; j < n; ++j) kept[j] = g.add(j, f[j], a[j], 1, b[j], 1, in_groups != 0);\n    return 0;\n}\n' \
          'extern "C" int decide_default(unsigned n, const unsigned *f, const unsigned *a, const unsigned *b, int *kept) {\n' \
          '    MhJunctionGroups g(16);\n    for (unsigned j = 0; j < n; ++j) kept[j] = g.add(j, f[j], a[j], 1, b[j], 1);\n    return 0;\n}\n'
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "decide.cpp"), "w") as fh:
        fh.write(src)
    so = os.path.join(d, "decide.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), os.path.join(d, "decide.cpp"), "-o", so])
    return ctypes.CDLL(so)


def test_the_group_decision_with_and_without_the_parameter():
    lib = _decision()
    NO, BIL, HZ, SH, DMP = 0xFFFFFFFF, 1, 2, 4, 8

    def decide(junctions, in_groups=None):
        n = len(junctions)
        arr = lambda k: (ctypes.c_uint * n)(*[j[k] for j in junctions])
        kept = (ctypes.c_int * n)()
        if in_groups is None:
            lib.decide_default(n, arr(0), arr(1), arr(2), kept)
        else:
            lib.decide(n, arr(0), arr(1), arr(2), int(in_groups), kept)
        return [k >= 0 for k in kept]

    hub = [(SH, 1, 0), (SH | HZ, 1, 2), (SH | HZ, 1, NO)]
    assert decide(hub) == decide(hub, False) == [True, False, False]
    assert decide(hub, True) == [True, True, True]
    assert decide([(SH | HZ, 1, 0), (SH, 1, 2)], True) == [True, True] and decide([(SH | HZ, 1, 0), (SH, 1, 2)]) == [True, False]
    # every other left-out kind is what it was, with the parameter and without
    for flag in (None, False, True):
        assert decide([(SH | HZ, 1, 0), (SH | DMP, 1, 2)], flag) == [True, False]  # a damped junction in a group
        assert decide([(SH | DMP, 1, 0), (SH | HZ, 1, 2)], flag) == [True, False]
        assert decide([(SH, 0, NO)] * 5, flag) == [True] * 4 + [False]  # a fifth member
        assert decide([(SH | HZ, 0, NO)] * 5, flag) == ([True] * 4 + [False] if flag else [True] + [False] * 4)
        assert decide([(0, 1, 0), (SH | HZ, 1, 2)], flag) == [True, False]  # a flagged junction on an unflagged junction's object
        assert decide([(SH, 1, 0), (HZ, 1, 2)], flag) == [True, False]  # an unflagged one on a kept junction's object
    assert BIL == 1  # (Hertz with bilateral is refused ahead of the decision, by RenderBlock and the C entry)


# ---- header, export, binding ----
def test_the_entry_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "modalhip.h")).read()
    assert re.search(r"int mh_bank_render_mixed\(mh_bank \*,[^;]*uint32_t \*unconverged_out\);", header)
    assert "4m" in header and "Hertz junctions in groups" in header
    observed = re.search(r"int mh_bank_render_observed\(([^;]*)\);", header).group(1)
    mixed = re.search(r"int mh_bank_render_mixed\(([^;]*)\);", header).group(1)
    squeeze = lambda s: re.sub(r"\s+", " ", s)
    assert squeeze(mixed) == squeeze(observed) + ", uint32_t *unconverged_out"
    assert "RenderModalMixed" in open(os.path.join(ROOT, "mesheditor_amd", "cpp", "include", "modal", "bank.hpp")).read()
    assert "mhx_render_mixed" in open(os.path.join(ROOT, "mesheditor_amd", "cpp", "src", "capi.cpp")).read()
    from mesheditor_amd import bank as hipbank
    assert hasattr(hipbank.Scene, "render_mixed")
    lib_path = os.path.join(ROOT, "mesheditor_amd", "libmodalhip.so")
    if os.path.exists(lib_path):
        import subprocess
        symbols = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True).stdout
        assert " mh_bank_render_mixed" in symbols and " mh_bank_render_observed" in symbols
