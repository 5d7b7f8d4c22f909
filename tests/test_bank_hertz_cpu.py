"""CPU-side checks of the Hertz law of the contact junctions: every layer declares the flag, the scalar solve of step 4h (four Newton steps
from the smaller of two upper bounds, include/modalhip.h) reaches the exact root's force in float32 and float64 -- and three steps do not
in float64 --, and the restatement the GPU tests trust (tests/hertz_harness.py) agrees with closed forms on one mode."""
import os
import re

import numpy as np
import pytest

from tests import hertz_harness as hh
from tests.test_bank_pickups_cpu import _OneMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_binding_and_record_carry_the_hertz_flag():
    header = open(os.path.join(ROOT, "include", "modalhip.h")).read()
    assert re.search(r"#define\s+MH_JUNCTION_HERTZ\s+2u", header) and re.search(r"#define\s+MH_JUNCTION_BILATERAL\s+1u", header)
    from mesheditor_amd import _lib, bank
    assert bank.JUNCTION_HERTZ == 2 and _lib.JUNCTION_HERTZ == 2
    a = (3, 2, (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 2.0)
    assert bank.Junction.of(a, None, 5.0).flags == 0
    assert bank.Junction.of(a, None, 5.0, hertz=True).flags == 2
    assert bank.Junction.of(a, None, 5.0, bilateral=True, hertz=True).flags == 3
    assert hh.record(hh.spec(hh.side(3, 2), None, 5.0)).flags == 2 and hh.record(hh.spec(hh.side(3, 2), None, 5.0, hertz=False)).flags == 0
    mirror = open(os.path.join(ROOT, "mesheditor_amd", "cpp", "include", "modal", "bank.hpp")).read()
    assert re.search(r"ModalJunctionHertz\{2\}", mirror)  # (its value is held by the static_assert of tests/cpp/modal_hertz_test.cpp)


# ---- the scalar solve alone ----
SOLVE_BOUND = 4  # eps, relative, on f: a condition on the algorithm (measured: 2.6 in both formats, K included)


def _grid(T, n=20000, seed=20240607):
    """c sqrt(x) log-uniform in 1e-8 ... 1e8, x in 1e-12 ... 1, K in 1e-2 ... 1e4: (x, c, K), each already a number of format T."""
    rng = np.random.default_rng(seed)
    sigma, x, k = 10.0 ** rng.uniform(-8, 8, n), 10.0 ** rng.uniform(-12, 0, n), 10.0 ** rng.uniform(-2, 4, n)
    return x.astype(T), (sigma / np.sqrt(x)).astype(T), k.astype(T)


def _worst(T, steps=None, start_factor=1.0):
    """The largest relative deviation of the working-precision f from the longdouble root's, in eps of T."""
    L = np.longdouble
    x, c, k = _grid(T)
    got = hh.hertz_force(x, c, k, T, steps, start_factor)
    want = hh.hertz_force(x.astype(L), c.astype(L), k.astype(L), L)
    assert (want > 0).all() and np.isfinite(got).all()
    return float((np.abs(got.astype(L) - want) / want).max()) / float(np.finfo(T).eps)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_four_newton_steps_reach_the_exact_roots_force(T):
    L = np.longdouble
    for x, c in ((1e-3, 1e2), (1.0, 1e-8), (1e-12, 1e14)):  # the longdouble iteration has stopped moving (to the last bit or two), at a root
        y = hh.hertz_root(L(x), L(c), L)
        assert abs(hh.hertz_root(L(x), L(c), L, hh.EXACT_STEPS + 1) - y) <= 2 * np.finfo(L).eps * y and abs((y + L(c) * y * np.sqrt(y)) - L(x)) <= 4 * np.finfo(L).eps * L(x)
    worst = _worst(T)
    print("%s: f within %.2f eps of the longdouble root's over the grid" % (T.__name__, worst))
    assert worst <= SOLVE_BOUND, worst
    for factor in (1 + 1e-3, 1 - 1e-3):  # a cube root that is off by 1e-3: the device's need not be correctly rounded
        off = _worst(T, start_factor=factor)
        print("%s: start value x %.3f: %.2f eps" % (T.__name__, factor, off))
        assert off <= SOLVE_BOUND, (factor, off)


def test_three_newton_steps_are_not_enough_in_double():
    """The step count is pinned for a reason: with three steps float64 misses the bound (float32 meets it)."""
    worst = _worst(np.float64, steps=3)
    print("float64, three steps: %.3g eps" % worst)
    assert worst > SOLVE_BOUND


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_edges_of_the_solve_are_finite(T):
    assert hh.hertz_force(0.0, 5.0, 2.0, T) == 0 and hh.hertz_force(-1.0, 5.0, 2.0, T) == 0 and hh.hertz_force(np.nan, 5.0, 2.0, T) == 0
    assert hh.hertz_root(0.25, 0.0, T) == T(0.25) and hh.hertz_force(0.25, 0.0, 2.0, T) == T(2.0) * T(0.25) * T(0.5)  # c = 0: y = x, f = K x^1.5
    for x in (1.0, 1e-6, float(np.finfo(T).tiny)):
        f = hh.hertz_force(x, 1e30, 1e3, T)
        assert np.isfinite(f) and f >= 0, (x, f)


# ---- closed forms on one mode ----
NORMAL, COUPLING, POINT = (0.25, -1.0, 0.5), 3.0, 2


def _one_mode_gains(s):
    """(a, read) of the one mode at POINT along NORMAL, in double."""
    along = s.shape_x[POINT] * NORMAL[0] + s.shape_y[POINT] * NORMAL[1] + s.shape_z[POINT] * NORMAL[2]
    return s.rad * along, COUPLING * s.defl_scale * along * s.defl


@pytest.mark.parametrize("dtype", [np.longdouble, np.float64, np.float32])
@pytest.mark.parametrize("stiffness", [0.5, 40.0, 3000.0])
def test_a_hertz_junction_on_one_mode_meets_the_law_and_its_static_limit(dtype, stiffness):
    """One mode, constant u, no other excitation.  The force of frame s is the law at the displacement of frame s + 1,
    f[s] = K max(u - read1[s], 0)^1.5 with read1 from the restatement's own trace, to 64 eps of the row's peak (met by construction: what is
    left is the rounding of the solve and of the trace's few operations); and f settles on the root of the static equation
    f = K (u - G f)^1.5, G = read a c_im / |1 - c|^2 the one-mode static compliance: a constant force f holds the mode at z = a f / (1 - c).
    The limit is compared to 64 eps x (1 + 1.5 K G sqrt(y)), the loop's static gain: what a rounding of d is divided by."""
    s, frames = _OneMode(), 1200
    r = hh.Restatement(s, [1], dtype)
    u = np.full((1, frames), 0.375, np.float32)
    junction = hh.spec(hh.side(0, POINT, direction=NORMAL, coupling=COUPLING), None, stiffness)
    trace = {}
    _, f, comp, status = r.render_coupled([], [junction], u, frames, trace)
    a, read = _one_mode_gains(s)
    assert status[0] == 1 and comp[0] > 0 and abs(comp[0] - read * s.c.imag * a) <= 4 * float(np.finfo(dtype).eps) * abs(comp[0]) + 1e-18
    eps = max(float(np.finfo(dtype).eps), float(np.finfo(np.float64).eps))
    forces, read1 = np.asarray(f[0], np.longdouble), np.asarray(trace["read1"][0], np.longdouble)
    law = np.longdouble(stiffness) * np.maximum(np.longdouble(0.375) - read1, 0) ** np.longdouble(1.5)
    peak = float(np.abs(forces).max())
    assert peak > 0 and np.isfinite(forces).all() and (forces >= 0).all()
    assert float(np.abs(forces - law).max()) <= 64 * eps * peak, (float(np.abs(forces - law).max()), peak)
    G = read * a * s.c.imag / abs(1 - s.c) ** 2
    y = float(hh.hertz_root(np.longdouble(0.375), np.longdouble(stiffness * G), np.longdouble))
    limit = stiffness * y ** 1.5
    assert abs(float(forces[-1]) - limit) <= 64 * eps * (1 + 1.5 * stiffness * G * np.sqrt(y)) * limit, (float(forces[-1]), limit)


@pytest.mark.parametrize("dtype", [np.longdouble, np.float64, np.float32])
def test_a_hertz_junction_never_pulls(dtype):
    """A contact that makes and breaks: u a slow sine around zero over a mode rung by a drive.  f >= 0 throughout, f = 0 exactly where
    x = u[s] - d <= 0 (d: the free prediction), and f > 0 elsewhere."""
    s, frames = _OneMode(), 600
    r = hh.Restatement(s, [1], dtype)
    t = np.arange(frames)
    u = (0.05 * np.sin(2 * np.pi * t / 150.0)).astype(np.float32)[None, :]
    drive = (0.3 * np.sin(0.9 * t)).astype(np.float32)
    trace = {}
    _, f, _, status = r.render_coupled([(0, 1, (1.0, 0.5, 0.0), drive)], [hh.spec(hh.side(0, POINT, direction=NORMAL, coupling=COUPLING), None, 25.0)], u, frames, trace)
    f, d = np.asarray(f[0]), np.asarray(trace["d"][0])
    open_ = u[0].astype(dtype) <= d
    assert status[0] == 1 and (f >= 0).all() and np.isfinite(f).all()
    assert 0.1 * frames < open_.sum() < 0.9 * frames  # it does make and break
    assert (f[open_] == 0).all() and (f[~open_] > 0).all()


def test_the_restatements_linear_junctions_are_the_junction_harness():
    """A spec without the law (and a 4-tuple of tests/junction_harness.py) goes through the inherited arithmetic: the same bits."""
    from tests import junction_harness as jh
    s, frames = _OneMode(), 200
    t = np.arange(frames)
    u = (0.05 * np.sin(2 * np.pi * t / 150.0)).astype(np.float32)[None, :]
    rows = [(0, 1, (1.0, 0.5, 0.0), (0.3 * np.sin(0.9 * t)).astype(np.float32))]
    sd = hh.side(0, POINT, direction=NORMAL, coupling=COUPLING)
    want = jh.Restatement(s, [1], np.float32).render_coupled(rows, [jh.spec(sd, None, 25.0)], u, frames)
    for linear in (hh.spec(sd, None, 25.0, hertz=False), jh.spec(sd, None, 25.0)):
        got = hh.Restatement(s, [1], np.float32).render_coupled(rows, [linear], u, frames)
        assert all(np.array_equal(a, b) for a, b in zip(want, got))
    other = hh.Restatement(s, [1], np.float32).render_coupled(rows, [hh.spec(sd, None, 25.0)], u, frames)
    assert not np.array_equal(other[1], want[1])


def test_a_hertz_junction_with_negative_compliance_is_refused_and_with_bilateral_left_out():
    """A negative coupling makes C negative: status 2 and a zero row whatever K is -- also where 1 + K C > 0, which the linear law solves --
    and the objects move as with K = 0.  Hertz + bilateral: status 0, C = 0, a zero row."""
    s, frames = _OneMode(), 64
    drive = (0.3 * np.sin(0.9 * np.arange(frames))).astype(np.float32)
    rows = [(0, 1, (1.0, 0.5, 0.0), drive)]
    u = np.full((1, frames), 0.25, np.float32)
    sd = hh.side(0, POINT, direction=NORMAL, coupling=-COUPLING)
    comp = hh.Restatement(s, [1], np.float64).compliance(hh.spec(sd, None, 1.0)[:4])
    assert comp < 0
    free, f0, _, status0 = hh.Restatement(s, [1], np.float64).render_coupled(rows, [hh.spec(sd, None, 0.0, hertz=False)], u, frames)
    assert status0[0] == 1 and (f0 == 0).all()
    for k in (-2.0 / comp, -0.01 / comp):
        out, f, c, status = hh.Restatement(s, [1], np.float64).render_coupled(rows, [hh.spec(sd, None, k)], u, frames)
        assert status[0] == 2 and c[0] == comp and (f == 0).all() and np.array_equal(out, free), k
    _, f_lin, _, status_lin = hh.Restatement(s, [1], np.float64).render_coupled(rows, [hh.spec(sd, None, -0.01 / comp, hertz=False)], u, frames)
    assert status_lin[0] == 1 and np.abs(f_lin).max() > 0
    good = hh.side(0, POINT, direction=NORMAL, coupling=COUPLING)
    out, f, c, status = hh.Restatement(s, [1], np.float64).render_coupled(rows, [hh.spec(good, None, 25.0, bilateral=True)], u, frames)
    assert status[0] == 0 and c[0] == 0 and (f == 0).all() and np.array_equal(out, free)
