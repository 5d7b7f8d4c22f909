"""Helpers of the contact-damping tests (tests/test_bank_damped_cpu.py, tests/test_bank_damped_gpu.py): junction records with the law and
damping fields, the scalar solves of step 4d of the junction contract (include/modalhip.h, MH_JUNCTION_DAMPED), their yardstick (bisection
in numpy.longdouble), and tests/hertz_harness.Restatement with that step and the carry, in a number format of the caller's choice:

  numpy.longdouble               the reference: the header's trees with Newton's iteration run to a fixed point (EXACT_STEPS steps);
  numpy.float32 / numpy.float64  the WORKING-PRECISION restatement: the header's trees with every operation rounded to the bank's format,
                                 six Newton steps, nothing contracted.  Its deviation from the longdouble one is the yardstick the device's
                                 deviation is measured by."""
import numpy as np

from tests import hertz_harness as hh
from tests import junction_harness as jh

POINTS = hh.POINTS
NO_OBJECT = hh.NO_OBJECT
side = hh.side
replay_drives = hh.replay_drives
row_figure = hh.row_figure
STEPS, EXACT_STEPS = 6, 200
_QUIET = dict(over="ignore", under="ignore", divide="ignore", invalid="ignore")


def spec(a, b=None, stiffness=0.0, bilateral=False, hertz=False, damped=True):
    """A junction as plain data: (side a, side b or None, K as the float the record holds, bilateral, hertz, damped)."""
    return (a, b, float(np.float32(stiffness)), bool(bilateral), bool(hertz), bool(damped))


def _six(s):
    return tuple(s) + (False,) * (6 - len(s))


def record(s):
    """The binding's Junction record of a spec (also of a 4- or 5-tuple of the junction and Hertz harnesses)."""
    from mesheditor_amd import bank as hipbank
    a, b, k, bilateral, hertz, damped = _six(s)
    return hipbank.Junction.of(a, b, k, bilateral, hertz, damped=damped)


def records(specs):
    from mesheditor_amd import bank as hipbank
    return (hipbank.Junction * len(specs))(*[record(s) for s in specs]) if specs else []


def _min(a, b):
    """The header's min: b < a ? b : a."""
    return np.where(b < a, b, a)


def damped_solve(x, c, l, yp, k, T, hertz, steps=None, start_factor=1.0):
    """(f, y) of step 4d by the header's trees in format T, element by element over arrays (or scalars): the force and the compression
    the solve leaves.  l = 0 and yp = 0 are what a frame without history passes.  steps: Newton steps of the Hertz tree (default: six in
    a working precision, EXACT_STEPS in longdouble); start_factor scales the Hertz start value (what device exp2 / log2 / cbrt that are
    not correctly rounded would do)."""
    x, c, l, yp, k = (np.asarray(v, T) for v in (x, c, l, yp, k))
    x, c, l, yp, k = np.broadcast_arrays(x, c, l, yp, k)
    if steps is None:
        steps = EXACT_STEPS if T == np.longdouble else STEPS
    one = T(1)
    with np.errstate(**_QUIET):
        cl = c * l
        solve = (x > 0) & (one + l * (x - yp) > 0)
        xs = np.where(solve, x, one)  # (lanes that are not solved compute something harmless)
        m0 = one - l * yp
        if not hertz:
            b = one + c * m0
            r = np.sqrt(b * b + (T(4) * cl) * xs)
            y = _min(xs, np.where(b >= 0, (T(2) * xs) / (b + r), (r - b) / (T(2) * cl)))
            m = one + l * (y - yp)
            m = np.where(m > 0, m, T(0))
            f = (k * y) * m
        else:
            big = T(np.finfo(T).max)
            c15 = T(1.5) * c
            p5 = np.where(cl > 0, np.exp2(T(0.4) * np.log2(xs / cl)), big) * T(start_factor)
            cm = c * m0
            t = np.cbrt(xs / cm) * T(start_factor)
            g = np.where(cm > 0, t * t, big)
            above = _min(_min(xs, g), p5)
            ylo = -m0 / l
            lin = xs / ((cl * ylo) * np.sqrt(ylo))
            below = _min(xs, ylo + _min(lin, p5))
            y = np.where(m0 >= 0, above, below)
            for _ in range(steps):
                r = np.sqrt(y)
                m = one + l * (y - yp)
                q = (c * y) * r
                y = y - ((y + q * m) - xs) / ((one + (c15 * r) * m) + q * l)
            m = one + l * (y - yp)
            m = np.where(m > 0, m, T(0))
            f = ((k * y) * np.sqrt(y)) * m
        f, y = np.where(solve, f, T(0)), np.where(solve, y, x)
    assert f.dtype == T and y.dtype == T
    return f[()], y[()]


def damped_step(x, c, c15, cl, l, yp, k, T, hertz, steps):
    """damped_solve for scalars of format T with Python branches (the restatement's frame loop): the same bits."""
    zero, one = T(0), T(1)
    if not x > 0:
        return zero, x
    if not one + l * (x - yp) > 0:
        return zero, x
    with np.errstate(**_QUIET):
        m0 = one - l * yp
        if not hertz:
            b = one + c * m0
            r = np.sqrt(b * b + (T(4) * cl) * x)
            y = (T(2) * x) / (b + r) if b >= 0 else (r - b) / (T(2) * cl)
            y = y if y < x else x
            m = one + l * (y - yp)
            if not m > 0:
                m = zero
            return (k * y) * m, y
        lo = lambda a, b: b if b < a else a
        big = T(np.finfo(T).max)
        p5 = np.exp2(T(0.4) * np.log2(x / cl)) if cl > 0 else big
        if m0 >= 0:
            cm = c * m0
            t = np.cbrt(x / cm) if cm > 0 else big
            y = lo(lo(x, t * t if cm > 0 else big), p5)
        else:
            ylo = -m0 / l
            y = lo(x, ylo + lo(x / ((cl * ylo) * np.sqrt(ylo)), p5))
        for _ in range(steps):
            r = np.sqrt(y)
            m = one + l * (y - yp)
            q = (c * y) * r
            y = y - ((y + q * m) - x) / ((one + (c15 * r) * m) + q * l)
        m = one + l * (y - yp)
        if not m > 0:
            m = zero
        return ((k * y) * np.sqrt(y)) * m, y


def law(y, yp, l, k, hertz, T=np.longdouble):
    """f = K phi(y) max(1 + l (y - y_p), 0) in format T."""
    y, yp, l, k = (np.asarray(v, T) for v in (y, yp, l, k))
    with np.errstate(**_QUIET):
        reach = np.maximum(y, 0)
        phi = reach * np.sqrt(reach) if hertz else reach
        return (k * phi * np.maximum(T(1) + l * (y - yp), 0))[()]


def bisected(x, c, l, yp, k, hertz, rounds=160):
    """(f*, y*) of the law in longdouble by bisection of g(y) = y + c phi(y) max(1 + l (y - y_p), 0) - x: for x > 0 and
    m_x = 1 + l (x - y_p) > 0 the root lies in (max(0, y_p - 1/l), x] (g is increasing, g(x) >= 0, and g is below 0 at 0 and at the kink);
    otherwise f* = 0 and y* = x.  The interval is halved geometrically where its lower end is 0, so that a root many decades below x
    is found to the format's relative precision."""
    L = np.longdouble
    x, c, l, yp, k = np.broadcast_arrays(*(np.asarray(v, L) for v in (x, c, l, yp, k)))
    with np.errstate(**_QUIET):
        solve = (x > 0) & (L(1) + l * (x - yp) > 0)
        xs = np.where(solve, x, L(1))
        kink = np.where(l > 0, yp - L(1) / np.where(l > 0, l, L(1)), -np.inf)
        lo = np.maximum(kink, L(0))
        hi = xs.copy()
        g = lambda y: y + c * (y * np.sqrt(y) if hertz else y) * np.maximum(L(1) + l * (y - yp), 0) - xs
        tiny = xs * L(2) ** -400
        lo = np.maximum(lo, tiny)  # (g(tiny) < 0: c phi(tiny) m is far below x)
        for _ in range(rounds):
            mid = np.where(lo > L(0.5) * hi, L(0.5) * (lo + hi), np.sqrt(lo * hi))
            up = g(mid) > 0
            hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
        y = L(0.5) * (lo + hi)
    return np.where(solve, law(y, yp, l, k, hertz), L(0)), np.where(solve, y, x)


class Restatement(hh.Restatement):
    """tests/hertz_harness.Restatement with render_damped: specs with a law and a damping field (this module's spec; shorter tuples of the
    other harnesses are undamped), step 4d for a damped junction, and the carry."""

    steps = None  # Newton steps of a damped Hertz junction (None: the format's default); hertz_harness's `steps` of an undamped one

    def render_damped(self, rows, junctions, approach, damping, carry, frames, trace=None):
        """As hh.Restatement.render_coupled, plus damping: l per junction and frame (float32, as mh_bank_render_damped takes it), and carry:
        one value per junction (None: no history).  Returns (out, forces, compliances, statuses, carry).  Statuses of a damped junction: 0
        with bilateral or with an l that is not finite or below 0 (left out: a zero row, C = 0), 2 when C < 0 or C, K C or K C l is not
        finite.  trace also receives "y": the compression each solved damped junction's solve left, [junction][frame]."""
        T = self.T
        exact = T == np.longdouble
        total = np.sum if exact else jh._sequential
        junctions = [_six(s) for s in junctions]
        n = len(junctions)
        out, forces = np.zeros(frames, T), np.zeros((n, frames), T)
        u = np.asarray(approach, np.float32).reshape(n, frames)
        u = np.where(np.isfinite(u), u, np.float32(0)).astype(T)
        lam = [T(v) for v in np.asarray(damping, np.float32).reshape(n)]
        came = np.full(n, np.nan, T) if carry is None else np.asarray(carry, T).reshape(n)
        mine = [[(self.drive_gain(o, p, d), np.asarray(f, np.float32).astype(T)) for (obj, p, d, f) in rows if obj == o] for o in range(len(self.objects))]
        gains = [[(sd[0],) + self.side_gains(sd) for sd in (s[0], s[1]) if sd is not None] for s in junctions]
        comp = [self.compliance(s[:4]) for s in junctions]
        stiff = [T(np.float32(s[2])) for s in junctions]
        status = []
        with np.errstate(**_QUIET):
            kc = [k * c for k, c in zip(stiff, comp)]
            kcl = [v * l for v, l in zip(kc, lam)]
            denom = [T(1) + v for v in kc]
        ok = lambda v: bool(np.isfinite(v) and v >= 0)
        for j, s in enumerate(junctions):
            if (s[4] and s[3]) or (s[5] and (s[3] or not ok(lam[j]))):
                status.append(0)
                comp[j] = T(0)
            elif s[5]:
                status.append(1 if ok(comp[j]) and ok(kc[j]) and ok(kcl[j]) else 2)
            elif s[4]:
                status.append(1 if ok(comp[j]) and ok(kc[j]) else 2)
            else:
                status.append(1 if (np.isfinite(denom[j]) and denom[j] > 0) else 2)
        steps = self.steps if self.steps is not None else (EXACT_STEPS if exact else STEPS)
        kc15 = [T(1.5) * v for v in kc]
        history = [bool(np.isfinite(v)) for v in came]
        y_prev = [came[j] if history[j] else T(0) for j in range(n)]
        free, after, left = np.zeros((n, frames), T), np.zeros((n, frames), T), np.full((n, frames), np.nan, T)
        for t in range(frames):
            stepped = []
            for o, ob in enumerate(self.objects):
                (z_re, z_im), c_re, c_im = self.z[o], ob["c_re"], ob["c_im"]
                e = np.zeros(len(z_re), T)
                for g, f in mine[o]:
                    e = e + f[t] * g
                stepped.append([z_re * c_re - z_im * c_im + e, z_re * c_im + z_im * c_re])
            for j, s in enumerate(junctions):
                d = total(np.concatenate([g_im * stepped[o][1] + g_re * stepped[o][0] for (o, _, g_im, g_re) in gains[j]]))
                free[j, t] = d
                if status[j] != 1:
                    continue
                x = u[j, t] - d
                if s[5]:
                    l_now, cl_now = (lam[j], kcl[j]) if history[j] else (T(0), T(0))
                    f, y = damped_step(x, kc[j], kc15[j], cl_now, l_now, y_prev[j], stiff[j], T, s[4], steps)
                    y_prev[j], history[j] = y, True
                    left[j, t] = y
                elif s[4]:
                    f = hh.hertz_force(x, kc[j], stiff[j], T, None)
                else:
                    reach = x if s[3] else (x if x > 0 else T(0))
                    f = (stiff[j] * reach) / denom[j]
                forces[j, t] = f
                for (o, a, _, _) in gains[j]:
                    stepped[o][0] = stepped[o][0] + a * f
            for j in range(n):  # what an advance-1 pickup on every side reads after the frame: the next frame's deflection
                after[j, t] = total(np.concatenate([g_im * stepped[o][1] + g_re * stepped[o][0] for (o, _, g_im, g_re) in gains[j]]))
            for o, ob in enumerate(self.objects):
                z_re, z_im = stepped[o]
                self.z[o] = (z_re, z_im)
                out[t] += ob["mix"] * np.sum(ob["p_im"] * z_im + ob["p_re"] * z_re)
        if trace is not None:
            trace["d"], trace["read1"], trace["y"] = free, after, left
        gone = np.array([y_prev[j] if (junctions[j][5] and status[j] == 1 and frames) else T(np.nan) for j in range(n)], T)
        if frames == 0 and carry is not None:
            gone = came.copy()
        return out, forces, np.array([float(c) for c in comp]), np.array(status, np.uint8), gone
